"""GPU: Camera.get_img_from_pano on the HIP path (gclm_render_from_pano) against float64 grid_sample, per pixel.

Gate (tests/pano_gate.py, checked on CPU by test_pano_abi.py): |out - ref| <= L delta_p + 4 ulp(A), delta_p the atan2-
conditioned coordinate bound with kappa derived per case from float32 against float64 at that case's shapes and cameras."""
import os

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from geocalib_amd import camera_models
from geocalib_amd.gravity import Gravity
import pano_gate as pg
import undistort_gate as ug

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_pano.npz")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def render(model, cams, rolls, pitches, yaws, pano, resize_factor=None):
    g = Gravity.from_rp(rolls.to(cams.device), pitches.to(cams.device))
    return camera_models[model](cams).get_img_from_pano(pano, g, yaws.to(cams.device), resize_factor)


def device_rotations(rolls, pitches, yaws, dev):
    """The R_i the method hands to the kernel: computed on the device, as the method does.  Near a pole the roll of
    Gravity.R is ill-conditioned (1 - g_z^2 cancels), so a CPU R_i may differ from it by far more than an ulp's effect."""
    return pg.rotations(rolls.to(dev), pitches.to(dev), yaws.to(dev)).cpu()


@pytest.mark.parametrize("case", pg.CASES, ids=[f"{c[0]}-{c[1]}-n{c[2]}-nb{c[3]}-C{c[4]}-{c[5]}x{c[6]}-p{c[11]}-y{c[12]}"
                                                 for c in pg.CASES])
def test_parity_against_float64(dev, case):
    model, H, W = case[0], case[5], case[6]
    cams, _, pano, yaws, rolls, pitches = pg.case_inputs(case)
    out = render(model, cams.to(dev), rolls, pitches, yaws, pano[0].to(dev))
    torch.cuda.synchronize()
    assert out.shape == (case[2], case[4], H, W) and out.dtype == torch.float32 and out.device == dev
    ys = pg.Yardstick(model, cams, device_rotations(rolls, pitches, yaws, dev), H, W, pano.to(dev, torch.float64))
    ratio = ys.worst_ratio(out)
    print(f"{case}: kappa {ys.kappa:.2f}, seam pixels {int(ys.seam.sum())}, worst ratio to the gate {ratio:.3f}")
    assert ratio <= 1, ratio


def _resized(pano, shape, mode):
    return F.interpolate(pano, size=shape, mode=mode).clamp(pano.min(), pano.max())


@pytest.mark.parametrize("model", pg.MODELS)
@pytest.mark.parametrize("resize", [False, True], ids=["plain", "resize"])
def test_golden_reference_outputs(dev, model, resize):
    """The reference's own CPU float32 outputs: both sides are float32 evaluations of the float64 yardstick, so the gate
    doubles; with resize_factor, the device resize may differ from the CPU one by D (measured here), which bilinear
    weights summing to 1 pass through at most once."""
    d = np.load(GOLDEN)
    pano = torch.from_numpy(d["pano_u8"]).to(torch.float32) / 255
    cams, rp, yaws = (torch.from_numpy(d[f"{model}_{k}"]) for k in ("cams", "rp", "yaws"))
    golden = torch.from_numpy(d[f"{model}_{'resize' if resize else 'plain'}"])
    rf = torch.from_numpy(d["resize"]) if resize else None
    out = render(model, cams.to(dev), rp[:, 0], rp[:, 1], yaws, pano.to(dev), rf)
    torch.cuda.synchronize()
    assert out.shape == golden.shape
    rot = device_rotations(rp[:, 0], rp[:, 1], yaws, dev)
    H, W = golden.shape[-2:]
    worst, D_max = 0.0, 0.0
    cam = camera_models[model](cams)
    for i in range(cams.shape[0]):
        src, D = pano[None], 0.0
        if resize:
            scale = torch.pi / float(cam.vfov[i]) * float(H) / pano.shape[-2] * rf[i]
            shape, mode = (int(pano.shape[-2] * scale), int(pano.shape[-1] * scale)), "bicubic" if scale >= 1 else "area"
            src = _resized(pano[None], shape, mode)
            D = (_resized(pano[None].to(dev), shape, mode).cpu() - src).abs().max().item()
        ys = pg.Yardstick(model, cams[i:i + 1], rot[i:i + 1], H, W, src.to(dev, torch.float64))
        err = (out[i:i + 1].double() - golden[i:i + 1].to(dev).double()).abs()
        ratio = (err / (2 * ys.bound + D).clamp(min=1e-300)).max().item()
        worst, D_max = max(worst, ratio), max(D_max, D)
    print(f"{model} resize={resize}: device-vs-CPU resize difference {D_max:.2e}, worst ratio to the doubled gate {worst:.3f}")
    assert worst <= 1, worst


def test_hip_path_is_taken(dev, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("F.grid_sample called on the HIP path")

    monkeypatch.setattr(F, "grid_sample", refuse)
    monkeypatch.setattr(torch.nn.functional, "grid_sample", refuse)
    cams, _, pano, yaws, rolls, pitches = pg.case_inputs(pg.CASES[1])
    out = render("simple_radial", cams.to(dev), rolls, pitches, yaws, pano[0].to(dev), 0.5)
    torch.cuda.synchronize()
    assert out.shape == (8, 3, 47, 65)
    with pytest.raises(AssertionError, match="grid_sample"):            # the torch path does call it
        render("simple_radial", cams.to(dev), rolls, pitches, yaws, pano[0].to(dev, torch.float64))


@pytest.mark.parametrize("model", pg.MODELS)
def test_non_finite_camera_gives_zeros(dev, model):
    cams = ug.make_cameras(model, 2, 40, 50, seed=14)
    cams[1, 3] = float("nan")                          # a NaN focal: every coordinate of that image is NaN
    pano = pg.make_pano("noise", 3, 128, 256)[0].to(dev)
    out = render(model, cams.to(dev), torch.zeros(2), torch.zeros(2), torch.tensor([0.0, 1.0]), pano)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert (out[1] == 0).all() and (out[0] != 0).any()


def test_64_bit_offsets(dev):
    """n C H W = 150 * 1 * 4000 * 3600 > 2^31: the last image lies beyond every 32-bit offset (about 8.6 GB)."""
    n, H, W = 150, 4000, 3600
    if torch.cuda.get_device_properties(dev).total_memory < 24 * 2 ** 30:
        pytest.skip("needs 24 GB of device memory")
    cams = ug.make_cameras("simple_radial", 1, H, W, 0.2, seed=15)
    pano = pg.make_pano("noise", 1, 256, 512, seed=16)
    yaws = torch.linspace(-3, 3, n)
    rolls, pitches = torch.zeros(n), torch.full((n,), 0.2)
    out = render("simple_radial", cams.to(dev), rolls, pitches, yaws, pano[0].to(dev))
    torch.cuda.synchronize()
    ys_, xs_ = slice(H - 200, H), slice(W // 2 - 100, W // 2 + 100)    # a crop of the last image
    tail = out[-1:, :, ys_, xs_].clone()
    del out
    rot = device_rotations(rolls[-1:], pitches[-1:], yaws[-1:], dev)
    c = cams.clone()
    c[:, 4] -= xs_.start
    c[:, 5] -= ys_.start                               # the crop is the image of a camera with a shifted centre
    ys = pg.Yardstick("simple_radial", c, rot, 200, 200, pano.to(dev, torch.float64))
    ratio = ys.worst_ratio(tail)
    print(f"64-bit offsets: last image, worst ratio to the gate {ratio:.3f}")
    assert ratio <= 1, ratio


def test_one_panorama_per_image_equals_separate_calls(dev):
    cams, _, _, yaws, rolls, pitches = pg.case_inputs(pg.CASES[3])
    panos = pg.make_pano("noise", 1, 200, 400, seed=17, n=8).to(dev)
    for rf in (None, torch.linspace(0.3, 1.6, 8)):
        out = render("simple_divisional", cams.to(dev), rolls, pitches, yaws, panos, rf)
        for i in range(8):
            one = render("simple_divisional", cams[i:i + 1].to(dev), rolls[i:i + 1], pitches[i:i + 1], yaws[i:i + 1],
                         panos[i], None if rf is None else rf[i:i + 1])
            torch.cuda.synchronize()
            assert torch.equal(out[i:i + 1], one), (i, rf is None)


def test_one_camera_many_yaws_and_many_cameras_one_yaw(dev):
    """1 camera + n yaws renders n images; n cameras + 1 yaw renders ONE image, from camera 0 (the reference's quirk)."""
    cams, _, pano, yaws, rolls, pitches = pg.case_inputs(pg.CASES[0])
    pano = pano[0].to(dev)
    many = render("pinhole", cams[:1].to(dev), rolls[:1], pitches[:1], yaws, pano)
    one = render("pinhole", cams.to(dev), rolls, pitches, yaws[:1], pano)
    first = render("pinhole", cams[:1].to(dev), rolls[:1], pitches[:1], yaws[:1], pano)
    torch.cuda.synchronize()
    assert many.shape[0] == 8 and one.shape[0] == 1
    assert torch.equal(one, first) and torch.equal(many[:1], first)
