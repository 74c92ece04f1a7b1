"""GPU: Camera.reproject_image / upright_image on the HIP path (gclm_reproject_image) against the float64 yardstick, per pixel.

Gate (tests/reproject_gate.py, its conditions checked on CPU by test_reproject_abi.py): |out - ref| <= L * delta + 4 ulp(A)
outside the pixels at a discontinuity of the definition, delta the coordinate bound derived per case from a float32
restatement against float64; exactly 0 where the yardstick is invisible, folded or far out of view; the mask compared
outside the excluded pixels and the delta band at the in-image edge."""
import functools
import math

import pytest
import torch

from geocalib_amd import Gravity, camera as camera_module, camera_models
import reproject_gate as rg
import undistort_gate as ug
from test_reproject_abi import LAT_GATE_DEG, LAT_RUNS, latitude_known_answer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def parts(case):
    """The yardstick of one case, computed once on the CPU and left unchanged."""
    return rg.case_parts(case)


def run(case, dev, **kw):
    p = parts(case)
    src, tgt = camera_models[case[0]](p["src"].to(dev)), camera_models[case[4]](p["tgt"].to(dev))
    out = src.reproject_image(p["img"].to(dev), tgt, None if p["rot"] is None else p["rot"].to(dev), **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", rg.CASES, ids=[rg.case_id(c) for c in rg.CASES])
def test_parity_against_float64(dev, case):
    p = parts(case)
    out, valid = run(case, dev, return_valid=True)
    assert out.shape == p["ref"].shape and out.dtype == torch.float32 and out.is_cuda
    assert valid.shape == p["valid"].shape and valid.dtype == torch.bool and valid.is_cuda
    ratio = rg.worst_ratio(out.cpu(), p["ref"], p["bound"])
    wrong = ((valid.cpu() != p["valid"]) & ~p["mask_free"]).sum().item()
    print(f"{rg.case_id(case)}: delta {p['delta']:.2e} px, worst ratio to the gate {ratio:.3f}, mask pixels off {wrong}")
    assert ratio <= 1, ratio
    assert wrong == 0, wrong
    assert torch.equal(run(case, dev), out)                                  # without the mask: the same image
    if case[7] == "yaw100":
        assert (out == 0).all() and not valid.any()


def test_hip_path_is_taken(dev, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("torch composition called")

    monkeypatch.setattr(camera_module, "_reproject_torch", refuse)
    cams = ug.make_cameras("radial", 1, 64, 96, seed=13).to(dev)
    cam, img = camera_models["radial"](cams), torch.rand(2, 3, 64, 96, device=dev)
    grav = Gravity.from_rp(torch.tensor([0.3], device=dev), torch.tensor([-0.2], device=dev))
    out, valid = cam.reproject_image(img, return_valid=True)
    up = cam.upright_image(img, grav, level_pitch=True)
    torch.cuda.synchronize()
    assert out.shape == up.shape == (2, 3, 64, 96) and valid.shape == (2, 64, 96) and valid.any() and up.abs().sum() > 0
    with pytest.raises(AssertionError, match="torch composition"):          # float64 does take the composition
        cam.reproject_image(img.double())


@pytest.mark.parametrize("model,k1,k2,Hin,Win", [("simple_radial", 0.3, None, 37, 53), ("radial", -0.2, 0.1, 37, 53),
                                                ("simple_divisional", -1.0, None, 50, 41), ("pinhole", None, None, 37, 53)])
def test_default_call_against_undistort_image(dev, model, k1, k2, Hin, Win):
    """reproject_image(img) is undistort_image(img) within the sum of the two gates, where the source model is not folded."""
    H, W, n = 37, 53, 3
    cams = ug.make_cameras(model, n, H, W, k1, k2, seed=21)
    img = ug.make_images("noise", n, 3, Hin, Win, seed=21)
    cam = camera_models[model](cams.to(dev))
    a, b = cam.reproject_image(img.to(dev)), cam.undistort_image(img.to(dev))
    torch.cuda.synchronize()
    pin = torch.cat([cams[:, :6], torch.zeros(n, 2)], -1)
    geo = (model, cams, "pinhole", pin, None, H, W, H, W, Hin, Win)
    c64, c32 = rg.coordinates(*geo), rg.coordinates(*geo, dtype=torch.float32)
    ex = rg.excluded(c64, model)
    src64 = img.double()
    _, bound_r = rg.reference(src64, c64, ex, rg.coordinate_bound(c64, c32, ex, Hin, Win))
    bound_u = ug.gate(src64, *ug.coordinates(model, cams, H, W, Hin, Win), ug.coordinate_bound(model, cams, H, W, Hin, Win))
    keep = (c64["ok"] & ~ex)[:, None].expand_as(a)
    assert keep.double().mean() > 0.5
    ratio = ug.worst_ratio(a.cpu()[keep], b.cpu().double()[keep], (bound_r + bound_u)[keep])
    print(f"{model}: reproject_image against undistort_image, worst ratio to the summed gates {ratio:.3f}")
    assert ratio <= 1, ratio
    assert (a.cpu()[~keep & ~ex[:, None].expand_as(a)] == 0).all()


def test_upright_image_levels_the_latitude_field_on_the_device(dev):
    worst = max(latitude_known_answer(*r, device=dev, dtype=torch.float32) for r in LAT_RUNS)
    print(f"device float32: worst latitude error {worst:.4f} deg (gate {LAT_GATE_DEG})")
    assert worst <= LAT_GATE_DEG, worst
    assert min(latitude_known_answer(*r, device=dev, dtype=torch.float32, transpose=True) for r in LAT_RUNS) > 10 * LAT_GATE_DEG


POISON_CASE = ("simple_radial", None, None, None, "radial", -0.1, 0.05, "roll25", 3, 3, 37, 53, "noise")
POISON = [(what, slot, v) for what, slots in (("src", (2, 4, 6)), ("tgt", (3, 5, 6)), ("rot", (0, 5, 8)))
          for slot in slots for v in (math.nan, math.inf, -math.inf)]


@pytest.mark.parametrize("what,slot,value", POISON, ids=[f"{w}[{s}]={v}" for w, s, v in POISON])
def test_non_finite_entry_zeroes_its_image_alone(dev, what, slot, value):
    src, tgt, rot, img = (t.to(dev) for t in rg.case_inputs(POISON_CASE, seed=3))
    cam = lambda s, t: (camera_models["simple_radial"](s), camera_models["radial"](t))  # noqa: E731
    s, t = cam(src, tgt)
    clean, clean_valid = s.reproject_image(img, t, rot, return_valid=True)
    bad = {"src": src.clone(), "tgt": tgt.clone(), "rot": rot.clone()}
    bad[what].view(3, -1)[1, slot] = value
    s, t = cam(bad["src"], bad["tgt"])
    out, valid = s.reproject_image(img, t, bad["rot"], return_valid=True)
    torch.cuda.synchronize()
    assert clean_valid[1].any() and (clean[1] != 0).any()
    assert (out[1] == 0).all() and not valid[1].any()
    for i in (0, 2):
        assert torch.equal(out[i].view(torch.int32), clean[i].view(torch.int32)) and torch.equal(valid[i], clean_valid[i])


def test_layout_stream_and_camera_batch_do_not_change_the_bits(dev):
    case = ("radial", None, None, None, "simple_radial", 0.2, None, "level", 1, 1, 37, 53, "noise")
    src, tgt, rot, img = (t.to(dev) for t in rg.case_inputs(case, seed=5))
    s, t = camera_models["radial"](src), camera_models["simple_radial"](tgt)
    plain, plain_valid = s.reproject_image(img, t, rot, return_valid=True)
    torch.cuda.synchronize()
    assert plain_valid.any() and not plain_valid.all()
    same = lambda o: torch.equal(o[0].view(torch.int32), plain.view(torch.int32)) and torch.equal(o[1], plain_valid)  # noqa: E731
    # a non-contiguous image (the memory of its transpose)
    strided = img.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not strided.is_contiguous() and torch.equal(strided, img)
    assert same(s.reproject_image(strided, t, rot, return_valid=True))
    # a non-default stream
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        o = s.reproject_image(img, t, rot, return_valid=True)
    stream.synchronize()
    assert same(o)
    # one camera pair and one rotation for the batch, or each repeated B times; a (3, 3) rotation
    s3, t3 = camera_models["radial"](src.expand(3, -1).contiguous()), camera_models["simple_radial"](tgt.expand(3, -1).contiguous())
    assert same(s3.reproject_image(img, t3, rot.expand(3, -1, -1).contiguous(), return_valid=True))
    assert same(s3.reproject_image(img, t, rot, return_valid=True))           # source B, target 1
    assert same(s.reproject_image(img, t3, rot[0], return_valid=True))        # source 1, target B
    torch.cuda.synchronize()


def test_64_bit_offsets(dev):
    """B * C * H * W = 33 * 8192 * 8192 > 2^31 from a small source: the last image and its mask lie beyond every 32-bit
    offset (about 9 GB of output)."""
    B, H, W = 33, 8192, 8192
    if torch.cuda.get_device_properties(dev).total_memory < 24 * 2 ** 30:
        pytest.skip("needs 24 GB of device memory")
    src = ug.make_cameras("simple_radial", 1, rg.HS, rg.WS, 0.2, seed=15)
    tgt = ug.make_cameras("pinhole", 1, H, W, seed=16)
    tgt[:, 2:4] = 0.9 * W
    one = ug.make_images("noise", 1, 1, rg.HIN, rg.WIN, seed=17).to(dev)
    s, t = camera_models["simple_radial"](src.to(dev)), camera_models["pinhole"](tgt.to(dev))
    rot = rg.make_rotations("roll25", 1).to(dev)
    first, first_valid = s.reproject_image(one, t, rot, return_valid=True)
    out, valid = s.reproject_image(one.expand(B, -1, -1, -1).contiguous(), t, rot, return_valid=True)
    torch.cuda.synchronize()
    assert out.numel() > 2 ** 31 and valid.numel() > 2 ** 31 and first_valid.any() and not first_valid.all()
    assert torch.equal(out[-1].view(torch.int32), first[0].view(torch.int32)) and torch.equal(valid[-1], first_valid[0])
    assert torch.equal(out[B // 2].view(torch.int32), first[0].view(torch.int32))
