"""GPU: get_perspective_field / get_up_field / get_latitude_field on the HIP path (gclm_perspective_fields) against the
float64 yardstick, per pixel.

Gate (tests/perspective_gate.py, checked on CPU by test_perspective_abi.py): kappa delta_q / |q| + 2 ulp(1) on the up
direction, kappa delta_q on the unnormalised up vector, the asin of kappa delta_s around sin(latitude) plus 2 ulp on the
latitude; kappa derived per case from a float32 restatement against float64."""
import math

import numpy as np
import pytest
import torch

from geocalib_amd import Gravity, camera_models, perspective_fields as pf
import perspective_gate as pg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def render(model, cams, gravs, dev, normalize=True):
    """HIP fields of float32 cameras / gravities: (up or q (B, H, W, 2), lat (B, H, W), the gravity as stored)."""
    cam, grav = camera_models[model](cams.to(dev)), Gravity(gravs.to(dev))
    if normalize:
        up, lat = pf.get_perspective_field(cam, grav)
        up, lat = up.permute(0, 2, 3, 1), lat[:, 0]
    else:
        up, lat = pf.get_up_field(cam, grav, normalize=False), pf.get_latitude_field(cam, grav)[..., 0]
    torch.cuda.synchronize()
    return up, lat, grav._data.detach().cpu()


def ratios(model, cams, gravs, up, lat, normalize, dev):
    H, W = lat.shape[-2:]
    ref = pg.fields(model, cams, gravs, H, W, device=dev)
    b_up, b_q, b_lat = pg.gates(ref, *pg.kappas(model, cams, gravs, H, W, dev, ref))
    r_up = pg.worst_ratio(up, ref["up"], b_up) if normalize else pg.worst_ratio(up, ref["q"], b_q)
    return r_up, pg.worst_ratio(lat, ref["lat"], b_lat)


@pytest.mark.parametrize("case", pg.CASES, ids=[f"{c[0]}-{c[1]}-B{c[3]}-{c[4]}x{c[5]}-{c[6]}-n{int(c[7])}" for c in pg.CASES])
def test_parity_against_float64(dev, case):
    model, k1, k2, B, H, W, kind, normalize = case
    cams, gravs = pg.case_inputs(case)
    up, lat, g = render(model, cams, gravs, dev, normalize)
    assert up.shape == (B, H, W, 2) and lat.shape == (B, H, W) and up.dtype == lat.dtype == torch.float32
    r_up, r_lat = ratios(model, cams, g, up, lat, normalize, dev)
    print(f"{case}: worst ratio to the gate up {r_up:.3f} latitude {r_lat:.3f}")
    assert r_up <= 1 and r_lat <= 1, (r_up, r_lat)


@pytest.mark.parametrize("model", pg.MODELS)
def test_golden_cameras_against_the_reference_float64_outputs(dev, model):
    """tests/golden/golden_host_api.npz: the reference's own float64 fields on its cameras (12 x 16 samples of 48 x 64).  The
    reference renormalised the gravity in float64, the device uses it as Gravity() stores it in float32: the gate is
    widened by what that difference moves the float64 fields."""
    from test_host_api import host_api_golden
    gold = host_api_golden()
    cams, gravs = gold[f"api/{model}/camera"], gold[f"api/{model}/gravity"]
    W, H = (int(v) for v in cams[0, :2].tolist())
    up, lat, g = render(model, cams, gravs, dev)
    ref = pg.fields(model, cams, g, H, W)
    ref64 = pg.fields(model, cams, torch.nn.functional.normalize(gravs.double(), dim=-1), H, W, clamp_hi=pg.LAT_HI64)
    b_up, _, b_lat = pg.gates(ref, *pg.kappas(model, cams, g, H, W, ref=ref))
    b_up, b_lat = b_up + (ref["up"] - ref64["up"]).abs(), b_lat + (ref["lat"] - ref64["lat"]).abs()
    rows, cols = torch.linspace(0, H - 1, 12).round().long(), torch.linspace(0, W - 1, 16).round().long()
    pick = lambda t: t[:, rows][:, :, cols]  # noqa: E731
    gold_up = gold[f"api/{model}/out64/up_field"].permute(0, 2, 3, 1)
    gold_lat = gold[f"api/{model}/out64/latitude_field"][:, 0]
    r_up = pg.worst_ratio(pick(up.cpu()), gold_up, pick(b_up))
    r_lat = pg.worst_ratio(pick(lat.cpu()), gold_lat, pick(b_lat))
    print(f"{model}: golden worst ratios up {r_up:.3f} latitude {r_lat:.3f}")
    assert r_up <= 1 and r_lat <= 1, (r_up, r_lat)


def test_hip_path_is_taken(dev, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("torch path called")

    monkeypatch.setattr(pf, "_up_field_torch", refuse)
    monkeypatch.setattr(pf, "_latitude_field_torch", refuse)
    cams, gravs = pg.make_cameras("radial", 2, 40, 56, seed=5), pg.make_gravity(2, seed=5)
    cam, grav = camera_models["radial"](cams.to(dev)), Gravity(gravs.to(dev))
    up, lat = pf.get_perspective_field(cam, grav)
    assert up.shape == (2, 2, 40, 56) and lat.shape == (2, 1, 40, 56)
    assert pf.get_up_field(cam, grav).shape == (2, 40, 56, 2) and pf.get_latitude_field(cam, grav).shape == (2, 40, 56, 1)
    assert pf.get_perspective_field(cam, grav, use_up=False)[0].abs().max() == 0
    leaf = cams.to(dev).requires_grad_(True)
    with pytest.raises(AssertionError, match="torch path"):          # a camera that requires grad takes the torch path
        pf.get_perspective_field(camera_models["radial"](leaf), grav)
    monkeypatch.undo()
    up, lat = pf.get_perspective_field(camera_models["radial"](leaf), grav)
    (up.sum() + lat.sum()).backward()
    assert leaf.grad is not None and torch.isfinite(leaf.grad).all() and leaf.grad[:, 2:7].abs().sum() > 0


NAN_SLOTS = [("fx", 2), ("fy", 3), ("cx", 4), ("cy", 5), ("k1", 6), ("k2", 7)]


@pytest.mark.parametrize("model", pg.MODELS)
@pytest.mark.parametrize("normalize", [True, False])
def test_non_finite_inputs_give_nan_where_the_torch_path_does(dev, model, normalize):
    H, W = 37, 53
    cams, gravs = pg.make_cameras(model, 2, H, W, seed=7), pg.make_gravity(2, seed=7)
    cases = [(f"nan {n}", i, float("nan"), None) for n, i in NAN_SLOTS] + [("inf k1", 6, math.inf, None)]
    cases += [(f"nan gravity {j}", None, None, j) for j in range(3)]
    for what, slot, val, gj in cases:
        c = cams.clone()
        if slot is not None:
            c[1, slot] = val
        cam, grav = camera_models[model](c.to(dev)), Gravity(gravs.to(dev))
        if gj is not None:
            grav._data[1, gj] = float("nan")
        up = pf.get_up_field(cam, grav, normalize=normalize)
        lat = pf.get_latitude_field(cam, grav)
        up_t = pf._up_field_torch(cam, grav, H, W, normalize)
        lat_t = pf._latitude_field_torch(cam, grav, H, W)
        torch.cuda.synchronize()
        assert torch.equal(up.isnan(), up_t.isnan()), (what, up.isnan().sum().item(), up_t.isnan().sum().item())
        assert torch.equal(lat.isnan(), lat_t.isnan()), (what, lat.isnan().sum().item(), lat_t.isnan().sum().item())
        assert not up[0].isnan().any() and not lat[0].isnan().any(), what          # the other image is untouched


@pytest.mark.parametrize("model", ["pinhole", "simple_divisional"])
def test_shapes_and_strides_equal_the_torch_path(dev, model):
    cams, gravs = pg.make_cameras(model, 3, 30, 41, seed=8), pg.make_gravity(3, seed=8)
    hip = (camera_models[model](cams.to(dev)), Gravity(gravs.to(dev)))
    ref = (camera_models[model](cams.to(dev).double()), Gravity(gravs.to(dev).double()))
    for kw in ({}, {"use_up": False}, {"use_latitude": False}):
        for a, b in zip(pf.get_perspective_field(*hip, **kw), pf.get_perspective_field(*ref, **kw)):
            assert a.shape == b.shape and a.stride() == b.stride() and a.dtype == torch.float32, (kw, a.stride(), b.stride())
    for f in (pf.get_up_field, pf.get_latitude_field):
        a, b = f(*hip), f(*ref)
        assert a.shape == b.shape and a.stride() == b.stride() and a.is_contiguous()


def test_64_bit_offsets(dev):
    """B * H * W = 520 * 2048 * 2048 > 2^31: the last image's up and latitude lie beyond every 32-bit offset (26 GB)."""
    B, H, W = 520, 2048, 2048
    if torch.cuda.get_device_properties(dev).total_memory < 40 * 2 ** 30:
        pytest.skip("needs 40 GB of device memory")
    cams, gravs = pg.make_cameras("simple_radial", B, H, W, seed=9), pg.make_gravity(B, seed=9)
    cam, grav = camera_models["simple_radial"](cams.to(dev)), Gravity(gravs.to(dev))
    up, lat = pf.get_perspective_field(cam, grav)
    torch.cuda.synchronize()
    up, lat = up[-1:].permute(0, 2, 3, 1).clone(), lat[-1:, 0].clone()
    torch.cuda.empty_cache()
    r_up, r_lat = ratios("simple_radial", cams[-1:], grav._data[-1:].cpu(), up, lat, True, dev)
    print(f"64-bit offsets: last image, worst ratios up {r_up:.3f} latitude {r_lat:.3f}")
    assert r_up <= 1 and r_lat <= 1, (r_up, r_lat)


DIST = {"pinhole": None, "simple_radial": (-0.2, 0.1), "radial": (-0.2, 0.1), "simple_divisional": (-0.3, 0.3)}


@pytest.mark.parametrize("model", ["pinhole", "simple_radial", "radial"])
def test_round_trip_through_the_solver(dev, model):
    """The reference's gradient-checker end-to-end test at scale (siclib/geometry/gradient_checker.py:584-641, atol 1e-3):
    noise-free fields of 64 random cameras, rendered on the device, are solved back by LMOptimizer.  Not simple_divisional:
    the LM sweep evaluates the reference's float32 s' on purpose, which cancels near the principal point, so the exact
    fields rendered here are not its fixed point to 1e-3 (one camera of 64 lands 3 % off in focal)."""
    from geocalib_amd import LMOptimizer
    B, S = 64, 256
    g = torch.Generator().manual_seed(19)
    roll = (torch.rand(B, generator=g) - 0.5) * np.pi / 2
    pitch = (torch.rand(B, generator=g) - 0.5) * np.pi / 2
    vfov = np.deg2rad(20) + torch.rand(B, generator=g) * np.deg2rad(60)
    d = {"height": torch.full((B,), float(S)), "width": torch.full((B,), float(S)), "vfov": vfov}
    if DIST[model]:
        lo, hi = DIST[model]
        d["k1"] = lo + (hi - lo) * torch.rand(B, generator=g)
    cam = camera_models[model].from_dict(d).to(dev)
    grav = Gravity.from_rp(roll, pitch).to(dev)
    up, lat = pf.get_perspective_field(cam, grav)
    out = LMOptimizer({"camera_model": model}).eval()({"up_field": up.contiguous(), "latitude_field": lat.contiguous()})
    torch.cuda.synchronize()
    c, gv = out["camera"]._data.cpu(), out["gravity"]._data.cpu()
    f = cam.f[:, 1].cpu()
    assert torch.allclose(c[:, 3], f, rtol=1e-3, atol=1e-3), (c[:, 3] / f - 1).abs().max()
    assert torch.allclose(gv, grav.vec3d.cpu(), atol=1e-3), (gv - grav.vec3d.cpu()).abs().max()
    if DIST[model]:
        assert torch.allclose(c[:, 6], cam._data[:, 6].cpu(), atol=1e-3), (c[:, 6] - cam._data[:, 6].cpu()).abs().max()
