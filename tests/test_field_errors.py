"""GPU: metrics.perspective_field_metrics on the HIP path (gclm_field_errors) against the float64 yardstick.

Gates (tests/field_error_gate.py, checked on CPU by test_field_errors_abi.py): per pixel, the angle perspective_gate's bound
on the target subtends plus the float32 rounding of the angle evaluation (up), perspective_gate's latitude bound plus 2 ulp
of the prediction (latitude), each scaled by a kappa derived per case; the means by the mean of those plus a summation
term; every recall must be a count inside [#(e64 < t - gate), #(e64 < t + gate)]."""
import math

import numpy as np
import pytest
import torch

from geocalib_amd import Gravity, LMOptimizer, camera_models, metrics, perspective_fields as pf
import field_error_gate as fg
import perspective_gate as pg

pytestmark = pytest.mark.gpu

KEYS = [f"{f}_angle_{k}" for f in ("up", "latitude") for k in ["error", "error_weighted"] + [f"recall@{t}" for t in fg.THRESHOLDS]]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def calibration(model, cams, gravs, dev):
    cam, grav = camera_models[model](cams.to(dev)), Gravity(gravs.to(dev))
    grav._data = gravs.to(dev)                    # as stored: the cases' gravities are scored as they are
    return cam, grav


def on_device(t, dev, offset4=False):
    """`t` on the device; with `offset4` in a buffer that starts 4 bytes past an aligned address."""
    if not offset4:
        return t.to(dev)
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    flat[1:].copy_(t.reshape(-1))
    return flat[1:].view(t.shape)


def score(case, cams, gravs, data, dev, maps=False):
    """The device's answer in the form field_error_gate.verdict takes; absent keys become NaN columns."""
    cam, grav = calibration(case[0], cams, gravs, dev)
    out = metrics.perspective_field_metrics({k: on_device(v, dev, case[5]) for k, v in data.items()}, cam, grav, fg.THRESHOLDS, maps)
    torch.cuda.synchronize()
    nan = torch.full((case[1],), math.nan, device=dev)
    stats = torch.stack([out.get(k, nan) for k in KEYS], -1)
    assert set(out) - {"up_error", "latitude_error"} <= set(KEYS) and all(out[k].dtype == torch.float32 for k in out)
    return {"stats": stats, "up_err": out.get("up_error"), "lat_err": out.get("latitude_error")}, out


def check(case, dev):
    cams, gravs, data = fg.make_case(case)
    for which, maps in (("all", True), ("noconf", False), ("up", True), ("lat", False)):
        d = fg.subset(data, which)
        res, out = score(case, cams, gravs, d, dev, maps)
        assert ("up_error" in out) == (maps and "up_field" in d) and ("latitude_error" in out) == (maps and "latitude_field" in d)
        assert ("up_angle_error_weighted" in out) == ("up_confidence" in d)
        assert ("latitude_angle_error_weighted" in out) == ("latitude_confidence" in d)
        v = fg.verdict(fg.yardstick(case, cams, gravs, d), res)
        print(f"{fg.case_id(case)} {which}{' +maps' if maps else ''}: {v}")
        assert fg.passes(v), (which, v)


@pytest.mark.parametrize("case", fg.CASES, ids=fg.case_id)
def test_parity_against_float64(dev, case):
    check(case, dev)


@pytest.mark.parametrize("case", fg.EXTREMES, ids=fg.case_id)
def test_gravity_extremes(dev, case):
    check(case, dev)


def _all(out):
    return torch.stack([out[k] for k in KEYS], -1)


@pytest.mark.parametrize("case", [fg.CASES[0], fg.CASES[8], fg.CASES[5]], ids=fg.case_id)
def test_results_are_bit_identical_and_independent_of_the_batch(dev, case):
    cams, gravs, data = fg.make_case(case)
    cam, grav = calibration(case[0], cams, gravs, dev)
    d = {k: on_device(v, dev, case[5]) for k, v in data.items()}
    a = metrics.perspective_field_metrics(d, cam, grav, return_errors=True)
    b = metrics.perspective_field_metrics(d, cam, grav, return_errors=True)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for i in range(case[1]):                     # image i alone, its planes where they lie in the batch
        one = calibration(case[0], cams[i:i + 1], gravs[i:i + 1], dev)        # (slicing a Gravity renormalises it)
        alone = metrics.perspective_field_metrics({k: v[i:i + 1] for k, v in d.items()}, *one)
        assert torch.equal(_all(alone)[0], _all(a)[i]), i


def test_a_nan_pixel_poisons_its_image_and_field_only(dev):
    case = fg.CASES[2]                           # pinhole, 2 x 30 x 200
    cams, gravs, data = fg.make_case(case)
    cam, grav = calibration(case[0], cams, gravs, dev)
    d = {k: v.to(dev) for k, v in data.items()}
    clean = metrics.perspective_field_metrics(d, cam, grav, return_errors=True)
    for field, col, pre in (("up_field", 0, "up"), ("up_field", 1, "up"), ("latitude_field", 0, "latitude")):
        bad = {k: v.clone() for k, v in d.items()}
        bad[field][1, col, 10, 7] = math.nan
        out = metrics.perspective_field_metrics(bad, cam, grav, return_errors=True)
        other = "latitude" if pre == "up" else "up"
        assert out[f"{pre}_angle_error"][1].isnan() and out[f"{pre}_angle_error_weighted"][1].isnan()
        assert out[f"{pre}_error"][1, 10, 7].isnan() and out[f"{pre}_error"].isnan().sum() == 1
        hw = case[2] * case[3]
        for t in fg.THRESHOLDS:                  # the pixel counts at no threshold: it was a hit where its error was below t
            was_hit = bool(clean[f"{pre}_error"][1, 10, 7] < t)
            want = (clean[f"{pre}_error"][1] < t).sum().item() - was_hit
            assert round(out[f"{pre}_angle_recall@{t}"][1].item() * hw) == want, t
        for k in KEYS:                           # image 0, and the other field of image 1, bit for bit
            assert torch.equal(out[k][0], clean[k][0]), k
            if k.startswith(other):
                assert torch.equal(out[k][1], clean[k][1]), k


def test_dispatch(dev, monkeypatch):
    case = fg.CASES[0]
    cams, gravs, data = fg.make_case(case)
    cam, grav = calibration(case[0], cams, gravs, dev)
    d = {k: v.to(dev) for k, v in data.items()}

    def refuse(*a, **k):
        raise AssertionError("torch path called")

    monkeypatch.setattr(metrics, "_field_metrics_torch", refuse)
    out = metrics.perspective_field_metrics(d, cam, grav)
    assert sorted(out) == sorted(KEYS)
    leaf = d["up_field"].clone().requires_grad_(True)
    with pytest.raises(AssertionError, match="torch path"):          # a field that requires grad takes the torch path
        metrics.perspective_field_metrics({**d, "up_field": leaf}, cam, grav)
    with pytest.raises(AssertionError, match="torch path"):
        metrics.perspective_field_metrics({k: v.double() for k, v in d.items()}, cam, grav)
    monkeypatch.undo()
    lat = d["latitude_field"].clone().requires_grad_(True)
    got = metrics.perspective_field_metrics({**d, "up_field": leaf, "latitude_field": lat}, cam, grav)
    (got["up_angle_error_weighted"].sum() + got["latitude_angle_error"].sum()).backward()
    assert torch.isfinite(lat.grad).all() and lat.grad.abs().sum() > 0 and leaf.grad is not None and leaf.grad.shape == leaf.shape
    # ... and the two paths agree to what the float32 torch path resolves
    assert torch.allclose(got["up_angle_error"].detach(), out["up_angle_error"], atol=0.05)
    assert torch.allclose(got["latitude_angle_error"].detach(), out["latitude_angle_error"], rtol=1e-4, atol=1e-4)


DIST = {"pinhole": None, "simple_radial": (-0.2, 0.1), "radial": (-0.2, 0.1)}


@pytest.mark.parametrize("model", ["pinhole", "simple_radial", "radial"])
def test_a_solve_explains_the_fields_it_was_given(dev, model):
    """Noise-free fields of 16 random cameras, rendered on the device, are solved by LMOptimizer and scored against the
    returned camera and gravity: every pixel of both fields within 1 degree.  Not simple_divisional, for the reason
    test_perspective_fields.py::test_round_trip_through_the_solver gives."""
    B, S = 16, 128
    g = torch.Generator().manual_seed(23)
    roll, pitch = ((torch.rand(B, generator=g) - 0.5) * np.pi / 2 for _ in range(2))
    d = {"height": torch.full((B,), float(S)), "width": torch.full((B,), float(S)),
         "vfov": np.deg2rad(20) + torch.rand(B, generator=g) * np.deg2rad(60)}
    if DIST[model]:
        lo, hi = DIST[model]
        d["k1"] = lo + (hi - lo) * torch.rand(B, generator=g)
    cam, grav = camera_models[model].from_dict(d).to(dev), Gravity.from_rp(roll, pitch).to(dev)
    up, lat = pf.get_perspective_field(cam, grav)
    data = {"up_field": up.contiguous(), "latitude_field": lat.contiguous()}
    out = LMOptimizer({"camera_model": model}).eval()(data)
    m = metrics.perspective_field_metrics(data, out["camera"], out["gravity"])
    torch.cuda.synchronize()
    print({k: (v.min().item(), v.max().item()) for k, v in m.items()})
    assert (m["up_angle_recall@1"] == 1).all() and (m["latitude_angle_recall@1"] == 1).all()
    assert "up_angle_error_weighted" not in m and m["up_angle_error"].max() < 0.1 and m["latitude_angle_error"].max() < 0.1


def test_64_bit_offsets(dev):
    """B * H * W = 520 * 2048 * 2048 > 2^31: the last image's latitude plane (8.7 GB in all) lies beyond every 32-bit offset.
    Its statistics equal those of the image scored alone, bit for bit."""
    B, H, W = 520, 2048, 2048
    if torch.cuda.get_device_properties(dev).total_memory < 24 * 2 ** 30:
        pytest.skip("needs 24 GB of device memory")
    cams, gravs = pg.make_cameras("simple_radial", B, H, W, seed=9), pg.make_gravity(B, seed=9)
    cam, grav = calibration("simple_radial", cams, gravs, dev)
    moved = fg._perturbed(cams, gravs, 1.0)
    lat = pf.get_latitude_field(*calibration("simple_radial", *moved, dev)).view(B, 1, H, W)
    batch = metrics.perspective_field_metrics({"latitude_field": lat}, cam, grav)
    alone = metrics.perspective_field_metrics({"latitude_field": lat[-1:]}, *calibration("simple_radial", cams[-1:], gravs[-1:], dev))
    first = metrics.perspective_field_metrics({"latitude_field": lat[:1]}, *calibration("simple_radial", cams[:1], gravs[:1], dev))
    torch.cuda.synchronize()
    assert sorted(batch) == sorted(k for k in KEYS if k.startswith("latitude") and "weighted" not in k)
    for k in batch:
        assert batch[k].shape == (B,) and torch.equal(batch[k][-1], alone[k][0]) and torch.equal(batch[k][0], first[k][0]), k
    assert 0.5 < batch["latitude_angle_error"][-1] < 15 and torch.isfinite(batch["latitude_angle_error"]).all()
