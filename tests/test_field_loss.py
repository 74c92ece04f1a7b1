"""GPU: losses.perspective_field_loss on the HIP path (gclm_field_loss, gclm_field_loss_grad) against the float64 yardstick.

Gates (tests/field_loss_gate.py, checked on CPU by test_field_loss_abi.py): perspective_gate's bound on the target propagated
to first order through each loss and each derivative, plus the float32 rounding of the evaluation and of the sums, each scaled
by a kappa derived per case; an l1 sign is held exactly except where the float64 residual lies within the target's bound."""
import math

import pytest
import torch
from torch.nn import functional as F

from geocalib_amd import Gravity, camera_models, fields, losses, perspective_fields as pf
import field_error_gate as fg
import field_loss_gate as lg
import perspective_gate as pg
from test_field_errors import calibration, on_device

pytestmark = pytest.mark.gpu
U = lg.U


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def run(case, which, types, dev, data=None, gout=None, den=False):
    """The device's answer in the form field_loss_gate.verdict takes: weighted losses (B, 2) (NaN for an absent field), the
    gradient planes of sum_b grad_output[b, k] total_k[b] through autograd, and with `den` the denominators of the C call."""
    T = lg.target(case)
    B = case[1]
    cam, grav = calibration(case[0], T["cams"], T["gravs"], dev)
    d = {k: on_device(v, dev, case[5]) for k, v in fg.subset(T["data"] if data is None else data, which).items()}
    leaves = {k: v.requires_grad_(True) for k, v in d.items() if k.endswith("_field")}
    out = losses.perspective_field_loss(d, cam, grav, types[0], types[1], True, *lg.WEIGHTS)
    gout = (lg.grad_output(B) if gout is None else gout).to(dev)
    nan = torch.full((B,), math.nan, device=dev)
    total = sum((gout[:, i] * out[f"{n}_total"]).sum() for i, n in enumerate(("up", "latitude")) if f"{n}_field" in d)
    total.backward()
    torch.cuda.synchronize()
    assert all(v.dtype == torch.float32 and v.shape == (B,) for v in out.values())
    res = {"loss": torch.stack([out.get("up_total", nan), out.get("latitude_total", nan)], -1).detach(),
           "g_up": None if "up_field" not in d else leaves["up_field"].grad,
           "g_lat": None if "latitude_field" not in d else leaves["latitude_field"].grad}
    if den:
        res["den"] = fields.field_loss(case[0], cam._data, grav._data, d.get("up_field"), d.get("latitude_field"), d.get("up_confidence"),
                                       d.get("latitude_confidence"), *types)[:, 2:]
    return res, out


@pytest.mark.parametrize("case", lg.CASES, ids=lg.case_id)
def test_parity_against_float64(dev, case):
    """Losses and all three gradient planes of every loss type and subset of the case, with the non-uniform grad_output of
    the gate: an image whose grad_output is 0 gets exact zeros."""
    gout = lg.grad_output(case[1])
    for types in lg.loss_types(case):
        for which in lg.SUBSETS:
            res, out = run(case, which, types, dev, den=True)
            assert ("up_total" in out) == (which != "lat") and ("latitude_total" in out) == (which != "up")
            assert ("perspective_total" in out) and (f"up-{types[0]}-loss" in out) == (which != "lat")
            v = lg.verdict(lg.yardstick(case, which, types), res)
            print(f"{lg.case_id(case)} {types} {which}: {v}")
            assert lg.passes(v), (types, which, v)
            for i, k in enumerate(("g_up", "g_lat")):
                if res[k] is not None:
                    zero = gout[:, i] == 0
                    assert (res[k][zero.to(dev)] == 0).all() and (res[k][~zero.to(dev)] != 0).any(), (types, which, k)


E2E = [("pinhole", 3, 37, 53, "random", False), ("simple_divisional", 3, 37, 53, "random", False),
       ("simple_divisional", 2, 11, 70, "random", False)]


@pytest.mark.parametrize("case", E2E, ids=lg.case_id)
def test_autograd_end_to_end(dev, case):
    """Raw head outputs go through F.normalize (up) and asin(tanh(.)) (latitude) into perspective_total.sum().backward() on
    the device.  The leaf gradients are held to the chain rule in float64 on the CPU -- the torch path's gradient at the
    device's float32 fields, pulled back through the two maps in float64 -- within the gate propagated through the maps:
        up:   |J|^T gate_G + 8 U (|G_x| + |G_y|) / |raw|       (J = (I - p p^T) / |raw|, evaluated in float32)
        lat:  |J| gate_G + 8 U |J G| (1 + 2 / (1 - tanh^2))    (J = sech(raw) as sech^2 / sqrt(1 - tanh^2): the float32
                                                                difference 1 - tanh^2 carries U / (1 - tanh^2))
    The loss types are smooth ones: an l1 sign at a residual within float32 rounding of 0 is undecided (the gate's own rule),
    which no bound through the maps can express.  The confidences are leaves too: their .grad stays None."""
    model, B, H, W, _, _ = case
    T = lg.target(case)
    types = ("cauchy", "huber")
    g = torch.Generator().manual_seed(3)
    raw_up = T["data"]["up_field"] * (0.5 + 1.5 * torch.rand(B, 1, H, W, generator=g)) + 0.01 * torch.randn(B, 2, H, W, generator=g)
    raw_lat = torch.atanh(torch.sin(T["data"]["latitude_field"].double().clamp(-1.3, 1.3))).float()
    cam, grav = calibration(model, T["cams"], T["gravs"], dev)
    leaves = {"up": raw_up.to(dev).requires_grad_(True), "lat": raw_lat.to(dev).requires_grad_(True)}
    confs = {k: T["data"][k].to(dev).requires_grad_(True) for k in ("up_confidence", "latitude_confidence")}
    pred = {"up_field": F.normalize(leaves["up"], dim=1), "latitude_field": torch.asin(torch.tanh(leaves["lat"])), **confs}
    out = losses.perspective_field_loss(pred, cam, grav, *types, True, *lg.WEIGHTS)
    out["perspective_total"].sum().backward()
    torch.cuda.synchronize()
    assert all(c.grad is None for c in confs.values())
    # the yardstick and its gate at the device's float32 fields
    data = {"up_field": pred["up_field"].detach().cpu(), "latitude_field": pred["latitude_field"].detach().cpu(),
            "up_confidence": T["data"]["up_confidence"], "latitude_confidence": T["data"]["latitude_confidence"]}
    y = lg.yardstick(case, "all", types, data=data, gout=torch.ones(B, 2))
    # the torch path in float64 on the CPU, at the same fields
    cam64, grav64 = camera_models[model](T["cams"].double()), Gravity(T["gravs"].double())
    grav64._data = T["gravs"].double()
    p64 = {k: data[k].double().requires_grad_(True) for k in ("up_field", "latitude_field")}
    ref = losses.perspective_field_loss({**{k: v.double() for k, v in data.items()}, **p64}, cam64, grav64, *types, True, *lg.WEIGHTS)
    ref["perspective_total"].sum().backward()
    tol = 1e-5 if model == "simple_divisional" else 1e-9          # (test_field_loss_abi.py: the torch path's s' in float64)
    for k, name in (("up", "up_field"), ("lat", "latitude_field")):
        assert torch.allclose(p64[name].grad, y[f"G_{k}"], rtol=tol, atol=1e-12 + tol * y[f"G_{k}"].abs().max().item())
    # ... pulled back through the maps in float64 (from the yardstick, which the torch path has just been held to: the gate
    # is drawn around it)
    r_up, r_lat = raw_up.double().requires_grad_(True), raw_lat.double().requires_grad_(True)
    F.normalize(r_up, dim=1).backward(y["G_up"])
    torch.asin(torch.tanh(r_lat)).backward(y["G_lat"])
    n = raw_up.double().norm(dim=1, keepdim=True)
    p = data["up_field"].double()
    Gu, gate_u = y["G_up"], y["gate_up"]
    J_abs = ((torch.eye(2).reshape(1, 2, 2, 1, 1) - p[:, :, None] * p[:, None]).abs() / n[:, None])      # |J| (B, 2, 2, H, W), symmetric
    bound_up = (J_abs * gate_u[:, None]).sum(2) + 8 * U * Gu.abs().sum(1, keepdim=True) / n
    th = torch.tanh(raw_lat.double())
    J = 1 / torch.cosh(raw_lat.double())
    bound_lat = J * y["gate_lat"] + 8 * U * (J * y["G_lat"]).abs() * (1 + 2 / (1 - th * th))
    worst = {}
    for k, want, bound in (("up", r_up.grad, bound_up), ("lat", r_lat.grad, bound_lat)):
        d = (leaves[k].grad.double().cpu() - want).abs()
        worst[k] = lg._ratio(d, bound).max().item()
    print(f"{lg.case_id(case)} end to end: worst ratios {worst}")
    assert worst["up"] <= 1 and worst["lat"] <= 1, worst


def _answer(case, d, cam, grav, types, gout):
    """(losses (B, 3), grad_up, grad_lat) of fields d[...] -- fresh leaves of the same memory -- for bitwise comparisons."""
    leaves = {k: d[k].detach().requires_grad_(True) for k in ("up_field", "latitude_field")}
    out = losses.perspective_field_loss({**d, **leaves}, cam, grav, *types, True, *lg.WEIGHTS)
    ((gout[:, 0] * out["up_total"]).sum() + (gout[:, 1] * out["latitude_total"]).sum()).backward()
    return torch.stack([out["up_total"], out["latitude_total"], out["perspective_total"]], -1).detach(), leaves["up_field"].grad, \
        leaves["latitude_field"].grad


@pytest.mark.parametrize("case", [fg.CASES[0], fg.CASES[8], fg.CASES[5]], ids=fg.case_id)
def test_results_are_bit_identical_and_independent_of_the_batch(dev, case):
    T = lg.target(case)
    cam, grav = calibration(case[0], T["cams"], T["gravs"], dev)
    d = {k: on_device(v, dev, case[5]) for k, v in T["data"].items()}
    gout = torch.tensor([[0.5, -2.0]], device=dev).expand(case[1], 2)
    for types in (("l1", "huber"), ("cauchy", "l2")):
        a, b = _answer(case, d, cam, grav, types, gout), _answer(case, d, cam, grav, types, gout)
        for x, z in zip(a, b):
            assert torch.equal(x, z)
        for i in range(case[1]):                 # image i alone, its planes where they lie in the batch
            one = calibration(case[0], T["cams"][i:i + 1], T["gravs"][i:i + 1], dev)
            alone = _answer(case, {k: v[i:i + 1] for k, v in d.items()}, *one, types, gout[:1])
            for x, z in zip(alone, a):
                assert torch.equal(x[0], z[i]), (types, i)


def test_nan_and_zero_confidence_stay_in_their_image_and_field(dev):
    case = fg.CASES[2]                           # pinhole, 2 x 30 x 200
    T = lg.target(case)
    cam, grav = calibration(case[0], T["cams"], T["gravs"], dev)
    d = {k: v.to(dev) for k, v in T["data"].items()}
    gout = torch.tensor([[0.5, -2.0]], device=dev).expand(2, 2)
    for types in (("l1", "l1"), ("cauchy", "huber"), ("l2", "cauchy")):
        clean = _answer(case, d, cam, grav, types, gout)
        assert all(torch.isfinite(x).all() for x in clean)
        for field, col, f in (("up_field", 0, 0), ("up_field", 1, 0), ("latitude_field", 0, 1)):
            bad = {k: v.clone() for k, v in d.items()}
            bad[field][1, col, 10, 7] = math.nan
            loss, *grads = _answer(case, bad, cam, grav, types, gout)
            assert loss[1, f].isnan() and loss[1, 2].isnan() and torch.equal(loss[0], clean[0][0]) and torch.equal(loss[1, 1 - f], clean[0][1, 1 - f])
            nans = grads[f].isnan()
            assert nans[1, col, 10, 7] and nans.sum() == nans[1, :, 10, 7].sum(), (types, field, col)      # that pixel only
            assert torch.equal(grads[f][~nans], clean[1 + f][~nans]) and torch.equal(grads[1 - f], clean[2 - f])
        for conf, f in (("up_confidence", 0), ("latitude_confidence", 1)):
            bad = {k: v.clone() for k, v in d.items()}
            bad[conf][1] = 0.0                   # sum conf = 0: 0 / 0, as in the reference
            loss, *grads = _answer(case, bad, cam, grav, types, gout)
            assert loss[1, f].isnan() and torch.equal(loss[0], clean[0][0]) and torch.equal(loss[1, 1 - f], clean[0][1, 1 - f])
            assert grads[f][1].isnan().all() and torch.equal(grads[f][0], clean[1 + f][0]) and torch.equal(grads[1 - f], clean[2 - f])


def test_dispatch(dev, monkeypatch):
    case = fg.CASES[0]
    T = lg.target(case)
    cam, grav = calibration(case[0], T["cams"], T["gravs"], dev)
    d = {k: v.to(dev) for k, v in T["data"].items()}

    def refuse(*a, **k):
        raise AssertionError("torch path called")

    hip = losses.perspective_field_loss(d, cam, grav)
    monkeypatch.setattr(losses, "_field_loss_torch", refuse)
    assert not losses.perspective_field_loss(d, cam, grav)["perspective_total"].requires_grad
    leaf = d["up_field"].clone().requires_grad_(True)
    out = losses.perspective_field_loss({**d, "up_field": leaf}, cam, grav)                 # a field that requires grad stays on the HIP path
    assert out["up_total"].requires_grad and out["perspective_total"].requires_grad
    out["perspective_total"].sum().backward()
    assert torch.isfinite(leaf.grad).all() and leaf.grad.abs().sum() > 0
    both, scores = losses.perspective_decoder_loss({**d, "up_field": leaf}, cam, grav)     # ... and so does the scorer, on detached fields
    assert both["up_total"].requires_grad and not any(v.requires_grad for v in scores.values()) and "up_angle_recall@5" in scores
    with pytest.raises(AssertionError, match="torch path"):
        losses.perspective_field_loss({k: v.double() for k, v in d.items()}, cam, grav)
    cam_leaf = camera_models[case[0]](T["cams"].to(dev).requires_grad_(True))
    with pytest.raises(AssertionError, match="torch path"):
        losses.perspective_field_loss(d, cam_leaf, grav)
    with pytest.raises(AssertionError, match="torch path"):
        losses.perspective_field_loss({k: v.half() for k, v in d.items()}, cam, grav)
    monkeypatch.undo()
    got = losses.perspective_field_loss(d, cam_leaf, grav)                                  # the torch path carries the camera's graph
    assert got["perspective_total"].requires_grad
    for k in hip:                                # ... and agrees with the HIP path to what float32 resolves
        assert torch.allclose(got[k].detach(), hip[k], rtol=1e-4, atol=1e-6), k
    for bad in (dict(up_loss="l3"), dict(latitude_loss="dot")):
        with pytest.raises(ValueError):
            losses.perspective_field_loss(d, cam, grav, **bad)


def test_64_bit_offsets(dev):
    """B * H * W = 520 * 2048 * 2048 > 2^31: the last image's latitude plane and its gradient plane (8.7 GB each) lie beyond every
    32-bit offset.  Its loss and gradient equal those of the image run alone, bit for bit."""
    B, H, W = 520, 2048, 2048
    if torch.cuda.get_device_properties(dev).total_memory < 40 * 2 ** 30:
        pytest.skip("needs 40 GB of device memory")
    cams, gravs = pg.make_cameras("simple_radial", B, H, W, seed=9), pg.make_gravity(B, seed=9)
    cam, grav = calibration("simple_radial", cams, gravs, dev)
    moved = fg._perturbed(cams, gravs, 1.0)
    lat = pf.get_latitude_field(*calibration("simple_radial", *moved, dev)).view(B, 1, H, W).requires_grad_(True)
    batch = losses.perspective_field_loss({"latitude_field": lat}, cam, grav, latitude_loss="huber")
    batch["latitude_total"].sum().backward()
    assert sorted(batch) == ["latitude-huber-loss", "latitude_total", "perspective_total"] and batch["latitude_total"].shape == (B,)
    for i in (B - 1, 0):
        one = lat.detach()[i:i + 1].requires_grad_(True)
        alone = losses.perspective_field_loss({"latitude_field": one}, *calibration("simple_radial", cams[i:i + 1], gravs[i:i + 1], dev),
                                              latitude_loss="huber")
        alone["latitude_total"].sum().backward()
        torch.cuda.synchronize()
        assert torch.equal(alone["latitude_total"][0], batch["latitude_total"][i]) and torch.equal(one.grad[0], lat.grad[i]), i
        assert one.grad.abs().max() > 0
    assert torch.isfinite(batch["latitude_total"]).all() and 0 < batch["latitude_total"][-1] < 0.3
