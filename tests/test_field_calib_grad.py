"""GPU: `calibration_grad=True` of losses.perspective_field_loss and get_perspective_field / get_up_field / get_latitude_field
-- the gradients to `camera._data` and `gravity._data` through autograd on the HIP path (gclm_field_loss_param_grad,
gclm_perspective_fields_backward).

Accuracy: the gate of tests/field_calib_grad_gate.py against the reference's recorded gradients, every case.  Routing: with the
keyword the torch compositions are never called and backward fills the calibration's leaves; without it nothing changes -- a
calibration that requires grad takes the torch composition and no new entry is called.  Bits: with the keyword, loss values
and field gradients are the flag-off HIP values for a calibration without grad.  Launches: backward computes only what
needs_input_grad asks for.  Seam: the loss of the differentiable LM's optimised calibration reaches the fields and both
confidences through gclm_lm_backward, and the gradients handed to it agree with the flag-off route's (the torch composition
in float32) under the same gate, with a float64 torch composition on the CPU as the yardstick."""
import numpy as np
import pytest
import torch

from geocalib_amd import Gravity, LMOptimizer, _call, camera_models, losses, perspective_fields as pf
import field_calib_grad_gate as gate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def leaves(model, d, dtype=torch.float32):
    """(camera, gravity, camera leaf, gravity leaf): the gravity as stored (its constructor's normalisation bypassed)."""
    cam_leaf, grav_leaf = d["cam"].to(dtype).clone().requires_grad_(True), d["grav"].to(dtype).clone().requires_grad_(True)
    cam, grav = camera_models[model](cam_leaf), Gravity(grav_leaf.detach())
    cam._data, grav._data = cam_leaf, grav_leaf
    return cam, grav, cam_leaf, grav_leaf


def prediction(d, ul, ll, conf=True):
    pred = {}
    if ul is not None:
        pred.update(up_field=d["up"], up_confidence=d["upc"])
    if ll is not None:
        pred.update(latitude_field=d["lat"], latitude_confidence=d["latc"])
    return pred


def total_of(c, d, cam, grav, flag=True):
    """The scalar whose gradient the fixture records, from the public functions."""
    kind, ul, ll, conf, normalize = gate.parse(c[4])
    if kind == "loss":
        out = losses.perspective_field_loss(prediction(d, ul, ll), cam, grav, ul or "l1", ll or "l1", use_uncertainty_loss=conf,
                                            calibration_grad=flag)
        return (gate.grad_output(d["cam"].device).to(out["perspective_total"].dtype) * out["perspective_total"]).sum()
    if ul is not None and ll is not None and normalize:
        up, lat = pf.get_perspective_field(cam, grav, calibration_grad=flag)            # (B, 2, h, w), (B, 1, h, w): permuted views
        return (d["gup"].permute(0, 3, 1, 2) * up).sum() + (d["glat"][:, None] * lat).sum()
    t = 0
    if ul is not None:
        t = t + (d["gup"] * pf.get_up_field(cam, grav, normalize, calibration_grad=flag)).sum()
    if ll is not None:
        t = t + (d["glat"][..., None] * pf.get_latitude_field(cam, grav, calibration_grad=flag)).sum()
    return t


def refuse_torch_paths(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("torch path called")

    for mod, name in ((losses, "_field_loss_torch"), (pf, "_up_field_torch"), (pf, "_latitude_field_torch")):
        monkeypatch.setattr(mod, name, refuse)


@pytest.mark.parametrize("c", gate.cases(), ids=gate.case_id)
def test_accuracy_through_autograd(dev, monkeypatch, c):
    refuse_torch_paths(monkeypatch)
    d = gate.inputs(c[0], c[2], c[3], device=dev)
    cam, grav, cam_leaf, grav_leaf = leaves(c[1], d)
    total_of(c, d, cam, grav).backward()
    r = gate.ratios(c, cam_leaf.grad, grav_leaf.grad)
    gate.report(c, r)
    assert cam_leaf.grad.shape == (gate.B, 8) and grav_leaf.grad.shape == (gate.B, 3)
    assert torch.all(cam_leaf.grad[:, gate.unread_columns(c[1])] == 0)
    assert np.nanmax(r) <= gate.G and not np.isnan(r).any(), r


class Spy:
    """Records the names (and arguments) of the C calls made through _call.call."""

    def __init__(self, monkeypatch):
        self.calls = []
        real = _call.call

        def call(name, *a, **k):
            self.calls.append((name, a))
            return real(name, *a, **k)

        monkeypatch.setattr(_call, "call", call)

    def names(self):
        return [n for n, _ in self.calls]


NEW = {"gclm_field_loss_param_grad", "gclm_perspective_fields_backward"}


def test_routing(dev, monkeypatch):
    c = ("radial", "radial", *gate.SHAPES[0], "l1-l1-conf")
    d = gate.inputs(c[0], c[2], c[3], device=dev)
    spy = Spy(monkeypatch)
    # the default: a calibration that requires grad takes the torch compositions, no new entry is called
    cam, grav, cam_leaf, grav_leaf = leaves(c[1], d)
    total_of(c, d, cam, grav, flag=False).backward()
    up, lat = pf.get_perspective_field(cam, grav)
    (up.sum() + lat.sum()).backward()
    torch_grads = cam_leaf.grad.clone(), grav_leaf.grad.clone()
    assert not spy.names(), spy.names()
    # (the keyword reaches the loss through the decoder's pair as well; the scorer stays without a graph)
    both, scores = losses.perspective_decoder_loss(prediction(d, "l1", "l1"), cam, grav, calibration_grad=True)
    assert both["perspective_total"].requires_grad and not any(v.requires_grad for v in scores.values())
    assert spy.names()[0] == "gclm_field_loss" and not NEW & set(spy.names())
    spy.calls.clear()
    refuse_torch_paths(monkeypatch)
    with pytest.raises(AssertionError, match="torch path"):
        losses.perspective_field_loss(prediction(d, "l1", "l1"), cam, grav)
    for fn in (pf.get_perspective_field, pf.get_up_field, pf.get_latitude_field):
        with pytest.raises(AssertionError, match="torch path"):
            fn(cam, grav)
    # the keyword: the HIP path, forward and backward
    cam, grav, cam_leaf, grav_leaf = leaves(c[1], d)
    total_of(c, d, cam, grav).backward()
    up, lat = pf.get_perspective_field(cam, grav, calibration_grad=True)
    assert up.shape == (gate.B, 2, c[2], c[3]) and lat.shape == (gate.B, 1, c[2], c[3]) and up.requires_grad and lat.requires_grad
    (up.sum() + lat.sum()).backward()
    assert spy.names() == ["gclm_field_loss", "gclm_field_loss_param_grad", "gclm_perspective_fields", "gclm_perspective_fields_backward"]
    for got, want in zip((cam_leaf.grad, grav_leaf.grad), torch_grads):
        assert torch.isfinite(got).all() and got.abs().sum() > 0
        assert torch.allclose(got, want, rtol=2e-3, atol=2e-4 * want.abs().max().item())     # (one float32 composition against another)
    # inputs that cannot take the HIP path fall to the torch composition, flag or not
    cam64, grav64, _, _ = leaves(c[1], d, torch.float64)
    with pytest.raises(AssertionError, match="torch path"):
        losses.perspective_field_loss({k: v.double() for k, v in prediction(d, "l1", "l1").items()}, cam64, grav64, calibration_grad=True)
    with pytest.raises(AssertionError, match="torch path"):
        pf.get_up_field(cam64, grav64, calibration_grad=True)


def test_flag_on_keeps_the_bits_of_a_calibration_without_grad(dev, monkeypatch):
    for model in ("pinhole", "radial"):
        d = gate.inputs(model, *gate.SHAPES[3], device=dev)
        cam, grav = camera_models[model](d["cam"]), Gravity(d["grav"])
        res = []
        for flag in (False, True):
            spy = Spy(monkeypatch)
            pred = {k: v.clone().requires_grad_(k.endswith("_field")) for k, v in prediction(d, "huber", "cauchy").items()}
            out = losses.perspective_field_loss(pred, cam, grav, "huber", "cauchy", calibration_grad=flag)
            out["perspective_total"].sum().backward()
            up, lat = pf.get_perspective_field(cam, grav, calibration_grad=flag)
            assert not up.requires_grad and not lat.requires_grad
            res.append(({k: v.detach() for k, v in out.items()}, pred["up_field"].grad, pred["latitude_field"].grad, up, lat))
            assert spy.names() == ["gclm_field_loss", "gclm_field_loss_grad", "gclm_perspective_fields"], spy.names()
            monkeypatch.undo()
        off, on = res
        assert all(torch.equal(off[0][k], on[0][k]) for k in off[0])
        assert all(torch.equal(a, b) for a, b in zip(off[1:], on[1:]))


def test_backward_computes_only_what_is_asked_for(dev, monkeypatch):
    c = ("simple_radial", "simple_radial", *gate.SHAPES[0], "cauchy-huber-conf")
    d = gate.inputs(c[0], c[2], c[3], device=dev)
    full_cam, full_grav, cl, gl = leaves(c[1], d)
    total_of(c, d, full_cam, full_grav).backward()
    want = cl.grad, gl.grad
    spy = Spy(monkeypatch)
    # gravity alone: the same gravity bits, a NULL camera gradient, no field-gradient pass
    cam, grav, cam_leaf, grav_leaf = leaves(c[1], d)
    cam._data = cam_leaf.detach()
    total_of(c, d, cam, grav).backward()
    assert spy.names() == ["gclm_field_loss", "gclm_field_loss_param_grad"]
    assert spy.calls[1][1][-3] is None and spy.calls[1][1][-2] is not None and torch.equal(grav_leaf.grad, want[1])
    # camera alone, with a field that requires grad: both passes, the field's pass without the other field
    spy.calls.clear()
    cam, grav, cam_leaf, grav_leaf = leaves(c[1], d)
    grav._data = grav_leaf.detach()
    up = d["up"].clone().requires_grad_(True)
    out = losses.perspective_field_loss({**prediction(d, "cauchy", "huber"), "up_field": up}, cam, grav, "cauchy", "huber", calibration_grad=True)
    (gate.grad_output(dev) * out["perspective_total"]).sum().backward()
    assert spy.names() == ["gclm_field_loss", "gclm_field_loss_grad", "gclm_field_loss_param_grad"]
    grad_call, param_call = spy.calls[1][1], spy.calls[2][1]
    assert grad_call[7] is None and grad_call[9] is None and grad_call[6] is not None         # latitude and its confidence left out
    assert param_call[6] is not None and param_call[7] is not None and param_call[-2] is None
    assert torch.equal(cam_leaf.grad, want[0]) and torch.isfinite(up.grad).all() and up.grad.abs().sum() > 0
    # the rendered fields: a cotangent for one output only, gravity alone
    spy.calls.clear()
    cam, grav, cam_leaf, grav_leaf = leaves(c[1], d)
    cam._data = cam_leaf.detach()
    up_f, lat_f = pf.get_perspective_field(cam, grav, calibration_grad=True)
    (d["glat"][:, None] * lat_f).sum().backward()
    assert spy.names() == ["gclm_perspective_fields", "gclm_perspective_fields_backward"] and spy.calls[1][1][-3] is None
    alone = leaves(c[1], d)
    (d["glat"][..., None] * pf.get_latitude_field(alone[0], alone[1], calibration_grad=True)).sum().backward()
    assert torch.equal(grav_leaf.grad, alone[3].grad)          # (the unused up field gets no cotangent plane: the same pass)
    assert spy.calls[1][1][7] is None and spy.calls[1][1][8] is not None


def _yardstick(model, d, cam_data, grav_data, types):
    """(ref64, A), each (B, 11): the float64 torch composition on the CPU at the given calibration, and per entry the sum over
    pixels of |that pixel's contribution| (tests/golden/make_golden_field_calib_grad.py forms the fixture's the same way)."""
    d = {k: v.detach().double().cpu() for k, v in d.items()}
    cam_data, grav_data = cam_data.detach().double().cpu(), grav_data.detach().double().cpu()

    def targets(c, g):
        cam, grav = camera_models[model](c), Gravity(g.detach())
        grav._data = g
        return pf.get_perspective_field(cam, grav)

    def total(up_t, lat_t):
        return (losses.field_loss(d["up"], up_t, d["upc"], types[0]) + losses.field_loss(d["lat"], lat_t, d["latc"], types[1])).sum()

    c, g = cam_data.clone().requires_grad_(True), grav_data.clone().requires_grad_(True)
    ref = torch.cat(torch.autograd.grad(total(*targets(c, g)), [c, g]), 1)
    with torch.no_grad():
        t0 = [t.clone() for t in targets(cam_data, grav_data)]
    t0 = [t.requires_grad_(True) for t in t0]
    cot = torch.autograd.grad(total(*t0), t0)
    A = torch.zeros_like(ref)
    for j in range(11):
        tc, tg = torch.zeros_like(cam_data), torch.zeros_like(grav_data)
        (tc if j < 8 else tg)[:, j if j < 8 else j - 8] = 1.0
        _, tangents = torch.autograd.functional.jvp(targets, (cam_data, grav_data), (tc, tg))
        A[:, j] = sum((g_ * t_).sum(1) for g_, t_ in zip(cot, tangents)).abs().sum((1, 2))
    return ref.numpy(), A.numpy()


@pytest.mark.parametrize("model", ["pinhole", "simple_radial"])
def test_seam_with_the_differentiable_lm(dev, model):
    H, W = gate.SHAPES[0]
    d = gate.inputs(model, H, W, device=dev)
    types = ("l1", "huber")
    grads = {}
    for flag in (True, False):
        data = {k: v.clone().requires_grad_(True) for k, v in prediction(d, *types).items()}
        out = LMOptimizer({"camera_model": model, "differentiable": True, "num_steps": 3}).train()(dict(data))
        cam, grav = out["camera"], out["gravity"]
        assert cam._data.requires_grad and grav._data.requires_grad
        handed = {}
        cam._data.register_hook(lambda g: handed.__setitem__("cam", g.clone()))
        grav._data.register_hook(lambda g: handed.__setitem__("grav", g.clone()))
        loss = losses.perspective_field_loss({k: v.detach() for k, v in data.items()}, cam, grav, *types, calibration_grad=flag)
        loss["perspective_total"].sum().backward()
        for k, v in data.items():
            assert v.grad is not None and torch.isfinite(v.grad).all() and v.grad.abs().sum() > 0, (flag, k)
        grads[flag] = (handed["cam"], handed["grav"], cam._data.detach(), grav._data.detach())
    assert torch.equal(grads[True][2], grads[False][2]) and torch.equal(grads[True][3], grads[False][3])     # one solve, two losses
    ref64, A = _yardstick(model, d, grads[True][2], grads[True][3], types)
    hip, flag_off = (np.concatenate([g[0].double().cpu().numpy(), g[1].double().cpu().numpy()], 1) for g in (grads[True], grads[False]))
    unit = np.maximum(np.abs(flag_off - ref64), 2.0 ** -23 * A)
    err = np.abs(hip - ref64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / unit)
    print(f"seam {model}: worst {r.max():.3f} median {np.median(r[r > 0]):.3f}")
    assert r.max() <= gate.G, r


# ------------------------------------------------------------------ the branches the fixture stays clear of
def _planes_backward(model, cam, grav, gup, glat, dev):
    from geocalib_amd import fields
    return torch.cat(fields.perspective_fields_backward(model, cam.to(dev), grav.to(dev), gup.to(dev), glat.to(dev)), 1).double().cpu()


def _hold(got, want, what):
    tol = 2e-5 * want.abs() + 1e-5 * want.abs().amax(1, keepdim=True).clamp(max=1.0) + 1e-6
    print(f"{what}: worst |hip - ref| / tol {((got - want).abs() / tol).max():.3f}")
    assert torch.isfinite(got).all() and ((got - want).abs() <= tol).all(), (what, got, want)


@pytest.mark.parametrize("model", ["pinhole", "simple_radial"])
def test_latitude_clamp_and_norm_floor(dev, model):
    """Gravity along the optical axis and the principal point on a pixel: at that pixel q = (0, 0) exactly, so F.normalize's
    1e-12 floor acts (a constant norm: the cotangent times 1e12), and sin(latitude) = 1, beyond the clamp (no gradient).
    The yardstick is the package's torch composition in float64 on the CPU, whose F.normalize and clamp autograd treats so."""
    H, W, B = 6, 9, 2
    g = torch.Generator().manual_seed(11)
    cam = torch.tensor([[W, H, 7.0, 7.5, 4.0, 2.0, 0.1 if model != "pinhole" else 0.0, 0.0],
                        [W, H, 8.0, 7.0, 3.0, 3.0, -0.1 if model != "pinhole" else 0.0, 0.0]])
    grav = torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]])
    gup, glat = torch.rand(B, H, W, 2, generator=g) - 0.5, torch.rand(B, H, W, generator=g) - 0.5
    c, gr, cl, gl = leaves(model, {"cam": cam, "grav": grav}, torch.float64)
    up, lat = pf.get_perspective_field(c, gr)                                 # the torch composition, float64, CPU
    assert (up[0, :, 2, 4] == 0).all() and lat[0, 0, 2, 4] > 1.569           # the floor and the clamp act
    ((gup.double().permute(0, 3, 1, 2) * up).sum() + (glat.double()[:, None] * lat).sum()).backward()
    want = torch.cat([cl.grad, gl.grad], 1)
    assert want.abs().max() > 1e10                                            # (the floor's 1e12 is in there)
    _hold(_planes_backward(model, cam, grav, gup, glat, dev), want, f"clamp and floor, {model}")


def test_simple_divisional_beyond_its_singular_circle(dev):
    """k1 = 2: tau = 1 - 4 k1 r2 is negative over the outer part of the image (s = 1 / (2 k1 r2), s' the reference's clamped
    expression) and positive inside.  The yardstick restates include/gclm.h's forms per branch in float64 torch."""
    H, W, B = 9, 12, 2
    g = torch.Generator().manual_seed(12)
    cam = torch.tensor([[W, H, 11.0, 11.7, 5.63, 4.21, 2.0, 0.0], [W, H, 12.0, 11.0, 6.37, 3.79, 1.5, 0.0]])
    grav = torch.nn.functional.normalize(torch.tensor([[0.2, -0.9, 0.3], [-0.1, -0.95, -0.25]]), dim=-1)
    gup, glat = torch.rand(B, H, W, 2, generator=g) - 0.5, torch.rand(B, H, W, generator=g) - 0.5
    c, gr = cam.double().requires_grad_(True), grav.double().requires_grad_(True)
    fx, fy, cx, cy, k1 = (c[:, i, None, None] for i in range(2, 7))
    a, b, cc = (gr[:, i, None, None] for i in range(3))
    x, y = torch.arange(W, dtype=torch.float64)[None, None, :], torch.arange(H, dtype=torch.float64)[None, :, None]
    u, v = ((x - cx) / fx).expand(B, H, W), ((y - cy) / fy).expand(B, H, W)
    r2 = u * u + v * v
    kr = k1 * r2
    tau = 1 - 4 * kr
    inside = tau.detach() >= 1e-6
    assert inside.any() and (tau.detach() <= 0).any() and not ((tau.detach() > 0) & ~inside).any()
    rt = torch.sqrt(torch.where(inside, tau, torch.ones_like(tau)))             # (safe under the mask)
    s = torch.where(inside, 2 / (1 + rt), 1 / (2 * kr))
    tt = 1e-3
    sp = torch.where(inside, 4 * k1 / (rt * (1 + rt) ** 2), (2 * kr - (1 - tt) * tt) / (2 * k1 * r2 ** 2 * tt))
    px, py = a - cc * u, b - cc * v
    o = 2 * sp * (u * px + v * py)
    q = torch.stack([s * px + o * u, s * py + o * v], -1)
    up = q / q.norm(dim=-1, keepdim=True)
    t = 1 / (1 + kr)
    X, Y = u * t, v * t
    lat = torch.asin(((X * a + Y * b + cc) / torch.sqrt(X * X + Y * Y + 1)).clamp(-1 + 1e-6, 1 - 1e-6))
    ((gup.double() * up).sum() + (glat.double() * lat).sum()).backward()
    want = torch.cat([c.grad, gr.grad], 1)
    _hold(_planes_backward("simple_divisional", cam, grav, gup, glat, dev), want, "simple_divisional, tau <= 0")
