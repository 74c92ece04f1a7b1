"""GPU: fields.pack_fields with a graph -- the typed forward (gclm_pack_fields_typed) and the head epilogue's backward
(gclm_pack_fields_backward) behind a torch.autograd.Function.

The yardstick of every accuracy test is the reference's four lines (UpDecoder._forward / LatitudeDecoder._forward), written
out below as `torch_lines` and run through autograd in float64 on the float32 (or widened 16-bit) inputs; the unit of an error
is the error of the same lines run in float32 on the same device.  No package function stands in for them.

Every test that reads planes runs over the walks of the two kernels: H W odd (scalar), H W a multiple of 4 but not of 8
(vector for float32, scalar for the 16-bit types), a multiple of 8 (vector for all), and that shape with one tensor whose
storage starts one element into its allocation (scalar again)."""
import math

import pytest
import torch
import torch.nn.functional as F

from geocalib_amd import LMOptimizer, _call, _lib
from geocalib_amd.camera import camera_models
from geocalib_amd.fields import pack_fields
from geocalib_amd.gravity import Gravity
from geocalib_amd.losses import perspective_field_loss
from geocalib_amd.perspective_fields import get_perspective_field

pytestmark = pytest.mark.gpu

WALKS = [(3, 5, 7, False), (2, 6, 6, False), (2, 8, 12, False), (2, 8, 12, True)]
WALK_IDS = ["3x5x7", "2x6x6", "2x8x12", "2x8x12-misaligned"]
HALVES = [torch.float16, torch.bfloat16]
OUT_KEYS = ("up_field", "latitude_field", "up_confidence", "latitude_confidence")
EPS = 2.0 ** -23
RATIO = 4.0      # an error of the HIP backward against the float64 yardstick, in units of the float32 torch lines' error


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def torch_lines(up_raw, lat_raw, up_log_confidence=None, lat_log_confidence=None):
    up_field = F.normalize(up_raw, dim=1)
    latitude_field = torch.asin(torch.clamp(torch.tanh(lat_raw), -1 + 1e-5, 1 - 1e-5))
    up_confidence = None if up_log_confidence is None else torch.sigmoid(up_log_confidence)
    latitude_confidence = None if lat_log_confidence is None else torch.sigmoid(lat_log_confidence)
    return up_field, latitude_field, up_confidence, latitude_confidence


def same_bits(a, b):
    view = torch.int32 if a.dtype is torch.float32 else torch.int16
    return a.dtype is b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def offset_by_one(t):
    """`t`'s values in storage that starts one element into an allocation: contiguous, never 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t.reshape(-1)
    return buf[1:].view(t.shape)


def make_raws(dev, B, H, W, misaligned=False, seed=0, dtype=torch.float32):
    """The inputs of the accuracy test: up raws N(0, 1), a tenth of the pixels scaled by 1e-3; latitude raws N(0, 2) clipped to
    |x| <= 5.5; log-confidences N(0, 3), the latitude's as (B, 1, H, W); and the incoming gradients N(0, 1) of the four outputs."""
    g = torch.Generator().manual_seed(1000 * seed + 100 * B + H * W)
    up_raw = torch.randn(B, 2, H, W, generator=g)
    up_raw = torch.where(torch.rand(B, 1, H, W, generator=g) < 0.1, up_raw * 1e-3, up_raw)
    lat_raw = (2 * torch.randn(B, 1, H, W, generator=g)).clamp(-5.5, 5.5)
    ulc, llc = 3 * torch.randn(B, H, W, generator=g), 3 * torch.randn(B, 1, H, W, generator=g)
    grads = [torch.randn(s, generator=g).to(dev) for s in ((B, 2, H, W), (B, 1, H, W), (B, H, W), (B, H, W))]
    raws = [t.to(dtype).to(dev) for t in (up_raw, lat_raw, ulc, llc)]
    if misaligned:
        raws[0] = offset_by_one(raws[0])
        assert raws[0].data_ptr() % 16 != 0 and raws[0].is_contiguous()
    return raws, grads


def backward_of(fn, raws, grads, wanted=(0, 1, 2, 3)):
    """(outputs, gradients of the raws of `wanted`) under the incoming `grads` of every output that carries a graph, through
    `fn`; a None raw is absent."""
    leaves = [None if t is None else t.detach().clone().requires_grad_(i in wanted) for i, t in enumerate(raws)]
    if raws[0].data_ptr() % 16 != 0:
        leaves[0] = offset_by_one(raws[0].detach()).requires_grad_(0 in wanted)
    out = fn(*leaves)
    pairs = [(o, g.reshape(o.shape)) for o, g in zip(out, grads) if o is not None and o.requires_grad]
    got = torch.autograd.grad([o for o, _ in pairs], [t for t in leaves if t is not None and t.requires_grad], [g for _, g in pairs])
    return out, got


def hip_lines(*raws):
    out = pack_fields(raws[0], raws[1], raws[2], raws[3])
    return tuple(out.get(k) for k in OUT_KEYS)


def ex_call(raws, sin_latitude=True):
    """gclm_pack_fields_ex itself, on float32 raws: the six planes."""
    up_raw, lat_raw, ulc, llc = raws
    B, _, H, W = lat_raw.shape
    up, lat, slat = torch.empty_like(up_raw), torch.empty_like(lat_raw), torch.empty_like(lat_raw)
    upc = None if ulc is None else torch.empty_like(ulc).view(B, H, W)
    latc = None if llc is None else torch.empty_like(llc).view(B, H, W)
    p = _call.ptr
    _call.call("gclm_pack_fields_ex", p(up_raw), p(ulc), p(lat_raw), p(llc), B, H, W, p(up), p(upc), p(lat), p(latc),
               p(slat) if sin_latitude else None, _call.raw_stream(lat_raw.device), device=lat_raw.device)
    return up, lat, upc, latc, slat


# ------------------------------------------------------------------ 1. the plain path, and the graph on top of it
@pytest.mark.parametrize("B,H,W,misaligned", WALKS, ids=WALK_IDS)
def test_plain_path_is_unchanged_and_the_graph_returns_its_bits(dev, B, H, W, misaligned):
    raws, _ = make_raws(dev, B, H, W, misaligned)
    want = ex_call(raws)
    with torch.no_grad():
        plain = pack_fields(*raws[:2], raws[2], raws[3], sin_latitude=True)
    for k, w in zip(OUT_KEYS + ("sin_latitude",), want):
        assert same_bits(plain[k], w) and plain[k].grad_fn is None and not plain[k].requires_grad, k
    for t in raws:
        t.requires_grad_(True)
    with torch.no_grad():
        plain = pack_fields(*raws[:2], raws[2], raws[3], sin_latitude=True)
    assert all(same_bits(plain[k], w) and not plain[k].requires_grad for k, w in zip(OUT_KEYS + ("sin_latitude",), want))
    out = pack_fields(*raws[:2], raws[2], raws[3], sin_latitude=True)
    for k, w in zip(OUT_KEYS + ("sin_latitude",), want):
        assert same_bits(out[k], w), k
    assert all(out[k].grad_fn is not None for k in OUT_KEYS)
    assert out["sin_latitude"].grad_fn is None and not out["sin_latitude"].requires_grad
    assert out["up_confidence"].shape == out["latitude_confidence"].shape == (B, H, W)


# ------------------------------------------------------------------ 2. the typed forward
@pytest.mark.parametrize("confidences", [True, False], ids=["confidences", "no-confidences"])
@pytest.mark.parametrize("dtype", HALVES, ids=str)
@pytest.mark.parametrize("B,H,W,misaligned", WALKS, ids=WALK_IDS)
def test_half_raws_give_the_bits_of_the_widened_planes(dev, B, H, W, misaligned, dtype, confidences):
    raws, _ = make_raws(dev, B, H, W, misaligned, seed=1, dtype=dtype)
    if not confidences:
        raws[2] = raws[3] = None
    got = pack_fields(raws[0], raws[1], raws[2], raws[3], sin_latitude=True)
    wide = [None if t is None else t.float() for t in raws]
    want = pack_fields(wide[0], wide[1], wide[2], wide[3], sin_latitude=True)
    assert list(got) == list(want) and len(got) == (5 if confidences else 3)
    for k in want:
        assert got[k].dtype is torch.float32 and same_bits(got[k], want[k]), k
    for w, t in zip(ex_call(wide), (want.get(k) for k in OUT_KEYS + ("sin_latitude",))):
        assert (w is None and t is None) or same_bits(w, t)


# ------------------------------------------------------------------ 3. the backward against float64
def plane_errors(got, want):
    """Per image and plane: max |got - want| / max |want|, `want` in float64."""
    got, want = got.double().reshape(-1, *got.shape[-2:]), want.reshape(-1, *want.shape[-2:])
    return (got - want).abs().amax(dim=(1, 2)) / want.abs().amax(dim=(1, 2))


@pytest.mark.parametrize("B,H,W,misaligned", WALKS, ids=WALK_IDS)
def test_backward_against_the_float64_torch_lines(dev, B, H, W, misaligned):
    raws, grads = make_raws(dev, B, H, W, misaligned, seed=2)
    _, want = backward_of(torch_lines, [t.double() for t in raws], [g.double() for g in grads])
    _, unit = backward_of(torch_lines, raws, grads)
    _, got = backward_of(hip_lines, raws, grads)
    for name, g, u, w, t in zip(("up_raw", "lat_raw", "up_log_confidence", "lat_log_confidence"), got, unit, want, raws):
        assert g.dtype is torch.float32 and g.shape == t.shape and g.is_contiguous(), name
        e_hip, e_torch = plane_errors(g, w), plane_errors(u, w)
        print(f"{name} {B}x{H}x{W}{' misaligned' if misaligned else ''}: HIP error {e_hip.max().item():.3e}, float32 torch error "
              f"{e_torch.max().item():.3e}, ratio per image and plane {[round(r, 2) for r in (e_hip / e_torch).tolist()]}")
        assert (e_hip <= RATIO * e_torch).all(), (name, e_hip.tolist(), e_torch.tolist())
    # the up gradient is orthogonal to the raw vector wherever the norm is not clamped
    r, d = raws[0].double(), got[0].double()
    live = r.norm(dim=1) > 1e-12
    dot, bound = (d * r).sum(1).abs(), 16 * EPS * d.norm(dim=1) * r.norm(dim=1)
    assert live.all() and (dot[live] <= bound[live]).all(), (dot[live] / (d.norm(dim=1) * r.norm(dim=1))[live]).max().item() / EPS


# ------------------------------------------------------------------ 4. planted pixels
def ulps_apart(a, b):
    return (a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs()


def test_planted_pixels_have_their_exact_gradients(dev):
    inf, nan = float("inf"), float("nan")
    up_px = [(0.0, 0.0), (3e-13, 4e-13), (6e-13, 8e-13), (0.5, -2.0)]
    lat_px = [0.0, 20.0, -20.0, inf, -inf, nan, 1.0]
    conf_px = [0.0, 100.0, -100.0, 1.0]
    g = torch.Generator().manual_seed(4)
    for W in (8, 7):                                        # one row of 8 pixels: the vector walk; of 7: the scalar walk
        up_raw = torch.randn(1, 2, 1, W, generator=g)
        lat_raw, ulc, llc = torch.randn(1, 1, 1, W, generator=g), torch.randn(1, 1, W, generator=g), torch.randn(1, 1, W, generator=g)
        for i, (x, y) in enumerate(up_px):
            up_raw[0, 0, 0, i], up_raw[0, 1, 0, i] = x, y
        for i, x in enumerate(lat_px):
            lat_raw[0, 0, 0, i] = x
        for i, x in enumerate(conf_px):
            ulc[0, 0, i], llc[0, 0, W - 1 - i] = x, x
        raws = [t.to(dev) for t in (up_raw, lat_raw, ulc, llc)]
        grads = [(torch.randn(s, generator=g).abs() + 0.25).to(dev) * sign
                 for s, sign in (((1, 2, 1, W), 1), ((1, 1, 1, W), -1), ((1, 1, W), 1), ((1, 1, W), -1))]
        _, (d_up, d_lat, d_ulc, d_llc) = backward_of(hip_lines, raws, grads)
        g_up, g_lat, g_ulc, g_llc = grads
        # up: the clamped branch of F.normalize is g / 1e-12, the float32 quotient to one ulp
        quotient = g_up / torch.tensor(1e-12, dtype=torch.float32, device=dev)
        for i in (0, 1):
            assert (ulps_apart(d_up[0, :, 0, i], quotient[0, :, 0, i]) <= 1).all(), (W, i, d_up[0, :, 0, i], quotient[0, :, 0, i])
        # ... and a norm exactly at the clamp is projected: (g - u (u . g)) / n in float64 on the float32 raws, held to a few
        # roundings of |g| / n (u, the product, the quotient), and nowhere near g / 1e-12
        for i in (2, 3):
            r, gg = raws[0][0, :, 0, i].double(), g_up[0, :, 0, i].double()
            nrm = r.norm()
            assert nrm.float() >= torch.tensor(1e-12, dtype=torch.float32)
            want = (gg - r / nrm * (r / nrm * gg).sum()) / nrm
            assert ((d_up[0, :, 0, i].double() - want).abs() <= 8 * EPS * gg.norm() / nrm).all(), (W, i, d_up[0, :, 0, i], want)
            assert (d_up[0, :, 0, i].double() * r).sum().abs() <= 16 * EPS * d_up[0, :, 0, i].double().norm() * nrm
        assert (ulps_apart(d_up[0, :, 0, 2], quotient[0, :, 0, 2]) > 1000).any()
        # latitude
        assert same_bits(d_lat[0, 0, 0, 0], g_lat[0, 0, 0, 0])                                   # raw 0: exactly g
        assert (d_lat[0, 0, 0, 1:5].view(torch.int32) << 1 == 0).all(), d_lat[0, 0, 0, 1:5]       # +-20, +-inf: exactly 0
        assert torch.isnan(d_lat[0, 0, 0, 5]) and torch.isfinite(d_lat[0, 0, 0, 6])
        # (raw 1: expf to an ulp, then four roundings -- well inside 8 eps)
        sech = 1 / math.cosh(1.0)
        assert abs(d_lat[0, 0, 0, 6].item() / g_lat[0, 0, 0, 6].item() - sech) <= 8 * EPS * sech
        # ... the NaN stays in its own plane
        assert torch.isfinite(d_up).all() and torch.isfinite(d_ulc).all() and torch.isfinite(d_llc).all()
        assert int(torch.isnan(d_lat).sum()) == 1
        # confidences
        for d, gc, at in ((d_ulc, g_ulc, lambda i: i), (d_llc, g_llc, lambda i: W - 1 - i)):
            assert same_bits(d[0, 0, at(0)], gc[0, 0, at(0)] / 4)                                 # raw 0: exactly g / 4
            for i in (1, 2):
                v = d[0, 0, at(i)]
                assert torch.isfinite(v) and abs(v.item()) < 1e-30, (W, i, v)
            s = 1 / (1 + math.exp(-1.0))
            assert abs(d[0, 0, at(3)].item() / gc[0, 0, at(3)].item() - s * (1 - s)) <= 8 * EPS * s * (1 - s)


def test_a_nan_in_any_group_stays_in_its_group(dev):
    raws, grads = make_raws(dev, 1, 2, 4, seed=5)
    for k in range(4):
        bad = [t.clone() for t in raws]
        bad[k].view(-1)[3] = float("nan")
        _, got = backward_of(hip_lines, bad, grads)
        for j, d in enumerate(got):
            assert int(torch.isnan(d).sum()) == ((2 if k == 0 else 1) if j == k else 0), (k, j, d)


# ------------------------------------------------------------------ 5. the clamp band
@pytest.mark.parametrize("rows", [2, 4], ids=["scalar-walk", "vector-walk"])
def test_forward_and_backward_agree_on_every_pixel_of_the_clamp_band(dev, rows):
    x = torch.linspace(6.05, 6.16, 2001, dtype=torch.float64)
    assert x[0] < math.atanh(1 - 1e-5) < x[-1]
    lat_raw = torch.stack([x, -x] * (rows // 2)).float().view(1, 1, rows, 2001).to(dev)      # 2 x 2001 is no multiple of 4
    g = torch.Generator().manual_seed(6)
    up_raw = torch.randn(1, 2, rows, 2001, generator=g).to(dev)
    g_lat = (0.5 + torch.rand(1, 1, rows, 2001, generator=g)).to(dev)
    leaf = lat_raw.clone().requires_grad_(True)
    out = pack_fields(up_raw, leaf)
    (d,) = torch.autograd.grad(out["latitude_field"], leaf, g_lat)
    lat, d, a = out["latitude_field"].detach().view(-1), d.view(-1), lat_raw.view(-1).abs()
    want = (g_lat.double() / torch.cosh(lat_raw.double())).view(-1)
    err = (d.double() - want).abs() / want.abs()
    # the unit: the float32 torch lines' own per-pixel error below the band, where they certainly do not clamp
    leaf32 = lat_raw.clone().requires_grad_(True)
    (u,) = torch.autograd.grad(torch_lines(up_raw, leaf32)[1], leaf32, g_lat)
    below, above, inside = a < 6.08, a > 6.13, (a >= 6.08) & (a <= 6.13)
    assert int(below.sum()) > 1000 and int(above.sum()) > 1000 and int(inside.sum()) > 1800
    gate = RATIO * ((u.view(-1).double() - want).abs() / want.abs())[below].max()
    print(f"clamp band: HIP error below the band {err[below].max().item():.3e}, gate {gate.item():.3e}; first zero gradient at "
          f"|x| = {a[d == 0].min().item():.5f}, last non-zero at {a[d != 0].max().item():.5f}")
    assert (err[below] <= gate).all(), (err[below].max().item(), gate.item())
    assert (d[above].view(torch.int32) << 1 == 0).all()
    assert ((d[inside] == 0) | (err[inside] <= gate)).all()
    # every pixel the forward did not clamp has a gradient: its latitude lies strictly inside the largest value written
    top = lat.abs().max()
    assert abs(top.item() - math.asin(1 - 1e-5)) < 1e-3 and int((lat.abs() == top).sum()) > 1000
    unclamped = lat.abs().view(torch.int32) < top.view(torch.int32)
    assert int(unclamped.sum()) > 500 and (d[unclamped] != 0).all()
    assert (lat.abs()[d == 0] == top).all()                      # ... and a zero gradient only where the forward wrote the bound


# ------------------------------------------------------------------ 6. 16-bit raws
@pytest.mark.parametrize("dtype", HALVES, ids=str)
@pytest.mark.parametrize("B,H,W,misaligned", WALKS, ids=WALK_IDS)
def test_half_backward_is_the_float32_backward_rounded(dev, B, H, W, misaligned, dtype):
    raws, grads = make_raws(dev, B, H, W, misaligned, seed=7, dtype=dtype)
    out, got = backward_of(hip_lines, raws, grads)
    out32, want = backward_of(hip_lines, [t.float() for t in raws], grads)
    assert all(same_bits(a, b) for a, b in zip(out, out32))
    for g, w, t in zip(got, want, raws):
        assert g.dtype is dtype and g.shape == t.shape and w.dtype is torch.float32
        assert same_bits(g, w.to(dtype))


# ------------------------------------------------------------------ 7. subsets
@pytest.mark.parametrize("absent", [(), (2,), (3,), (2, 3)], ids=["both-confidences", "no-up-confidence", "no-latitude-confidence",
                                                                  "no-confidence"])
@pytest.mark.parametrize("B,H,W,misaligned", WALKS, ids=WALK_IDS)
def test_one_output_alone_gives_its_raws_the_bits_of_the_full_call(dev, B, H, W, misaligned, absent):
    raws, grads = make_raws(dev, B, H, W, misaligned, seed=8)
    raws = [None if i in absent else t for i, t in enumerate(raws)]
    present = [i for i in range(4) if i not in absent]
    _, full = backward_of(hip_lines, raws, grads)
    full = dict(zip(present, full))
    for k in present:
        leaves = [None if t is None else t.detach().requires_grad_(True) for t in raws]
        out = hip_lines(*leaves)
        got = torch.autograd.grad(out[k], [leaves[i] for i in present], grads[k], allow_unused=True)
        for i, d in zip(present, got):
            assert (d is None) if i != k else same_bits(d, full[k]), (k, i)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
@pytest.mark.parametrize("B,H,W,misaligned", WALKS, ids=WALK_IDS)
def test_one_raw_alone_gets_its_gradient_and_nothing_else_is_written(dev, B, H, W, misaligned, dtype):
    raws, grads = make_raws(dev, B, H, W, misaligned, seed=9, dtype=dtype)
    _, full = backward_of(hip_lines, raws, grads)
    lib, p = _lib.load(), _call.ptr
    torch.cuda.synchronize()
    for k in range(4):
        out, got = backward_of(hip_lines, raws, grads, wanted=(k,))
        assert len(got) == 1 and same_bits(got[0], full[k]), k
        assert all((out[i].grad_fn is not None) for i in range(4))
        # the entry itself: one gradient asked for, inside a sentinel-filled buffer with room for all four and guards around
        n, pad = raws[k].numel(), 64
        buf = torch.full((4 * (n + 2 * pad),), -77.0, dtype=dtype, device=dev)
        lo = k * (n + 2 * pad) + pad + (1 if misaligned else 0)
        d = [None] * 4
        d[k] = buf[lo:lo + n]
        rc = lib.gclm_pack_fields_backward(_lib.LOGIT_DTYPE_IDS[str(dtype)[6:]], p(raws[0]), p(raws[2]), p(raws[1]), p(raws[3]), B, H, W,
                                           p(grads[0]), p(grads[2]), p(grads[1]), p(grads[3]), p(d[0]), p(d[2]), p(d[1]), p(d[3]),
                                           _call.raw_stream(dev))
        assert rc == 0
        torch.cuda.synchronize()
        assert same_bits(buf[lo:lo + n].view(raws[k].shape), full[k]), k
        assert (buf[:lo] == -77).all() and (buf[lo + n:] == -77).all(), k


# ------------------------------------------------------------------ 8. the chain
def test_loss_and_lm_gradients_reach_the_raws_as_the_two_stage_computation(dev):
    B, H, W = 2, 24, 32
    g = torch.Generator().manual_seed(10)
    cam = torch.tensor([[W, H, 30.0, 30.0, W / 2, H / 2, 0.0, 0.0], [W, H, 22.0, 22.0, W / 2, H / 2, 0.0, 0.0]], device=dev)
    camera = camera_models["pinhole"](cam)
    gravity = Gravity.from_rp(torch.tensor([0.1, -0.2]), torch.tensor([0.15, -0.05])).to(dev)
    up, lat = get_perspective_field(camera, gravity)
    up_raw = (2 * up.contiguous() + 0.02 * torch.randn(B, 2, H, W, generator=g).to(dev)).requires_grad_(True)
    lat_raw = (torch.atanh(torch.sin(lat.contiguous())) + 0.02 * torch.randn(B, 1, H, W, generator=g).to(dev)).requires_grad_(True)
    ulc = torch.randn(B, H, W, generator=g).to(dev).requires_grad_(True)
    llc = torch.randn(B, 1, H, W, generator=g).to(dev).requires_grad_(True)
    raws = [up_raw, lat_raw, ulc, llc]
    opt = LMOptimizer({"camera_model": "pinhole", "differentiable": True, "num_steps": 3}).train()
    data = {"camera": camera, "gravity": gravity}

    def loss_of(fields):
        pred = {**fields, **opt(fields)}
        return perspective_field_loss(fields, camera, gravity)["perspective_total"].sum() + opt.loss(pred, data)[0]["param_total"].sum()

    fields = pack_fields(up_raw, lat_raw, ulc, llc)
    loss = loss_of(fields)
    loss.backward()
    assert all(t.grad is not None and t.grad.shape == t.shape and torch.isfinite(t.grad).all() and t.grad.abs().max() > 0 for t in raws)
    # two stages: the same loss from detached fields as leaves, then pack_fields' backward alone under those field gradients
    fields2 = pack_fields(up_raw, lat_raw, ulc, llc)
    leaves = {k: v.detach().requires_grad_(True) for k, v in fields2.items()}
    loss2 = loss_of(leaves)
    assert same_bits(loss2.detach(), loss.detach())
    field_grads = torch.autograd.grad(loss2, [leaves[k] for k in OUT_KEYS])
    two_stage = torch.autograd.grad([fields2[k] for k in OUT_KEYS], raws, field_grads)
    for t, w in zip(raws, two_stage):
        assert same_bits(t.grad, w)


# ------------------------------------------------------------------ 9. more images than one grid's y-extent
def test_a_batch_beyond_65535_images_equals_two_calls(dev):
    B, cut = 65537, 65535
    g = torch.Generator().manual_seed(11)
    raws = [torch.randn(s, generator=g).to(dev) for s in ((B, 2, 2, 2), (B, 1, 2, 2), (B, 2, 2), (B, 1, 2, 2))]
    grads = [torch.randn(s, generator=g).to(dev) for s in ((B, 2, 2, 2), (B, 1, 2, 2), (B, 2, 2), (B, 2, 2))]
    out, got = backward_of(hip_lines, raws, grads)
    for part in (slice(0, cut), slice(cut, B)):
        out_p, got_p = backward_of(hip_lines, [t[part].contiguous() for t in raws], [t[part].contiguous() for t in grads])
        assert all(same_bits(a[part], b) for a, b in zip(out, out_p))
        assert all(same_bits(a[part], b) for a, b in zip(got, got_p))
