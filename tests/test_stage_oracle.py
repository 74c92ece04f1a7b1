"""CPU: float64 references and gates for the stage kernels of the reference-compatible API (include/gclm.h):
gclm_residual_fields, gclm_jacobian_fields, gclm_huber_costs, gclm_gradient_hessian, gclm_optimizer_step and
gclm_pack_fields.  tests/test_stage_parity.py holds each HIP kernel to these gates.

Every gate is derived from the float32 arithmetic of the operation it guards, starts at a stated constant and is checked
here in two directions, at the shapes and edges the GPU test uses:
  - an honest float32 evaluation of the same operation (the CPU oracle's float32 build, or the reference's formulas in
    float32) passes it, and
  - a float64 evaluation of a subtly wrong operation (a pixel off by one, another image's camera, a dropped workgroup
    tail, a dropped row, w^2 for w, the eps clamp dropped, the upper triangle read, ...) fails it (gate power).
The measured ratios of the GPU test go to MEASURED."""
import numpy as np
import pytest
import torch

from conftest import MEASURED
from test_step_oracle import NDIST

U = 2.0 ** -24                          # unit roundoff of float32
EPS32 = float(np.finfo(np.float32).eps)  # torch.finfo(torch.float).eps of huber_loss (lm_optimizer.py:82)
MODELS = ("pinhole", "simple_radial", "radial", "simple_divisional")
BLOCK = 256                             # threads per workgroup of the per-pixel kernels

# ------------------------------------------------------------------ residuals and Jacobians

# |r| <= 2 per component: an absolute gate of ~17 float32 ulps of 2 per pixel.
RES_TAU = 2e-6
# Each Jacobian entry against the RMS of its column (image, row kind, parameter) over the image.
JAC_TAU = 4e-5
# simple_divisional's float32 formulas cancel (camera.py:913): its entries add this multiple of the float32-vs-float64
# oracle spread, taken as the largest spread within DIV_WINDOW pixels (the cancellation varies smoothly over the image;
# a single pixel's spread can be zero by luck where a neighbour's is not).  The same named allowance as
# test_step_oracle.div_k_allowance; no other model gets one.
DIV_SPREAD_MULT = 10
DIV_WINDOW = 2

# the sweep's polynomial for sin on [-pi/2, pi/2] (gclm_pass.hip: sin_halfpi), for the "fold dropped" mutation
_SIN_HALFPI = (2.6000457182817627e-06, -0.00019806611817330122, 0.008333017118275166, -0.16666656732559204)


def well_conditioned(cam, grav, H, W):
    """Whether the fields of (cam, grav) are well conditioned over the whole image, so that float32 rounding of the
    inputs is not amplified anywhere: the vanishing point of gravity (where the up field turns around) lies at least
    half an image beyond the image, and the radial distortion r (1 + k1 r^2 + k2 r^4) stays monotonic with a slope of at
    least 0.3 out to the farthest corner (beyond the fold its inverse does not exist)."""
    w, h, fx, fy, cx, cy, k1, k2 = (float(v) for v in cam)
    if abs(grav[2]) > 1e-6:
        vx, vy = cx + fx * grav[0] / grav[2], cy + fy * grav[1] / grav[2]
        dx, dy = max(-vx, vx - (W - 1), 0.0), max(-vy, vy - (H - 1), 0.0)
        if np.hypot(dx, dy) < 0.5 * max(H, W):
            return False
    r2 = max(((x - cx) / fx) ** 2 + ((y - cy) / fy) ** 2 for x in (0, W - 1) for y in (0, H - 1))
    return 1 + 3 * k1 * r2 + 5 * k2 * r2 * r2 >= 0.3


def stage_cameras(model, B, H, W, seed=0):
    """B different cameras (B,8) and unit gravities (B,3), float32: vfov 20..90 deg, fx != fy, the principal point up to a
    quarter of the image off centre, distortion at the ends of the ranges of
    test_gpu_parity.test_jacobian_fields_match_autograd_of_the_forward_model (k1 -0.3 / 0.1, k2 +-0.03), roll and pitch
    within +-45 deg; draws that are not well_conditioned are drawn again."""
    rng = np.random.default_rng([seed, B, H, W, NDIST[model]])
    nd = NDIST[model]
    cams, gravs = np.zeros((B, 8)), np.zeros((B, 3))
    for b in range(B):
        while True:
            vfov = np.radians(rng.uniform(20, 90))
            fy = max(H, 2) / 2 / np.tan(vfov / 2)
            fx = fy * rng.uniform(0.8, 1.25)
            cx, cy = W / 2 + rng.uniform(-0.25, 0.25) * W, H / 2 + rng.uniform(-0.25, 0.25) * H
            k1 = (-0.3, 0.1)[b % 2] if nd else 0.0
            k2 = (0.03, -0.03)[b % 2] if nd == 2 else (k1 if nd == 1 else 0.0)
            cams[b] = [W, H, fx, fy, cx, cy, k1, k2]
            roll, pitch = np.radians(rng.uniform(-45, 45, 2))
            sr, cr, sp, cp = np.sin(roll), np.cos(roll), np.sin(pitch), np.cos(pitch)
            gravs[b] = [-sr * cp, -cr * cp, sp]
            if well_conditioned(cams[b], gravs[b], H, W):
                break
    return cams.astype(np.float32), gravs.astype(np.float32)


def stage_fields(oracle, model, cams, gravs, H, W, seed=0, wild=True):
    """Fields rendered from a slightly different camera (focal +3 %, k1 +0.02, gravity tilted) plus noise, so that every
    residual is non-zero; with `wild`, latitudes beyond +-pi/2 on a regular subset of pixels (k pi added, k = +-1..3, and
    "degrees" up to +-90), which the kernel folds back as torch.sin would."""
    rng = np.random.default_rng([seed, len(cams), H, W])
    true = cams.astype(np.float64).copy()
    true[:, 2:4] *= 1.03
    true[:, 6] += 0.02 * (NDIST[model] > 0)
    tg = gravs.astype(np.float64) + rng.normal(0, 0.03, gravs.shape)
    tg /= np.linalg.norm(tg, axis=1, keepdims=True)
    up, lat = oracle.render(model, H, W, true, tg, precision="f64")
    up = up + rng.normal(0, 0.02, up.shape).astype(np.float32)
    up /= np.sqrt((up.astype(np.float64) ** 2).sum(1, keepdims=True)).astype(np.float32)
    lat = lat + rng.normal(0, 0.02, lat.shape).astype(np.float32)
    if wild:
        flat = lat.reshape(len(cams), -1)
        idx = np.arange(flat.shape[1])
        k = rng.integers(1, 4, flat.shape) * rng.choice([-1, 1], flat.shape)
        flat[:, idx % 7 == 3] += (k * np.pi).astype(np.float32)[:, idx % 7 == 3]
        flat[:, idx % 11 == 5] = rng.uniform(-90, 90, flat[:, idx % 11 == 5].shape).astype(np.float32)
        lat = flat.reshape(lat.shape)
    return {"up_field": np.ascontiguousarray(up, np.float32), "latitude_field": np.ascontiguousarray(lat, np.float32)}


def _window_max(a, axes, r):
    out = a
    for ax in axes:
        n = a.shape[ax]
        cur = out.copy()
        for s in range(1, min(r, n - 1) + 1):
            lo, hi = [slice(None)] * a.ndim, [slice(None)] * a.ndim
            lo[ax], hi[ax] = slice(0, n - s), slice(s, n)
            np.maximum(cur[tuple(lo)], out[tuple(hi)], out=cur[tuple(lo)])
            np.maximum(cur[tuple(hi)], out[tuple(lo)], out=cur[tuple(hi)])
        out = cur
    return out


def ratio(diff, gate):
    """|diff| / gate with 0 / 0 = 0 and a NaN difference = inf."""
    diff = np.abs(np.asarray(diff, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff == 0, 0.0, diff / gate)
    return np.where(np.isnan(r), np.inf, r)


def div_allowance(model, ref32, ref64, H, W):
    """The named simple_divisional allowance: DIV_SPREAD_MULT x the float32-vs-float64 oracle spread, largest within
    DIV_WINDOW pixels; zero for every other model.  Arrays (B, H*W, ...) or (B, H, W, ...)."""
    if model != "simple_divisional":
        return 0.0
    spread = np.abs(np.asarray(ref32, np.float64) - ref64)
    img = spread if spread.ndim == 5 else spread.reshape(spread.shape[0], H, W, spread.shape[-1])
    return DIV_SPREAD_MULT * _window_max(img, (1, 2), DIV_WINDOW).reshape(spread.shape)


def residual_gate(model, got, ref64, ref32, H, W):
    """Per pixel and component: |r - r64| <= RES_TAU (+ the simple_divisional allowance).  Returns the ratio."""
    return ratio(np.asarray(got, np.float64) - ref64, RES_TAU + div_allowance(model, ref32, ref64, H, W))


def jacobian_gate(model, got, ref64, ref32):
    """Per entry of J (B,H,W,R,P): |J - J64| <= JAC_TAU x RMS of that column over the image (+ the allowance)."""
    B, H, W = ref64.shape[:3]
    rms = np.sqrt((ref64 ** 2).mean(axis=(1, 2), keepdims=True))
    return ratio(np.asarray(got, np.float64) - ref64, JAC_TAU * rms + div_allowance(model, ref32, ref64, H, W))


def sin_halfpi64(x):
    x = np.asarray(x, np.float64)
    t = x * x
    p = _SIN_HALFPI[0]
    for c in _SIN_HALFPI[1:]:
        p = p * t + c
    return x * t * p + x


def residual_mutations(oracle, model, data, cams, gravs):
    """float64 residuals of what a subtly wrong kernel would compute: name -> {"up_residual", "latitude_residual"}."""
    H, W = data["latitude_field"].shape[-2:]
    N = H * W
    out = {}
    c = cams.copy()
    c[:, 4] -= 1                                   # pixel x evaluated at x + 1
    out["x_off_by_one"] = oracle.residual_fields(model, data, c, gravs)
    if len(cams) > 1:
        c, g = cams.copy(), gravs.copy()
        c[1], g[1] = c[0], g[0]
        out["image_0_camera_for_image_1"] = oracle.residual_fields(model, data, c, g)
    c = cams.copy()
    c[:, [2, 3]] = c[:, [3, 2]]
    out["fx_fy_swapped"] = oracle.residual_fields(model, data, c, gravs)
    if N % BLOCK:
        r = oracle.residual_fields(model, data, cams, gravs)
        for v in r.values():
            v[:, BLOCK * (N // BLOCK):] = 0
        out["ragged_tail_zeroed"] = r
    lat = data["latitude_field"].reshape(len(cams), N).astype(np.float64)
    beyond = np.abs(lat) > np.pi / 2
    if beyond.any():
        r = oracle.residual_fields(model, data, cams, gravs)
        r["latitude_residual"][..., 0] += np.where(beyond, sin_halfpi64(lat) - np.sin(lat), 0)
        out["latitude_fold_dropped"] = r
    return out


def jacobian_mutations(oracle, model, H, W, cams, gravs, spherical, log_focal):
    """float64 Jacobians of subtly wrong kernels: name -> (J_up, J_lat)."""
    N = H * W
    jac = lambda c, g: oracle.jacobian_fields(model, H, W, c, g, spherical, log_focal, precision="f64")  # noqa: E731
    out = {}
    c = cams.copy()
    c[:, 4] -= 1
    out["x_off_by_one"] = jac(c, gravs)
    if len(cams) > 1:
        c, g = cams.copy(), gravs.copy()
        c[1], g[1] = c[0], g[0]
        out["image_0_camera_for_image_1"] = jac(c, g)
    c = cams.copy()
    c[:, [2, 3]] = c[:, [3, 2]]
    out["fx_fy_swapped"] = jac(c, gravs)
    if N % BLOCK:
        Ju, Jl = jac(cams, gravs)
        for J in (Ju, Jl):
            J.reshape(len(cams), N, *J.shape[3:])[:, BLOCK * (N // BLOCK):] = 0
        out["ragged_tail_zeroed"] = (Ju, Jl)
    if NDIST[model] == 2:
        Ju, Jl = jac(cams, gravs)
        Ju[..., 4] *= 1.001
        Jl[..., 4] *= 1.001
        out["k2_column_scaled_1.001"] = (Ju, Jl)
    return out


# the shapes of tests/test_stage_parity.py (B = 3 images, different cameras)
FIELD_SHAPES = [(1, 1), (7, 5), (16, 16), (17, 16), (33, 47), (480, 640)]


def _per_image(r):
    return r.reshape(r.shape[0], -1).max(1)


def _affected(name, B):
    return [1] if name == "image_0_camera_for_image_1" else list(range(B))


@pytest.mark.parametrize("shape", FIELD_SHAPES)
@pytest.mark.parametrize("model", MODELS)
def test_residual_gate_power(oracle, model, shape):
    """The float32 oracle's residuals pass the residual gate; every mutation fails it on every image it touches."""
    H, W = shape
    cams, gravs = stage_cameras(model, 3, H, W)
    data = stage_fields(oracle, model, cams, gravs, H, W)
    r64 = oracle.residual_fields(model, data, cams, gravs, precision="f64")
    r32 = oracle.residual_fields(model, data, cams, gravs, precision="f32")
    for k in r64:
        hon = residual_gate(model, r32[k], r64[k], r32[k], H, W)
        MEASURED[f"stage_gate/residual/{model}/{H}x{W}/f32_oracle/{k}"] = float(hon.max())
        assert hon.max() <= 0.5, (k, hon.max())
    worst = {}
    for name, m in residual_mutations(oracle, model, data, cams, gravs).items():
        per = np.max([_per_image(residual_gate(model, m[k], r64[k], r32[k], H, W)) for k in r64], 0)
        worst[name] = per
        MEASURED[f"stage_gate_power/residual/{model}/{H}x{W}/{name}"] = per.tolist()
    for name, per in worst.items():
        assert (per[_affected(name, 3)] > 1).all(), (name, per)


@pytest.mark.parametrize("form", ["loop", "rpf"])
@pytest.mark.parametrize("shape", FIELD_SHAPES)
@pytest.mark.parametrize("model", MODELS)
def test_jacobian_gate_power(oracle, model, shape, form):
    """The float32 oracle's Jacobians pass the Jacobian gate (spherical / log-focal form and the rpf form); every
    mutation fails it on every image it touches."""
    H, W = shape
    sph = form == "loop"
    cams, gravs = stage_cameras(model, 3, H, W)
    J64 = oracle.jacobian_fields(model, H, W, cams, gravs, sph, sph, precision="f64")
    J32 = oracle.jacobian_fields(model, H, W, cams, gravs, sph, sph, precision="f32")
    for i, k in enumerate(("J_up", "J_lat")):
        hon = jacobian_gate(model, J32[i], J64[i], J32[i])
        MEASURED[f"stage_gate/jacobian/{model}/{form}/{H}x{W}/f32_oracle/{k}"] = float(hon.max())
        assert hon.max() <= 0.5, (k, hon.max())
    for name, (mu, ml) in jacobian_mutations(oracle, model, H, W, cams, gravs, sph, sph).items():
        per = np.maximum(_per_image(jacobian_gate(model, mu, J64[0], J32[0])),
                         _per_image(jacobian_gate(model, ml, J64[1], J32[1])))
        MEASURED[f"stage_gate_power/jacobian/{model}/{form}/{H}x{W}/{name}"] = per.tolist()
        assert (per[_affected(name, 3)] > 1).all(), (name, per)


# ------------------------------------------------------------------ Huber

# Relative to the float64 value: the squared norm (dim fmas), y = x2 * (1 / a^2), the rsq (1 ulp) and up to three
# products / one quotient after it: < 8 roundings of 2^-24.  Values below FLT_MIN are free: float32 cannot hold them to a
# relative precision (d2 = -eps / 2x at x = 3e38 is 2e-46 in float64, -0 in float32).
HUBER_TAU = 8 * U
FLT_MIN = float(np.finfo(np.float32).tiny)
HUBER_BRANCH_ULPS = 4                   # within 4 float32 ulps of y = 1 either branch is accepted (d2 jumps there)


def huber_ref(x2, a, conf=None, floor=True, conf_in_d2=False, branch=None):
    """scaled_loss(x2, huber_loss, a) (lm_optimizer.py:61-87) in float64, times the confidence as calculate_costs does
    (:293-298): (cost, d1 = weight, d2).  `floor` keeps the eps floor of isx; `branch` forces y <= 1 (True) / > 1."""
    x2 = np.asarray(x2, np.float64)
    a2 = float(a) ** 2
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        y = x2 / a2
        mask = (y <= 1) if branch is None else np.full(y.shape, branch)
        sx = np.sqrt(y + 1e-8)
        isx = np.maximum(EPS32, 1 / sx) if floor else 1 / sx
        cost = np.where(mask, y, 2 * sx - 1) * a2
        d1 = np.where(mask, 1.0, isx)
        d2 = np.where(mask, 0.0, -isx / (2 * y)) / a2
        if conf is not None:
            c = np.asarray(conf, np.float64)
            cost, d1 = cost * c, d1 * c
            if conf_in_d2:
                d2 = d2 * c
    return cost, d1, d2


def huber_f32(x2, a, conf=None):
    """The reference's own float32 arithmetic (torch float32 on the CPU: one rounding per operation), as numpy."""
    f = np.float32
    x2 = np.asarray(x2, f)
    a2 = f(float(a) ** 2)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        y = x2 / a2
        mask = y <= 1
        sx = np.sqrt(y + f(1e-8))
        isx = np.maximum(f(EPS32), f(1) / sx)
        cost = np.where(mask, y, f(2) * sx - f(1)) * a2
        d1 = np.where(mask, f(1), isx)
        d2 = np.where(mask, f(0), -isx / (f(2) * y)) / a2
        if conf is not None:
            cost, d1 = cost * np.asarray(conf, f), d1 * np.asarray(conf, f)
    return cost, d1, d2


def x2_of(rows, dim):
    """|r|^2 in float64 of the float32-stored residual rows (dim = 0: the inputs are |r|^2)."""
    r = np.asarray(rows, np.float32).astype(np.float64)
    return r if dim == 0 else (r.reshape(-1, dim) ** 2).sum(1)


def _huber_one(got, ref):
    got = np.asarray(got, np.float64)
    exact = (got == ref) | (np.isnan(got) & np.isnan(ref))
    r = ratio(got - ref, HUBER_TAU * np.abs(ref) + FLT_MIN)
    return np.where(exact, 0.0, np.where(np.isfinite(ref), r, np.inf))


def huber_gate(got, x2, a, conf=None, **kw):
    """Ratios (cost, d1, d2) of got to the float64 reference, relative, HUBER_TAU; exact agreement where the reference is
    not finite; within HUBER_BRANCH_ULPS of y = 1 the better of the two branches."""
    out = [_huber_one(g, r) for g, r in zip(got, huber_ref(x2, a, conf, **kw))]
    y = np.asarray(x2, np.float64) / float(a) ** 2
    near = np.abs(y - 1) <= HUBER_BRANCH_ULPS * EPS32
    if near.any():
        for branch in (True, False):
            alt = [_huber_one(g, r) for g, r in zip(got, huber_ref(x2, a, conf, branch=branch, **kw))]
            worst_alt = np.maximum.reduce(alt)
            worst = np.maximum.reduce(out)
            take = near & (worst_alt < worst)
            out = [np.where(take, b, o) for o, b in zip(out, alt)]
    return out


def huber_inputs(n, dim, a, seed=0):
    """n residual rows of `dim` components (dim 0: |r|^2 directly): the edges first -- 0, exactly a^2, one ulp either side,
    1e13, 1e14, 1e20, +inf (as |r|^2 for dim 0; as a row (sqrt(v), 0, ...) otherwise) -- then magnitudes spread over
    1e-8 ... 1e8 around a^2, cut at n."""
    rng = np.random.default_rng([seed, n, dim])
    a2 = np.float32(np.float32(a) * np.float32(a))
    edges = np.array([0.0, a2, np.nextafter(a2, np.float32(0)), np.nextafter(a2, np.float32(np.inf)), 1e13, 1e14, 1e20,
                      np.inf], np.float32)
    k = max(n, len(edges))
    mag = (np.float64(a2) * 10.0 ** rng.uniform(-8, 8, k)).astype(np.float32)
    mag[:len(edges)] = edges
    mag = mag[:n]
    if dim == 0:
        return mag
    r = rng.normal(0, 1, (n, dim)).astype(np.float32)
    r /= np.sqrt((r.astype(np.float64) ** 2).sum(1, keepdims=True)).astype(np.float32)
    r *= np.sqrt(mag.astype(np.float64)).astype(np.float32)[:, None]
    ne = min(n, len(edges))
    r[:ne] = 0
    r[:ne, 0] = np.sqrt(edges[:ne].astype(np.float64)).astype(np.float32)
    return r.reshape(-1)


@pytest.mark.parametrize("dim", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("a", [1.0, 1e-2, 3.0])
def test_huber_gate_power(dim, a):
    """The reference's own float32 arithmetic passes the Huber gate (both derivatives, with and without a confidence);
    the eps floor dropped and the confidence applied to d2 each fail it."""
    n = 4099
    rows = huber_inputs(n, dim, a)
    x2 = x2_of(rows, dim)
    conf = np.random.default_rng(1).uniform(0.05, 1, n).astype(np.float32)
    for c in (None, conf):
        got = huber_f32(x2.astype(np.float32) if dim == 0 else x2, a, c)
        r = huber_gate(got, x2, a, c)
        MEASURED[f"stage_gate/huber/dim{dim}/a{a}/conf{c is not None}/f32_reference"] = [float(v.max()) for v in r]
        assert max(v.max() for v in r) <= 1, [v.max() for v in r]
    ref = huber_ref(x2, a, conf)
    nofloor = huber_ref(x2, a, conf, floor=False)
    big = x2 / a ** 2 > 1 / EPS32 ** 2
    assert big.sum() >= 2
    assert max(v[big].max() for v in huber_gate(nofloor, x2, a, conf)) > 1
    in_d2 = huber_ref(x2, a, conf, conf_in_d2=True)
    assert huber_gate(in_d2, x2, a, conf)[2].max() > 1
    # the edge values themselves: +inf gives (inf, eps, -0) scaled, as torch does
    i = int(np.argmax(np.isinf(x2)))
    assert ref[0][i] == np.inf and ref[1][i] == EPS32 * np.float64(conf[i]) and ref[2][i] == 0 and np.signbit(ref[2][i])


# ------------------------------------------------------------------ J^T W J, J^T W r

# Each term carries at most two float32 roundings (w J_k, then * r or * J_l), the sum is taken in double and rounded to
# float32 once: |H_kl - H64_kl| <= TAU sqrt(Hh_kk Hh_ll), Hh = sum |w| J^2 (Cauchy-Schwarz), TAU = 3 U + the double sum.
CONTRACT_TAU = 4 * U


def contraction_ref(J, r, w, G0=None, H0=None):
    """G = sum w J^T r, H = sum w J^T J in float64 on the float32 inputs J (B,N,R,P), r (B,N,R), w (B,N); plus the
    prefill (accumulate)."""
    J = np.asarray(J, np.float32).astype(np.float64)
    B, N, R, P = J.shape
    Jw = J * np.asarray(w, np.float32).astype(np.float64)[:, :, None, None]
    Jf, Jwf = J.reshape(B, N * R, P), Jw.reshape(B, N * R, P)
    H = np.matmul(Jwf.transpose(0, 2, 1), Jf)
    G = np.einsum("bkp,bk->bp", Jwf, np.asarray(r, np.float32).astype(np.float64).reshape(B, N * R))
    if G0 is not None:
        G, H = G + G0, H + H0
    return G, H


def contraction_f32(J, r, w):
    """The kernel's own arithmetic: float32 products w J_k, then * r / * J_l, summed in double, rounded to float32."""
    J = np.asarray(J, np.float32)
    B, N, R, P = J.shape
    wJ = (J * np.asarray(w, np.float32)[:, :, None, None]).astype(np.float32)
    G = (wJ * np.asarray(r, np.float32).reshape(B, N, R)[..., None]).astype(np.float64).sum((1, 2))
    H = np.zeros((B, P, P))
    for k in range(P):
        H[:, k] = (wJ[..., k:k + 1] * J).astype(np.float64).sum((1, 2))
    return G.astype(np.float32), H.astype(np.float32)


def contraction_bounds(J, r, w):
    """The contraction's own part of the gate: CONTRACT_TAU sqrt(Hh_k rr) for G (B,P), CONTRACT_TAU sqrt(Hh_k Hh_l) for
    H (B,P,P)."""
    J = np.asarray(J, np.float32).astype(np.float64)
    aw = np.abs(np.asarray(w, np.float32).astype(np.float64))
    B, N, R, P = J.shape
    Hh = np.einsum("bn,bnrp->bp", aw, J * J)
    rr = np.einsum("bn,bnr->b", aw, np.asarray(r, np.float32).astype(np.float64).reshape(B, N, R) ** 2)
    return CONTRACT_TAU * np.sqrt(Hh * rr[:, None]), CONTRACT_TAU * np.sqrt(Hh[:, :, None] * Hh[:, None, :])


def contraction_gate(G, H, J, r, w, G64, H64, G0=None, H0=None, adds=0):
    """Ratios (B,P), (B,P,P) per entry.  Each float32 addition after the contraction (the prefill of accumulate, or
    `adds` more, e.g. setup_system's up + latitude) adds U (|addend| + |result|)."""
    gG, gH = contraction_bounds(J, r, w)
    if G0 is not None:
        gG = gG + U * (np.abs(G0) + np.abs(G64))
        gH = gH + U * (np.abs(H0) + np.abs(H64))
    gG, gH = gG + adds * U * np.abs(G64), gH + adds * U * np.abs(H64)
    return ratio(np.asarray(G, np.float64) - G64, gG), ratio(np.asarray(H, np.float64) - H64, gH)


def contraction_inputs(B, N, R, P, seed=0, zero_image=None):
    """J ~ N(0,1) with columns of different scale, r ~ N(0, 0.1), w ~ U(0, 1) with every 5th weight exactly 0 (from
    pixel 2 on: the first and last pixels of every tested N keep theirs) and
    image `zero_image` all zero."""
    rng = np.random.default_rng([seed, B, N, R, P])
    J = (rng.normal(0, 1, (B, N, R, P)) * 10.0 ** rng.uniform(-2, 2, P)).astype(np.float32)
    r = rng.normal(0, 0.1, (B, N, R)).astype(np.float32)
    w = rng.uniform(0, 1, (B, N)).astype(np.float32)
    w[:, 2::5] = 0
    if zero_image is not None and zero_image < B:
        w[zero_image] = 0
    return J, r, w


def contraction_mutations(J, r, w, G0, H0):
    """float64 (G, H) of subtly wrong contractions (name -> (G, H)); with a prefill G0 / H0 (accumulate)."""
    B, N, R, P = J.shape
    out = {}
    out["last_pixel_dropped"] = contraction_ref(J[:, :-1], r[:, :-1], w[:, :-1], G0, H0)
    if R > 1:
        out["last_row_dropped"] = contraction_ref(J[:, :, :-1], r[:, :, :-1], w, G0, H0)
    out["w_squared"] = contraction_ref(J, r, w.astype(np.float64) ** 2, G0, H0)
    if P > 1:
        Js = J.copy()
        Js[..., [0, P - 1]] = Js[..., [P - 1, 0]]
        out["columns_swapped"] = contraction_ref(Js, r, w, G0, H0)
    if N % BLOCK and N > BLOCK:
        n0 = BLOCK * (N // BLOCK)
        out["pixels_past_last_256_dropped"] = contraction_ref(J[:, :n0], r[:, :n0], w[:, :n0], G0, H0)
    out["prefill_ignored"] = contraction_ref(J, r, w)
    return out


def symmetric_prefill(B, P, seed=0):
    rng = np.random.default_rng([seed, B, P, 7])
    M = rng.normal(0, 10, (B, P, P)).astype(np.float32)
    return rng.normal(0, 10, (B, P)).astype(np.float32), ((M + M.transpose(0, 2, 1)) / 2).astype(np.float32)


@pytest.mark.parametrize("N", [1, 255, 257, 307200 + 77])
@pytest.mark.parametrize("R", [1, 2, 3, 4])
def test_contraction_gate_power(N, R):
    """The kernel's own float32 arithmetic passes the per-entry contraction gate, with and without a prefill; every
    mutation fails it on every image (except the image whose weights are all zero, for those that scale w)."""
    P = 5
    B = 3 if N < 1000 else 1
    J, r, w = contraction_inputs(B, N, R, P)
    G0, H0 = symmetric_prefill(B, P)
    G64, H64 = contraction_ref(J, r, w)
    G32, H32 = contraction_f32(J, r, w)
    rg, rh = contraction_gate(G32, H32, J, r, w, G64, H64)
    MEASURED[f"stage_gate/contraction/N{N}/R{R}/kernel_arith"] = [float(rg.max()), float(rh.max())]
    assert max(rg.max(), rh.max()) <= 0.5
    Ga, Ha = contraction_ref(J, r, w, G0, H0)
    Gs, Hs = (G0 + G32).astype(np.float32), (H0 + H32).astype(np.float32)
    rg, rh = contraction_gate(Gs, Hs, J, r, w, Ga, Ha, G0, H0)
    assert max(rg.max(), rh.max()) <= 0.5
    for name, (Gm, Hm) in contraction_mutations(J, r, w, G0, H0).items():
        if name == "last_pixel_dropped" and N == 1:
            continue                      # that is the prefill alone: covered by prefill_ignored's converse
        rg, rh = contraction_gate(Gm, Hm, J, r, w, Ga, Ha, G0, H0)
        per = np.maximum(rg.max(1), rh.max((1, 2)))
        MEASURED[f"stage_gate_power/contraction/N{N}/R{R}/{name}"] = per.tolist()
        assert (per > 1).all(), (name, per)


# ------------------------------------------------------------------ damped step

# With D = diag(A)^1/2 and kappa the condition number of D^-1 A D^-1: ||D (delta - delta64)||_inf <= TAU kappa ||D delta64||_inf
# (the float32 rounding of the damped diagonal and a float32 Cholesky of a P <= 5 system).
STEP_TAU = 16 * U


def damped_matrix(H, lam, eps, upper=False, clamp=True, lam_identity=False):
    """H + diag(clamp(lambda diag H, eps)) in float64 from ONE triangle of H (the lower one, as torch.linalg.cholesky
    reads it)."""
    H = np.asarray(H, np.float32).astype(np.float64)
    T = np.triu(H) if upper else np.tril(H)
    A = T + np.swapaxes(np.triu(T, 1) if upper else np.tril(T, -1), -1, -2)
    d = np.diagonal(H, axis1=-2, axis2=-1)
    lam = np.broadcast_to(np.asarray(lam, np.float32).astype(np.float64).reshape(-1, 1), d.shape)
    add = lam if lam_identity else lam * d
    if clamp:
        add = np.where(np.isnan(add), add, np.maximum(add, eps))
    return A + add[..., None] * np.eye(H.shape[-1])


def chol_solve64(A, G):
    """Batched float64 Cholesky solve reading the lower triangle of A: (delta, failed); a pivot <= 0 or NaN fails the
    system with delta = 0."""
    A = np.asarray(A, np.float64)
    g = np.asarray(G, np.float32).astype(np.float64).copy()
    B, P = g.shape
    L = np.zeros_like(A)
    ok = np.ones(B, bool)
    for j in range(P):
        s = A[:, j, j] - (L[:, j, :j] ** 2).sum(1)
        ok &= s > 0
        l = np.sqrt(np.where(s > 0, s, 1.0))
        L[:, j, j] = l
        for i in range(j + 1, P):
            L[:, i, j] = (A[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(1)) / l
    for i in range(P):
        g[:, i] = (g[:, i] - (L[:, i, :i] * g[:, :i]).sum(1)) / L[:, i, i]
    for i in range(P - 1, -1, -1):
        g[:, i] = (g[:, i] - (L[:, i + 1:, i] * g[:, i + 1:]).sum(1)) / L[:, i, i]
    g[~ok] = 0
    return g, (~ok).astype(np.int32)


def step_ref(G, H, lam, eps=1e-6, **kw):
    A = damped_matrix(H, lam, eps, **kw)
    d, f = chol_solve64(A, G)
    return d, f, A


def step_f32(G, H, lam, eps=1e-6):
    """optimizer_step of the reference (lm_optimizer.py:109-137) in float32 torch on the CPU, per system (a failure
    zeroes that system only, as the HIP kernel does): (delta, failed)."""
    Ht, Gt = torch.from_numpy(np.asarray(H, np.float32)), torch.from_numpy(np.asarray(G, np.float32))
    lt = torch.as_tensor(np.asarray(lam, np.float32)).reshape(-1)
    diag = Ht.diagonal(dim1=-2, dim2=-1) * (lt[:, None] if lt.numel() > 1 else lt)
    A = Ht + diag.clamp(min=eps).diag_embed()
    U_, info = torch.linalg.cholesky_ex(A)
    bad = info != 0
    delta = torch.cholesky_solve(Gt[..., None], torch.where(bad[:, None, None], torch.eye(A.shape[-1]), U_))[..., 0]
    delta[bad] = 0
    return delta.numpy(), bad.numpy().astype(np.int32)


def step_gate(delta, failed, d64, f64, A64):
    """Per system: the ratio of ||D (delta - delta64)||_inf to STEP_TAU kappa ||D delta64||_inf; inf where the failure
    flags differ, where a failed system's delta is not exactly 0, or where NaNs of the float64 step are not NaN."""
    delta, d64 = np.asarray(delta, np.float64), np.asarray(d64, np.float64)
    B, P = d64.shape
    out = np.zeros(B)
    good = (np.asarray(failed) == 0) & (f64 == 0)
    nan64 = np.isnan(d64).any(1)
    fin = good & ~nan64
    if fin.any():
        A = A64[fin]
        D = np.sqrt(np.diagonal(A, axis1=-2, axis2=-1))
        S = A / (D[:, :, None] * D[:, None, :])
        ev = np.linalg.eigvalsh(S)
        kappa = ev[:, -1] / ev[:, 0]
        err = np.abs(D * (delta[fin] - d64[fin])).max(1)
        out[fin] = ratio(err, STEP_TAU * kappa * np.abs(D * d64[fin]).max(1))
    out[np.asarray(failed) != f64] = np.inf
    out[(f64 == 1) & (np.abs(delta).max(1) != 0)] = np.inf
    out[good & nan64 & (np.isnan(delta) != np.isnan(d64)).any(1)] = np.inf
    return out


def spd_systems(B, P, kappa, seed=0, scale_range=(-3, 3)):
    """B SPD matrices D S D, S with unit diagonal and condition number ~kappa, D = 10^U(scale_range); gradients N(0,1)
    scaled by D."""
    rng = np.random.default_rng([seed, B, P, int(np.log10(kappa) * 10)])
    Q, _ = np.linalg.qr(rng.normal(size=(B, P, P)))
    ev = np.exp(np.linspace(0, np.log(kappa), P))[None] * np.ones((B, 1))
    S = Q @ (ev[:, :, None] * np.swapaxes(Q, -1, -2))
    d = np.sqrt(np.diagonal(S, axis1=-2, axis2=-1))
    S = S / (d[:, :, None] * d[:, None, :])
    D = 10.0 ** rng.uniform(*scale_range, (B, P))
    H = (D[:, :, None] * S * D[:, None, :]).astype(np.float32)
    H = ((H + np.swapaxes(H, -1, -2)) / 2).astype(np.float32)
    G = (rng.normal(0, 1, (B, P)) * D).astype(np.float32)
    return G, H


def step_families(P, B=64, seed=0):
    """name -> (G, H, lambda, eps) of the GPU test's families."""
    rng = np.random.default_rng([seed, P])
    fam = {}
    G, H = spd_systems(B, P, 10.0, seed)
    fam["scaled_spd"] = (G, H, np.float32(0.1), 1e-6)
    fam["per_image_lambda"] = (G, H, rng.uniform(0, 10, B).astype(np.float32), 1e-6)
    lam = rng.uniform(0, 1, B).astype(np.float32)
    lam[::3] = 0
    fam["per_image_lambda_with_zeros"] = (G, H, lam, 1e-6)
    J = rng.normal(0, 0.01, (B, P + 2, P))
    J[:, :, -1] = J[:, :, 0]                 # rank P - 1: PSD, singular; eps alone makes it definite (kappa ~ 1e3)
    Hs = np.einsum("bnp,bnq->bpq", J, J).astype(np.float32)
    fam["rank_deficient_lambda_0"] = (rng.normal(0, 1, (B, P)).astype(np.float32), Hs, np.float32(0.0), 1e-6)
    G2, H2 = spd_systems(B, P, 10.0, seed + 1, scale_range=(-5, -4))
    fam["lambda_diag_below_eps"] = (G2, (H2 * np.float32(1e-3)).astype(np.float32), np.float32(0.1), 1e-6)
    for k in range(1, 7):
        Gk, Hk = spd_systems(B, P, 10.0 ** k, seed + 10 + k, scale_range=(-2, 2))
        fam[f"kappa_1e{k}"] = (Gk, Hk, np.float32(0.0), 1e-6)
    Ga, Ha = spd_systems(B, P, 10.0, seed + 2)
    Ha = Ha.copy()
    iu = np.triu_indices(P, 1)
    Ha[:, iu[0], iu[1]] = rng.normal(0, 100, (B, len(iu[0]))).astype(np.float32)   # the upper triangle is garbage
    fam["upper_triangle_garbage"] = (Ga, Ha, np.float32(0.1), 1e-6)
    fam["eps_1e-3"] = (G, H, np.float32(0.01), 1e-3)
    return fam


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5])
def test_step_gate_power(P):
    """The reference's float32 step (torch on the CPU) passes the step gate on every family; the eps clamp dropped,
    lambda I for lambda diag H and the upper triangle read each fail it on every system of the family that exposes it."""
    fam = step_families(P)
    for name, (G, H, lam, eps) in fam.items():
        d64, f64, A = step_ref(G, H, lam, eps)
        d32, f32 = step_f32(G, H, lam, eps)
        r = step_gate(d32, f32, d64, f64, A)
        MEASURED[f"stage_gate/step/P{P}/{name}/f32_reference"] = float(r.max())
        assert (f64 == 0).all() and r.max() <= 0.5, (name, r.max())
    checks = [("eps_clamp_dropped", "lambda_diag_below_eps", {"clamp": False}),
              ("lambda_identity", "scaled_spd", {"lam_identity": True})]
    if P > 1:
        checks.append(("upper_triangle_read", "upper_triangle_garbage", {"upper": True}))
    for mut, fname, kw in checks:
        G, H, lam, eps = fam[fname]
        d64, f64, A = step_ref(G, H, lam, eps)
        dm, fm, _ = step_ref(G, H, lam, eps, **kw)
        r = step_gate(dm, fm, d64, f64, A)
        MEASURED[f"stage_gate_power/step/P{P}/{mut}"] = float(r.min())
        assert (r > 1).all(), (mut, r.min())


def test_step_reference_edges():
    """The float64 step's own rules: NaN in the lower triangle fails with delta = 0, NaN only in the upper triangle is
    not read, NaN in G with a PD H gives a NaN delta and no failure (as torch.cholesky_solve does), all-zero H is eps I."""
    G, H = spd_systems(4, 3, 10.0, 5)
    Hn = H.copy()
    Hn[0, 2, 0] = np.nan
    Hn[1, 0, 2] = np.nan
    Hn[2, 1, 1] = np.nan
    Gn = G.copy()
    Gn[3, 1] = np.nan
    d, f, _ = step_ref(Gn, Hn, np.float32(0.1))
    assert f.tolist() == [1, 0, 1, 0] and (d[[0, 2]] == 0).all()
    assert np.array_equal(d[1], step_ref(G, H, np.float32(0.1))[0][1])
    assert np.isnan(d[3]).all()
    d32, f32 = step_f32(Gn, Hn, np.float32(0.1))
    assert f32.tolist() == [1, 0, 1, 0] and np.isnan(d32[3]).all()
    dz, fz, _ = step_ref(G, np.zeros_like(H), np.float32(0.1))
    assert (fz == 0).all() and np.allclose(dz, G / 1e-6)


# ------------------------------------------------------------------ CNN head epilogue

# Few float32 ulps: F.normalize (the squares, the sum, sqrt, one quotient), tanh and asin (plus the condition number of
# asin at the clamped argument), sigmoid (exp, one sum, one quotient).  Confidences below FLT_MIN are free.
HEAD_TAU = 8 * U
LAT_CLAMP = float(np.float32(1 - 1e-5))    # torch.clamp of a float32 tensor by the python float 1 - 1e-5


def head_ref(up_raw, lat_raw, ulc=None, llc=None, clamp=True, norm_eps=True, sigmoid_sign=1):
    """The head epilogues (geocalib.py:57,73-75) in float64: (up, latitude, up_conf, lat_conf, clamped tanh)."""
    u = np.asarray(up_raw, np.float32).astype(np.float64)
    n = np.sqrt((u ** 2).sum(1, keepdims=True))
    with np.errstate(divide="ignore", invalid="ignore"):
        up = u / (np.maximum(n, 1e-12) if norm_eps else n)
    t = np.tanh(np.asarray(lat_raw, np.float32).astype(np.float64))
    if clamp:
        t = np.clip(t, -LAT_CLAMP, LAT_CLAMP)
    lat = np.arcsin(t)

    def sig(x):                     # (B,H,W), as pack_fields returns the confidences
        if x is None:
            return None
        x = sigmoid_sign * np.asarray(x, np.float32).astype(np.float64)
        return np.exp(-np.logaddexp(0.0, -x)).reshape(lat.shape[0], *lat.shape[2:])
    return up, lat, sig(ulc), sig(llc), t


def head_gate(got, ref):
    """Ratios of (up, latitude, up_conf, lat_conf): up absolute (unit vectors), latitude HEAD_TAU (|lat| + |t| /
    sqrt(1 - t^2)) (asin's condition number at the clamped tanh t), confidences relative plus FLT_MIN."""
    up, lat, uc, lc, t = ref
    out = [ratio(np.asarray(got[0], np.float64) - up, HEAD_TAU),
           ratio(np.asarray(got[1], np.float64) - lat, HEAD_TAU * (np.abs(lat) + np.abs(t) / np.sqrt(1 - t * t)))]
    for g, c in ((got[2], uc), (got[3], lc)):
        if c is not None:
            assert np.shape(g) == c.shape, (np.shape(g), c.shape)
            out.append(ratio(np.asarray(g, np.float64) - c, HEAD_TAU * np.abs(c) + FLT_MIN))
    return out


def head_inputs(B, H, W, seed=0):
    """Raw head outputs with the edges on a regular subset of pixels: raw latitude +-30 (tanh saturates, the clamp
    acts), up vectors of norm < 1e-12 and of norm 1e18, logits +-100; N(0, 3) elsewhere."""
    rng = np.random.default_rng([seed, B, H, W])
    up = (rng.normal(0, 3, (B, 2, H, W))).astype(np.float32)
    lat = (rng.normal(0, 2, (B, 1, H, W))).astype(np.float32)
    ulc = rng.normal(0, 4, (B, H, W)).astype(np.float32)
    llc = rng.normal(0, 4, (B, 1, H, W)).astype(np.float32)
    fu, fl = up.reshape(B, 2, -1), lat.reshape(B, -1)
    fuc, flc = ulc.reshape(B, -1), llc.reshape(B, -1)
    idx = np.arange(H * W)
    fl[:, idx % 5 == 1] = 30
    fl[:, idx % 5 == 2] = -30
    fu[:, :, idx % 9 == 4] *= np.float32(1e-13)
    fu[:, :, idx % 9 == 5] *= np.float32(1e18 / 3)
    fu[:, :, idx % 97 == 6] = 0
    fuc[:, idx % 6 == 1], flc[:, idx % 6 == 2] = 100, -100
    fuc[:, idx % 6 == 3], flc[:, idx % 6 == 4] = -100, 100
    return up, lat, ulc, llc


def head_f32(up_raw, lat_raw, ulc, llc):
    """The reference's float32 expression (torch on the CPU)."""
    F = torch.nn.functional
    up = F.normalize(torch.from_numpy(up_raw), dim=1)
    lat = torch.asin(torch.clamp(torch.tanh(torch.from_numpy(lat_raw)), -1 + 1e-5, 1 - 1e-5))
    return (up.numpy(), lat.numpy(), torch.sigmoid(torch.from_numpy(ulc)).numpy(),
            torch.sigmoid(torch.from_numpy(llc)).numpy().reshape(ulc.shape))


def test_head_gate_power():
    """torch's float32 head epilogue passes the head gate; the clamp dropped, F.normalize's eps dropped and a sigmoid of
    the wrong sign each fail it."""
    up_raw, lat_raw, ulc, llc = head_inputs(2, 33, 47)
    ref = head_ref(up_raw, lat_raw, ulc, llc)
    r = head_gate(head_f32(up_raw, lat_raw, ulc, llc), ref)
    MEASURED["stage_gate/head/f32_torch"] = [float(v.max()) for v in r]
    assert max(v.max() for v in r) <= 0.5, [v.max() for v in r]
    assert np.float32(1 - 1e-5) == np.float32(1) - np.float32(1e-5)      # the kernel's constant is torch's clamp bound
    for kw, which in (({"clamp": False}, 1), ({"norm_eps": False}, 0), ({"sigmoid_sign": -1}, 2)):
        m = head_ref(up_raw, lat_raw, ulc, llc, **kw)
        got = (m[0], m[1], m[2], m[3])
        assert head_gate(got, ref)[which].max() > 1, kw
