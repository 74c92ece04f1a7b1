"""Float64 yardstick and per-pixel gate of the perspective fields (gclm_perspective_fields), shared by the CPU self-check
(test_perspective_abi.py) and the GPU parity test (test_perspective_fields.py).

Yardstick: the formulas of include/gclm.h in float64, from the float32 camera and the gravity as stored, simple_divisional's
s and s' in the forms that do not cancel, the latitude clamped at the float32 bound torch clamps at.  The kernel's float32
result differs from it by rounding, bounded per pixel:
  - q (the unnormalised up vector): delta_q, a first-order bound on the float32 rounding of q built from the magnitudes of
    its terms (and the conditioning of sqrt(tau) for simple_divisional, which grows at the singular circle 4 k1 r2 = 1);
  - sin(latitude) before the clamp: delta_s, the same for (u t a + v t b + c) / |(u t, v t, 1)|.
Both are scaled by kappa, DERIVED per case as 4 x the worst ratio of a float32 restatement of the kernel's formulas against
float64 at that case's cameras (at least 1).  Gates per pixel:
    up (normalised):   |up - up64|  <= kappa delta_q / |q| + 2 ulp(1)    (1/|q|: the direction's conditioning, which grows
                                                                          at the vanishing point of gravity in the image)
    up (normalize=False): |q - q64| <= kappa delta_q                     (per component)
    latitude:          |lat - lat64| <= max over s in [s64 - kappa delta_s, s64 + kappa delta_s] of
                                        |asin(clamp(s)) - lat64| + 2 ulp(lat64)
The latitude bound is kappa delta_s / sqrt(1 - s^2) away from the clamp and accepts either side of the clamp within
delta_s of its bound."""
import math

import torch

from undistort_gate import MODELS, make_cameras  # noqa: F401  (one camera generator for the image tests)

U = 2.0 ** -24
LAT_HI32 = float(torch.tensor(1 - 1e-6, dtype=torch.float32))     # torch clamps a float32 tensor at the float32 bound
LAT_HI64 = 1 - 1e-6                                               # ... and a float64 tensor at the float64 one


def make_gravity(n, kind="random", seed=0):
    """(n, 3) float32 gravities (roll, pitch as Gravity.from_rp, rounded to float32 as stored):
    random: |roll|, |pitch| <= 1.2;  pitch+ / pitch-: pitch +-1.5 (the vanishing point of gravity inside the image),
    roll+ / roll-: roll +-(pi/2 - 0.02)."""
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64)  # noqa: E731
    roll, pitch = u(-1.2, 1.2), u(-1.2, 1.2)
    if kind in ("pitch+", "pitch-"):
        pitch = torch.full((n,), 1.5 if kind == "pitch+" else -1.5, dtype=torch.float64) + u(-0.02, 0.02)
    elif kind in ("roll+", "roll-"):
        roll = torch.full((n,), math.pi / 2 - 0.02, dtype=torch.float64) * (1 if kind == "roll+" else -1) + u(-0.01, 0.01)
    h = -torch.cos(pitch)
    return torch.stack([torch.sin(roll) * h, torch.cos(roll) * h, torch.sin(pitch)], -1).to(torch.float32)


def scales(model, k1, k2, r2, cancelling=False):
    """(s, s', t) of camera.py's _distort_scale, _distort_scale_dr2, _undistort_scale in r2's dtype.  simple_divisional:
    the non-cancelling forms (include/gclm.h), or with `cancelling` the reference's own expressions."""
    one = torch.ones_like(r2)
    if model == "pinhole":
        return one, torch.zeros_like(r2), one
    if model == "simple_radial":
        return 1 + k1 * r2, k1 * one, 1 - k1 * r2
    if model == "radial":
        return 1 + k1 * r2 + k2 * r2 ** 2, k1 + 2 * k2 * r2, 1 - k1 * r2 + (3 * k1 ** 2 - k2) * r2 ** 2
    kr = k1 * r2
    den_t = 1 + kr
    t = 1 / torch.where(den_t == 0, 1e6 * one, den_t)
    tau = 1 - 4 * kr
    tt = torch.sqrt(torch.tensor(1e-6, dtype=r2.dtype)).to(r2.device)
    den = 2 * k1 * r2 ** 2 * tt
    sp_clamped = (2 * kr - (1 - tt) * tt) / torch.where(den == 0, 1e6 * one, den)
    if cancelling:
        num = 1 - torch.sqrt(tau.clamp(min=0))
        s = torch.where(kr == 0, one, num / torch.where(kr == 0, 1e6 * one, 2 * kr))
        rt = torch.sqrt(tau.clamp(min=1e-6))
        den = 2 * k1 * r2 ** 2 * rt
        sp = (2 * kr - (1 - rt) * rt) / torch.where(den == 0, 1e6 * one, den)
        return s, sp, t
    rt = torch.sqrt(tau.clamp(min=0))
    d = 1 + rt
    s = torch.where(tau > 0, 2 / d, 1 / torch.where(kr == 0, one, 2 * kr))
    sp = torch.where(tau >= torch.tensor(1e-6, dtype=r2.dtype), 4 * k1 / torch.where(rt == 0, one, rt * d * d), sp_clamped)
    return torch.where(kr == 0, one, s), torch.where(kr == 0, 0 * one, sp), t


def _error_of_scales(model, k1, k2, r2, s, sp, t):
    """First-order float32 error bounds (ds, ds', dt) of s, s', t, with r2 carrying ~4 U of relative error."""
    z = torch.zeros_like(r2)
    if model == "pinhole":
        return z, z, z
    kr = (k1 * r2).abs()
    if model == "simple_radial":
        return U * (s.abs() + 5 * kr), z, U * (t.abs() + 5 * kr)
    if model == "radial":
        q = r2 ** 2
        return (U * (s.abs() + 5 * kr + 9 * k2.abs() * q), U * (sp.abs() + 10 * k2.abs() * r2),
                U * (t.abs() + 5 * kr + 10 * (3 * k1 ** 2 + k2.abs()) * q))
    tau = 1 - 4 * k1 * r2
    rt = torch.sqrt(tau.clamp(min=0))
    dtau = U * (1 + 12 * kr)
    drt = torch.minimum(dtau / (2 * rt.clamp(min=1e-300)), torch.sqrt(dtau))
    ds = torch.where(tau > 0, 2 * drt / (1 + rt) ** 2 + 2 * U * s.abs(), 4 * U * s.abs())
    tt = 1e-3
    den = (2 * k1 * r2 ** 2 * tt).abs()
    dsp = torch.where(tau >= 1e-6, sp.abs() * (drt / rt.clamp(min=1e-300) + 2 * drt / (1 + rt) + 5 * U),
                      8 * U * (2 * kr + tt) / torch.where(den == 0, torch.ones_like(den), den) + 4 * U * sp.abs())
    dt = t ** 2 * U * (1 + 5 * kr) + U * t.abs()
    zero = kr == 0
    return torch.where(zero, z, ds), torch.where(zero, z, dsp), dt


def fields(model, cams, gravs, H, W, dtype=torch.float64, device="cpu", clamp_hi=LAT_HI32, mutant=None):
    """Per-pixel fields of (n, 8) cameras and (n, 3) gravities, (n, H, W) planes: a dict of q (..., 2), up (..., 2,
    normalised), sin (the dot product before the clamp), lat, and, in float64, the error bounds dq (..., 2) and ds.
    dtype float64 is the yardstick; float32 restates the kernel's evaluation order (1/f once, then products; q * (1/|q|)).
    `mutant` (CPU self-check only) names one deliberate error: offset, swap, noclamp, halfpx, fxfy, renorm, cancelling."""
    c = cams.to(device=device, dtype=dtype)
    g = gravs.to(device=device, dtype=dtype)
    fx, fy, cx, cy, k1, k2 = (c[:, i, None, None] for i in range(2, 8))
    if mutant == "fxfy":
        fx, fy = fy, fx
    if mutant == "renorm":
        g = g / g.norm(dim=-1, keepdim=True)
    a, b, gc = (g[:, i, None, None] for i in range(3))
    x = torch.arange(W, device=device, dtype=dtype)[None, None, :] + (0.5 if mutant == "halfpx" else 0.0)
    y = torch.arange(H, device=device, dtype=dtype)[None, :, None] + (0.5 if mutant == "halfpx" else 0.0)
    if dtype == torch.float64:
        u, v = (x - cx) / fx, (y - cy) / fy
    else:
        u, v = (x - cx) * (1 / fx), (y - cy) * (1 / fy)
    u, v = u.expand(-1, H, -1), v.expand(-1, -1, W)
    r2 = u * u + v * v
    s, sp, t = scales(model, k1, k2, r2, cancelling=mutant == "cancelling")
    px, py = a - gc * u, b - gc * v
    if model == "pinhole" or mutant == "offset":
        w = o = torch.zeros_like(r2)
        qx, qy = s * px, s * py
    else:
        w = u * px + v * py
        o = 2 * sp * w
        qx, qy = s * px + o * u, s * py + o * v
    q = torch.stack([qx, qy], -1)
    n = torch.sqrt(qx * qx + qy * qy)
    up = q / n.clamp(min=1e-12)[..., None] if dtype == torch.float64 else q * (1 / n.clamp(min=1e-12))[..., None]
    tl = s if mutant == "swap" else t
    X, Y = u * tl, v * tl
    nr = torch.sqrt(X * X + Y * Y + 1)
    num = X * a + Y * b + gc
    sd = num / nr
    lat = torch.asin(sd) if mutant == "noclamp" else torch.asin(sd.clamp(-clamp_hi, clamp_hi))
    out = {"q": q, "up": up, "sin": sd, "lat": lat, "qnorm": n}
    if dtype != torch.float64:
        return out
    # first-order float32 error bounds, from the magnitudes of the terms
    ds, dsp, dt = _error_of_scales(model, k1, k2, r2, s, sp, t)
    du, dv = 3 * U * u.abs(), 3 * U * v.abs()
    dpx = U * (px.abs() + 3 * (gc * u).abs()) + gc.abs() * du
    dpy = U * (py.abs() + 3 * (gc * v).abs()) + gc.abs() * dv
    if model == "pinhole":
        dqx, dqy = dpx, dpy
    else:
        dw = u.abs() * dpx + px.abs() * du + v.abs() * dpy + py.abs() * dv + 2 * U * ((u * px).abs() + (v * py).abs())
        do = 2 * (dsp * w.abs() + sp.abs() * dw) + U * o.abs()
        dqx = ds * px.abs() + s.abs() * dpx + do * u.abs() + o.abs() * du + 2 * U * ((s * px).abs() + (o * u).abs())
        dqy = ds * py.abs() + s.abs() * dpy + do * v.abs() + o.abs() * dv + 2 * U * ((s * py).abs() + (o * v).abs())
    dX = t.abs() * du + u.abs() * dt + U * X.abs()
    dY = t.abs() * dv + v.abs() * dt + U * Y.abs()
    dnum = a.abs() * dX + b.abs() * dY + 2 * U * ((X * a).abs() + (Y * b).abs() + gc.abs())
    dnr = (X.abs() * dX + Y.abs() * dY) / nr + 2 * U * nr
    out["dq"] = torch.stack([dqx, dqy], -1)
    out["ds"] = dnum / nr + num.abs() * dnr / nr ** 2 + U * sd.abs()
    return out


def kappas(model, cams, gravs, H, W, device="cpu", ref=None):
    """(kappa_q, kappa_s): 4 x the worst ratio of the float32 restatement's q and sin(latitude) to delta_q and delta_s,
    at least 1."""
    ref = ref if ref is not None else fields(model, cams, gravs, H, W, device=device)
    f32 = fields(model, cams, gravs, H, W, torch.float32, device)
    rq = ((f32["q"].double() - ref["q"]).abs() / ref["dq"].clamp(min=1e-300)).max().item()
    rs = ((f32["sin"].double() - ref["sin"]).abs() / ref["ds"].clamp(min=1e-300)).max().item()
    return max(4 * rq, 1.0), max(4 * rs, 1.0)


def ulp32(x):
    """ulp of |x| in float32 (x in float64; 0 -> the smallest normal's)."""
    e = torch.floor(torch.log2(x.abs().clamp(min=2.0 ** -126)))
    return torch.exp2(e - 23)


def gates(ref, kq, ks, clamp_hi=LAT_HI32):
    """Per-pixel bounds (up normalised (..., 2), q (..., 2), lat) of the module docstring."""
    dq = ref["dq"]
    b_up = (kq * dq.sum(-1) / ref["qnorm"])[..., None].expand_as(dq) + 2 * 2.0 ** -23
    b_q = kq * dq
    s, lat = ref["sin"], ref["lat"]
    lo = torch.asin((s - ks * ref["ds"]).clamp(-clamp_hi, clamp_hi))
    hi = torch.asin((s + ks * ref["ds"]).clamp(-clamp_hi, clamp_hi))
    b_lat = torch.maximum((hi - lat).abs(), (lat - lo).abs()) + 2 * ulp32(lat)
    return b_up, b_q, b_lat


def worst_ratio(out, ref, bound):
    """max |out - ref| / bound; a NaN or inf output where the yardstick is finite counts as inf."""
    d = (out.double() - ref).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, math.inf))
    return (d / bound).max().item() if d.numel() else 0.0


# Cases of the GPU parity test: (model, k1, k2, B, H, W, gravity kind, normalize).  k None: drawn across dist_range per
# camera.  fx != fy and an off-centre principal point throughout (make_cameras); strong distortion, simple_divisional with
# the singular circle 4 k1 r2 = 1 inside the image (k1 = 3: r = 0.29) and pixels beyond it, |k| <= 1e-4 and k = 0, pitch
# +-1.5 (the vanishing point in the image), roll near +-pi/2, normalize=False, sizes 1x1, 2x2 and 641x479, B up to 64.
CASES = [
    ("pinhole", None, None, 7, 479, 641, "random", True),
    ("pinhole", None, None, 3, 479, 641, "pitch+", True),
    ("pinhole", None, None, 3, 479, 641, "pitch-", False),
    ("simple_radial", None, None, 7, 479, 641, "random", True),
    ("simple_radial", 0.7, None, 3, 479, 641, "roll+", True),
    ("simple_radial", -0.7, None, 3, 479, 641, "pitch+", False),
    ("simple_radial", 0.0, None, 3, 479, 641, "random", True),
    ("radial", None, None, 7, 479, 641, "random", True),
    ("radial", 0.7, 0.7, 3, 479, 641, "pitch-", True),
    ("radial", -0.7, 0.3, 3, 479, 641, "roll-", False),
    ("radial", 1e-4, -1e-4, 3, 479, 641, "random", True),
    ("simple_divisional", None, None, 7, 479, 641, "random", True),
    ("simple_divisional", 3.0, None, 3, 479, 641, "random", True),
    ("simple_divisional", 3.0, None, 3, 479, 641, "pitch+", False),
    ("simple_divisional", -3.0, None, 3, 479, 641, "roll+", True),
    ("simple_divisional", 1e-4, None, 3, 479, 641, "random", True),
    ("simple_divisional", -1e-6, None, 3, 479, 641, "pitch-", False),
    ("simple_divisional", 0.0, None, 2, 479, 641, "random", True),
    ("radial", None, None, 3, 1, 1, "random", True),
    ("simple_divisional", None, None, 3, 2, 2, "pitch+", False),
    ("pinhole", None, None, 2, 2, 2, "random", True),
    ("simple_radial", None, None, 64, 120, 160, "random", True),
    ("simple_divisional", None, None, 64, 120, 160, "roll-", False),
]


def case_inputs(case, seed=0):
    """(cams (B, 8), gravs (B, 3)) float32 of one case."""
    model, k1, k2, B, H, W, kind, _ = case
    return make_cameras(model, B, H, W, k1, k2, seed), make_gravity(B, kind, seed)
