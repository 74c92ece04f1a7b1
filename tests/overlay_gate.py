"""Float64 yardstick and per-pixel gate of the field overlay (gclm_draw_fields, gclm_draw_fields_u8;
viz.draw_perspective_fields), shared by the CPU self-check (test_overlay_abi.py) and the GPU tests (test_overlay.py).

Yardstick: the definition of include/gclm.h in float64 from the float32 inputs (`render`, written here on its own: it shares no
code with viz.compose).  Gate, per pixel and channel:
    bytes:  |out - ref| <= 0.5 + bound          (0.5: the quantiser)
    floats: |out - ref| <= bound / 255
bound is DERIVED per case on the CPU, never from the kernel under test: 4 x the largest difference between a float32
restatement of the kernel's evaluation order (`render` in float32: 1 / f once, then products; float32 step and degrees; a
level as (2 k - (levels - 1)) 90 / (levels - 1)) and float64 over the pixels that are not excluded, plus 2 ulp of 255 (what contracted multiply-adds may move the last blend by),
as reproject_gate.coordinate_bound does for coordinates.

The definition is discontinuous in two places, and those pixels are excluded from the value gate:
  - where the nearest latitude level changes while a level's coverage is not zero: |lat - L_k| within 1e-3 step of step / 2 and
    g (halfwidth + 0.5) > 0.49 step;
  - within reach of an arrow anchor whose unnormalised up vector is shorter than 1e-3 (the direction's conditioning is 1 / |q|,
    and below 1e-6 the arrow is not drawn).
Excluded pixels are at most 2 % of any image: a condition on the cases, asserted for every case on the CPU.

Rounding: ties cannot be told from the value gate (either neighbour is 0.5 away), so TIE_CASE makes every intermediate
exact -- a tint of alpha 0.5 from a palette of one colour -- and `ties_to_even` holds those bytes to the even neighbour."""
import math
from collections import namedtuple

import torch

from geocalib_amd import viz

CAP = 0.02
HEAT, TINT, CONTOURS, HORIZON, ARROWS = 1, 2, 4, 8, 16
ALL = HEAT | TINT | CONTOURS | HORIZON | ARROWS
MODELS = ("pinhole", "simple_radial", "radial", "simple_divisional")
DIST = {"pinhole": (0.0, 0.0), "simple_radial": (0.2, 0.0), "radial": (-0.15, 0.06), "simple_divisional": (0.12, 0.0)}
# (roll, pitch) in degrees: the horizon in the frame, the pole in the frame, a level camera, nearly upside down
GRAVITIES = {"horizon": (12.0, 8.0), "pole": (-20.0, 85.0), "level": (0.0, 0.0), "roll170": (170.0, 17.0)}
LAT_HI32 = float(torch.tensor(1 - 1e-6, dtype=torch.float32))

Case = namedtuple("Case", "model grav H W B nb C layers")


def _cases():
    out = [Case(m, g, 48, 64, 3, 3, 3, ALL) for m in MODELS for g in GRAVITIES]                   # every model and gravity
    out += [Case("simple_radial", "horizon", 48, 64, 3, 1, 3, layer) for layer in (HEAT, TINT, CONTOURS, HORIZON, ARROWS)]
    out += [Case("radial", "horizon", 41, 59, 3, 3, 3, ALL), Case("radial", "roll170", 41, 59, 3, 1, 4, ALL),
            Case("simple_divisional", "horizon", 5, 130, 3, 3, 4, ALL), Case("pinhole", "level", 5, 130, 3, 1, 3, ALL),
            Case("pinhole", "horizon", 1, 1, 3, 3, 3, ALL), Case("simple_radial", "level", 1, 1, 3, 1, 4, TINT | HEAT)]
    return out


CASES = _cases()
TIE_CASE = Case("simple_radial", "horizon", 41, 59, 3, 3, 4, TINT)


def case_id(c):
    names = {ALL: "all", HEAT: "heat", TINT: "tint", CONTOURS: "contours", HORIZON: "horizon", ARROWS: "arrows", TINT | HEAT: "tint+heat"}
    return f"{c.model}-{c.grav}-{c.H}x{c.W}-nb{c.nb}-C{c.C}-{names[c.layers]}"


def style_of(c, tie=False):
    """Explicit styles (the default line width is 0 pixels at these sizes): lines of half-width 1, an arrow every 12 pixels, 7
    long, half-width 1 (7 + 1 + 0.5 <= 12)."""
    S = 12
    return viz.OverlayStyle(line_halfwidth=1.0, arrow_step=S, arrow_x0=((c.W % S) + S) // 2, arrow_y0=min(int(0.9 * S), c.H // 2),
                            arrow_length=7.0, arrow_halfwidth=1.0, tint_alpha=0.5 if tie else 0.4)


def heat_palette():
    """A smooth (256, 3) palette of the test's own (matplotlib's "turbo" is not needed)."""
    i = torch.arange(256, dtype=torch.float64)
    return torch.stack([i, 255 - i, 128 + 100 * torch.sin(i / 20)], -1).round().to(torch.uint8)


def case_inputs(c, tie=False):
    """dict of one case: cams (nb, 8), gravs (nb, 3) float32, img (B, C, H, W) uint8 noise, conf (B, H, W) float32 spanning both
    clamps of the heat range with zeros and values above 1, the two palettes, the style."""
    g = torch.Generator().manual_seed(1000 * c.H + c.W + 7 * c.nb + c.C)
    k1, k2 = DIST[c.model]
    n = torch.arange(c.nb, dtype=torch.float64)
    fx = max(0.8 * c.W + 10, 40.0) * (1 + 0.1 * n)
    cams = torch.stack([torch.full_like(n, c.W), torch.full_like(n, c.H), fx, 1.07 * fx, c.W / 2 + 0.7 + n, c.H / 2 - 0.4 - n,
                        k1 * (1 - 0.2 * n), k2 * (1 + 0.3 * n)], -1).to(torch.float32)
    roll, pitch = (math.radians(v) for v in GRAVITIES[c.grav])
    roll, pitch = roll + 0.1 * n, pitch * (1 - 0.15 * n) + 0.02 * n
    h = -torch.cos(pitch)
    gravs = torch.stack([torch.sin(roll) * h, torch.cos(roll) * h, torch.sin(pitch)], -1).to(torch.float32)
    img = torch.randint(0, 256, (c.B, c.C, c.H, c.W), generator=g, dtype=torch.uint8)
    conf = 10 ** (torch.rand((c.B, c.H, c.W), generator=g, dtype=torch.float64) * 5.5 - 5.2)
    conf[torch.rand((c.B, c.H, c.W), generator=g) < 0.05] = 0.0
    pal = torch.tensor([[101, 50, 7]], dtype=torch.uint8).expand(256, 3).contiguous() if tie else viz.resolve_palette("seismic", "cpu")
    return {"cams": cams, "gravs": gravs, "img": img, "conf": conf.to(torch.float32), "pal": pal, "heat": heat_palette(),
            "style": style_of(c, tie)}


# ------------------------------------------------------------------ the definition
def _scales(model, k1, k2, r2):
    """(s, s', t, t'): distort scale and ds/dr2 (non-cancelling forms), undistort scale and dt/dr2."""
    one = torch.ones_like(r2)
    if model == "pinhole":
        return one, 0 * one, one, 0 * one
    if model == "simple_radial":
        return 1 + k1 * r2, k1 * one, 1 - k1 * r2, -k1 * one
    if model == "radial":
        m = 3 * k1 * k1 - k2
        return 1 + (k1 + k2 * r2) * r2, k1 + 2 * k2 * r2, 1 - k1 * r2 + m * (r2 * r2), -k1 + 2 * m * r2
    kr = k1 * r2
    den = 1 + kr
    t = 1 / torch.where(den == 0, 1e6 * one, den)
    tau = 1 - 4 * kr
    rt = torch.sqrt(tau.clamp(min=0))
    s = torch.where(tau > 0, 2 / (1 + rt), 1 / torch.where(kr == 0, one, 2 * kr))
    tt = math.sqrt(1e-6)
    d2 = 2 * k1 * r2 * r2 * tt
    sp = torch.where(tau >= 1e-6, 4 * k1 / torch.where(rt == 0, one, rt * (1 + rt) ** 2),
                     (2 * kr - (1 - tt) * tt) / torch.where(d2 == 0, 1e6 * one, d2))
    return torch.where(kr == 0, one, s), torch.where(kr == 0, 0 * one, sp), t, -k1 * t * t


def _pal(pal, tau, nearest=False):
    p = 255 * tau
    if nearest:                                  # (mutant: matplotlib's bin)
        return pal[(tau * 256).floor().clamp(0, 255).long()]
    i = p.floor().clamp(0, 254)
    f = (p - i)[..., None]
    i = i.long()
    return pal[i] + (pal[i + 1] - pal[i]) * f


def _cover(hw, d):
    return torch.nan_to_num(hw + 0.5 - d, nan=0.0).clamp(0, 1)


def _seg(wx, wy, dx, dy):
    len2 = dx * dx + dy * dy
    s = torch.where(len2 > 0, (wx * dx + wy * dy) / torch.where(len2 > 0, len2, torch.ones_like(len2)), 0 * len2).clamp(0, 1)
    return torch.sqrt((wx - s * dx) ** 2 + (wy - s * dy) ** 2)


def render(c, inp, dtype=torch.float64, unit=1.0, img=None, mutant=None):
    """The drawn channels 0..2 of one case, (B, 3, H, W) in `dtype`, unrounded, and the exclusion mask (B, H, W).  `img`: the
    image in the units of `unit` (default: the bytes as 0..255).  float64 is the yardstick; float32 restates the kernel's
    evaluation order.  `mutant` names one deliberate error (CPU self-check)."""
    st, layers = inp["style"], c.layers
    f32 = dtype == torch.float32
    img = (inp["img"] if img is None else img).to(dtype)
    B, H, W = c.B, c.H, c.W
    out = img[:, :3].permute(0, 2, 3, 1).clone()
    cam, grav = inp["cams"].to(dtype), inp["gravs"].to(dtype)
    fx, fy, cx, cy, k1, k2 = (cam[:, i, None, None] for i in range(2, 8))
    a, b, gc = (grav[:, i, None, None] for i in range(3))
    ifx, ify = 1 / fx, 1 / fy
    deg = float(torch.tensor(180 / math.pi, dtype=torch.float32)) if f32 else 180 / math.pi
    off = 0.5 if mutant == "half-pixel offset" else 0.0
    xs = torch.arange(W, dtype=dtype)[None, None, :] + off
    ys = torch.arange(H, dtype=dtype)[None, :, None] + off
    excluded = torch.zeros((B, H, W), dtype=torch.bool)
    hw = st.line_halfwidth + (1 if mutant == "half-width + 1" else 0)

    def blend(o, colour, alpha):
        alpha = alpha if isinstance(alpha, float) else alpha[..., None]
        return o * (1 - alpha) + colour * unit * alpha

    def norm(p, q):             # (p - q) / f as the kernel takes it in float32
        return (p - q) * (ifx if q is cx else ify) if f32 else (p - q) / (fx if q is cx else fy)

    pal, heat = inp["pal"].to(dtype), inp["heat"].to(dtype)
    if layers & HEAT:
        cf = inp["conf"].to(dtype)
        lo, hi = st.heat_range
        tau = (torch.log10(cf.clamp(min=1e-6)).clamp(lo, hi) - lo) / (hi - lo)
        out = blend(out, _pal(heat, tau, mutant == "nearest-bin palette"), float(st.heat_alpha))
    if layers & (TINT | CONTOURS | HORIZON):
        u, v = norm(xs, cx).expand(-1, H, -1), norm(ys, cy).expand(-1, -1, W)
        r2 = u * u + v * v
        _, _, t, tp = _scales(c.model, k1, k2, r2)
        X, Y = u * t, v * t
        n = torch.sqrt(X * X + Y * Y + 1)
        s = (X * a + Y * b + gc) / n
        sc = s.clamp(-LAT_HI32, LAT_HI32)
        lat = torch.asin(sc) * deg
        gX, gY = (a - s * X / n) / n, (b - s * Y / n) / n
        w = 2 * tp * (u * gX + v * gY)
        sx, sy = (t * gX + w * u) * ifx, (t * gY + w * v) * ify
        slope = torch.sqrt(sx * sx + sy * sy) * deg / torch.sqrt((1 - sc) * (1 + sc))
        dist = 1 / slope.clamp(min=1e-4)
        if layers & TINT:
            tau = (lat + 90) * (1 / 180) if f32 else (lat + 90) / 180
            out = blend(out, _pal(pal, tau, mutant == "nearest-bin palette"), 0.5 if mutant == "tint alpha 0.5" else float(st.tint_alpha))
        last = st.levels - 1
        step = 180 / (st.levels if mutant == "level step 180/15" else last)
        if f32:
            step = float(torch.tensor(step, dtype=torch.float32))
        if layers & CONTOURS:
            k = torch.round((lat + 90) / step)
            level = (2 * k - last) * 90 / last if f32 else k * step - 90          # (the same number; the kernel's form is exact at 0)
            miss = (lat - level).abs()
            out = blend(out, _pal(pal, (k / last).clamp(0, 1), mutant == "nearest-bin palette"), _cover(hw, miss * dist))
            near_tie = ((step / 2 - miss) < 1e-3 * step) & (slope * (hw + 0.5) > 0.49 * step)
            excluded = excluded | near_tie.expand(B, -1, -1)
        if layers & HORIZON:
            out = blend(out, torch.tensor(st.horizon_color, dtype=dtype), _cover(hw, lat.abs() * dist))
    if layers & ARROWS:
        S, Ln = st.arrow_step, float(st.arrow_length)
        shift = S if mutant == "arrows one cell off" else 0
        ax = torch.arange(st.arrow_x0 + shift, max(W, st.arrow_x0 + shift), S, dtype=dtype)
        ay = torch.arange(st.arrow_y0, max(H, st.arrow_y0), S, dtype=dtype)
        best = torch.zeros((c.nb, H, W), dtype=dtype)
        reach = Ln + st.arrow_halfwidth + 0.5
        ct, sn = (math.cos(math.radians(30)), math.sin(math.radians(30))) if mutant == "tip at 30 degrees" else (math.sqrt(0.5),) * 2
        tip = st.arrow_tip * Ln
        for j in range(ay.numel()):
            for i in range(ax.numel()):
                ua, va = norm(ax[i], cx), norm(ay[j], cy)                         # (nb, 1, 1)
                s, sp, _, _ = _scales(c.model, k1, k2, ua * ua + va * va)
                px, py = a - gc * ua, b - gc * va
                o = 2 * sp * (ua * px + va * py)
                qx, qy = s * px + o * ua, s * py + o * va
                n = torch.sqrt(qx * qx + qy * qy)
                draws = (n >= 1e-6) & torch.isfinite(n)
                n = torch.where(draws, n, torch.ones_like(n))
                ex, ey = qx / n, qy / n
                wx, wy = (xs - off - ax[i]).expand(-1, H, -1), (ys - off - ay[j]).expand(-1, -1, W)
                d = _seg(wx, wy, Ln * ex, Ln * ey)
                tx, ty = wx - Ln * ex, wy - Ln * ey
                d = torch.minimum(d, _seg(tx, ty, tip * (-ct * ex - sn * ey), tip * (-ct * ey + sn * ex)))
                d = torch.minimum(d, _seg(tx, ty, tip * (-ct * ex + sn * ey), tip * (-ct * ey - sn * ex)))
                cov = _cover(st.arrow_halfwidth, d)
                best = torch.maximum(best, torch.where(draws, cov, torch.zeros_like(cov)))
                weak = (n < 1e-3) | ~draws
                excluded = excluded | (weak & (wx.abs() < reach) & (wy.abs() < reach)).expand(B, -1, -1)
        out = blend(out, torch.tensor(st.arrow_color, dtype=dtype), best)
    out = out.permute(0, 3, 1, 2)
    if mutant == "swapped channel order":
        out = out.flip(1)
    return out, excluded


def parts(c, tie=False):
    """One case on the CPU: inputs, the float64 yardstick `ref` (B, 3, H, W) in byte units, `excluded` (B, H, W), `bound` (a
    scalar, byte units) and the same for the float image img / 255 (`ref_f`, in 0..1 units, `bound_f` in byte units)."""
    inp = case_inputs(c, tie)
    ref, ex = render(c, inp)
    keep = ~ex[:, None].expand_as(ref)
    floor = 2 * 255 * 2.0 ** -23
    img_f = inp["img"].to(torch.float32) / 255
    ref_f, _ = render(c, inp, unit=1 / 255, img=img_f)

    r32, _ = render(c, inp, torch.float32)
    r32_f, _ = render(c, inp, torch.float32, unit=1 / 255, img=img_f)
    worst = lambda r, reference: (r.double() - reference).abs()[keep].max().item() if keep.any() else 0.0  # noqa: E731
    bound = 4 * worst(r32, ref) + floor
    bound_f = 4 * 255 * worst(r32_f, ref_f) + floor
    return {**inp, "ref": ref, "excluded": ex, "bound": bound, "img_f": img_f, "ref_f": ref_f, "bound_f": bound_f,
            "share": ex.double().mean(dim=(1, 2)).max().item()}


def quantise(out32):
    """The definition's last step: nearest, ties to even (torch.round), saturated."""
    return out32.round().clamp(0, 255).to(torch.uint8)


def worst_ratio(out, p, floats=False):
    """max |out - ref| / gate over channels 0..2 of the pixels that are not excluded; a non-finite output counts as inf."""
    ref = p["ref_f"] if floats else p["ref"]
    gate = p["bound_f"] / 255 if floats else 0.5 + p["bound"]
    keep = ~p["excluded"][:, None].expand_as(ref)
    if not keep.any():
        return 0.0
    d = (out[:, :3].double() - ref).abs()[keep]
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, math.inf))
    return (d / gate).max().item()


def ties_to_even(out, p):
    """TIE_CASE: every pixel is exactly (byte + colour) / 2, so the byte written is known: the even neighbour at a tie.
    Returns (bytes wrong, ties among them all)."""
    total = p["img"][:, :3].int() + p["pal"][0].int()[None, :, None, None]
    half = total // 2
    want = torch.where(total % 2 == 1, half + (half & 1), half).to(torch.uint8)
    return int((out[:, :3] != want).sum()), int((total % 2 == 1).sum())
