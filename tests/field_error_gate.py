"""Float64 yardstick and gates of gclm_field_errors (metrics.perspective_field_metrics on the HIP path), shared by the CPU
self-check (test_field_errors_abi.py) and the GPU parity test (test_field_errors.py).  Built on perspective_gate.py.

Yardstick: the reference's formulas in float64 on the float32 inputs -- the target fields from perspective_gate.fields(...,
float64), the up error rad2deg(acos(F.cosine_similarity(p, t, dim=1).clamp(-1, 1))) times the mask (p_x + p_y != 0)
evaluated on the float32 sum, the latitude error rad2deg(|lat - t_lat|), then mean, confidence-weighted mean and recalls.

Per-pixel gates (degrees), base terms:
    up:   asin(|b_up|) + (8 U + 4 U theta),  b_up perspective_gate's bound on the target's up direction (its kappa
          included), |.| over the two components: the angle that bound subtends; then the float32 rounding of the angle
          evaluation itself -- cross and dot product carry ~3 U |p| |t| each, atan2 and the conversion a few ulp of theta.
    lat:  b_lat + 2 ulp(lat) + 2 ulp(e),  b_lat perspective_gate's latitude bound, lat the prediction.
Each is scaled by a kappa DERIVED per case: 4 x the worst ratio of a float32 CPU restatement of the kernel's evaluation
(`restate`) against the yardstick to that base, at least 1.
Means: the mean of the per-pixel gates, plus a summation term kappa_s 12 U mean|e| (the kernel adds at most 12 float32
roundings per value before the float64 part: pixels of a lane, six butterfly levels, four waves), kappa_s derived as 4 x the
worst ratio of the restated block-then-float64 sum of the SAME float32 values against their float64 sum, at least 1; plus
2 U of the mean for the final rounding.  Weighted means: the same with the weights (numerator and denominator each carry a
summation term, the product one more rounding).
Recalls: an interval, not a tolerance -- the device count must lie in [#(e64 < t - gate), #(e64 < t + gate)], no pixel
exempt."""
import math

import torch
from torch.nn import functional as F

import perspective_gate as pg

U = pg.U
DEG = 180.0 / math.pi
THRESHOLDS = (1, 3, 5, 10)
BAND_SCALES = (0.1, 0.4, 1.2, 4.0)      # the perturbation of the four column bands of a prediction, x (3 deg, 3 deg, 3 %)
DIV_K1 = (0.8, -2.0, 0.25)

# (model, B, H, W, gravity kind, planes offset by 4 bytes)
SHAPES = [(3, 37, 53), (2, 30, 200), (2, 9, 132)]
CASES = [(m, B, H, W, "random", off) for m in pg.MODELS for (B, H, W) in SHAPES for off in (False, True)]
EXTREMES = [(m, 2, 30, 44, kind, False) for m in ("simple_divisional", "pinhole") for kind in ("pitch+", "roll+")]


def case_id(case):
    m, B, H, W, kind, off = case
    return f"{m}-B{B}-{H}x{W}-{kind}{'-off4' if off else ''}"


def _perturbed(cams, gravs, scale):
    """The calibration moved by scale x (roll 3 deg, pitch 3 deg, focal 3 %)."""
    g = gravs.double()
    pitch, roll = torch.asin(g[:, 2].clamp(-1, 1)), torch.atan2(-g[:, 0], -g[:, 1])
    pitch, roll = pitch - scale * math.radians(3), roll + scale * math.radians(3)
    h = -torch.cos(pitch)
    c = cams.clone().double()
    c[:, 2:4] *= 1 + 0.03 * scale
    return c.float(), torch.stack([torch.sin(roll) * h, torch.cos(roll) * h, torch.sin(pitch)], -1).float()


def make_case(case, seed=0):
    """Inputs of one case, float32 on the CPU: cams (B, 8), gravs (B, 3) as stored, and `data` -- up_field (B, 2, H, W),
    latitude_field (B, 1, H, W), both confidences (B, H, W).

    A prediction is the float64 field of a perturbed calibration, rounded: its four column bands are perturbed by
    BAND_SCALES x (3 deg of roll, 3 deg of pitch, 3 % of focal), so that one image's errors span 0 .. 15 deg and every default
    threshold cuts through them.  The LAST image's prediction is the rounded target itself (the small-angle regime).  Image 0
    holds a 3 x 3 patch of (0, 0) up vectors, one pixel (x, -x) and one pixel of norm 5e-9, below torch's eps."""
    model, B, H, W, kind, _ = case
    k1 = [DIV_K1[i % 3] for i in range(B)] if model == "simple_divisional" else None
    cams, gravs = pg.make_cameras(model, B, H, W, k1, None, seed), pg.make_gravity(B, kind, seed)
    band = (torch.arange(W) * 4 // W)[None, None, :].expand(B, H, W)
    up, lat = torch.zeros(B, H, W, 2, dtype=torch.float64), torch.zeros(B, H, W, dtype=torch.float64)
    for k, s in enumerate(BAND_SCALES):
        f = pg.fields(model, *_perturbed(cams, gravs, s), H, W)
        up = torch.where((band == k)[..., None], f["up"], up)
        lat = torch.where(band == k, f["lat"], lat)
    exact = pg.fields(model, cams, gravs, H, W)
    up[-1], lat[-1] = exact["up"][-1], exact["lat"][-1]
    up = up.permute(0, 3, 1, 2).float().contiguous()
    up[0, :, 2:5, 3:6] = 0.0
    up[0, :, 7, 11] = torch.tensor([0.625, -0.625])
    up[0, :, 8, 20] = torch.tensor([3e-9, 4e-9])
    g = torch.Generator().manual_seed(seed + 1)
    conf = lambda: 0.01 + 0.98 * torch.rand(B, H, W, generator=g)  # noqa: E731
    data = {"up_field": up, "latitude_field": lat[:, None].float().contiguous(), "up_confidence": conf(),
            "latitude_confidence": conf()}
    return cams, gravs, data


def pixels_per_lane(W, offset4):
    """The kernel's rule: four pixels per lane where W % 4 == 0 and the planes are 16-byte aligned, two where W is even and
    they are 8-byte aligned, else one."""
    if offset4:
        return 1
    return 4 if W % 4 == 0 else 2 if W % 2 == 0 else 1


def block_sum(v, px):
    """Per-image sum of v (B, H, W) in the kernel's order: float32 within a tile of 4 rows x 64 px columns (the px pixels of a
    lane in turn, the butterfly over 64 lanes, the 4 waves in turn), then float64 over the tiles in 8 strided chains added
    in order.  Float64 input is summed in float64 throughout (the order then does not matter to the gates)."""
    B, H, W = v.shape
    tw = 64 * px
    Hp, Wp = -(-H // 4) * 4, -(-W // tw) * tw
    t = F.pad(v, (0, Wp - W, 0, Hp - H)).reshape(B, Hp // 4, 4, Wp // tw, 64, px)
    lane = t[..., 0]
    for j in range(1, px):
        lane = lane + t[..., j]
    o = 32
    while o >= 1:
        lane = lane.reshape(*lane.shape[:-1], 2, o)
        lane = lane[..., 0, :] + lane[..., 1, :]
        o //= 2
    wave = lane[..., 0]                               # (B, tiles_y, 4, tiles_x)
    tile = wave[:, :, 0]
    for i in range(1, 4):
        tile = tile + wave[:, :, i]
    tile = tile.reshape(B, -1).double()
    chains = torch.zeros(B, 8, dtype=torch.float64)
    for i in range(tile.shape[1]):
        chains[:, i % 8] += tile[:, i]
    total = chains[:, 0]
    for i in range(1, 8):
        total = total + chains[:, i]
    return total


def _angle32(px, py, tx, ty):
    """The kernel's up angle in float32 (gclm_metrics.hip: up_error_deg), before the mask, in degrees."""
    eps = torch.tensor(1e-8, dtype=torch.float32)
    pn2, tn2 = px * px + py * py, tx * tx + ty * ty
    dot, crs = px * tx + py * ty, px * ty - py * tx
    ok = (pn2 >= eps * eps) & (tn2 >= eps * eps)
    ip, it = 1 / torch.sqrt(pn2).clamp(min=1e-8), 1 / torch.sqrt(tn2).clamp(min=1e-8)
    dn, cn = dot * (ip * it), crs * (ip * it)
    n = (pn2 * ip * ip) * (tn2 * it * it)
    sn = torch.sqrt((1 - n).clamp(min=0) + cn * cn)
    return torch.atan2(torch.where(ok, crs.abs(), sn), torch.where(ok, dot, dn)) * torch.tensor(DEG, dtype=torch.float32)


def _stats(e_up, e_lat, data, px, thresholds, mutant=None):
    """(B, 2 (2 + n)) float32 statistics of per-pixel errors in the layout of include/gclm.h; a missing field or
    confidence gives NaN.  float32 errors are summed in the kernel's order."""
    rows = []
    confs = [data.get("up_confidence"), data.get("latitude_confidence")]
    if mutant == "swapconf":
        confs = confs[::-1]
    for e, c, name in ((e_up, confs[0], "up"), (e_lat, confs[1], "lat")):
        B = (e_up if e_up is not None else e_lat).shape[0]
        nan = torch.full((B,), math.nan, dtype=torch.float64)
        if e is None:
            rows += [nan] * (2 + len(thresholds))
            continue
        hw = e.shape[1] * e.shape[2]
        den = hw
        if mutant == "unmasked_mean" and name == "up":
            den = (data["up_field"].sum(1) != 0).sum((1, 2)).double()
        rows.append(block_sum(e, px) / den)
        rows.append(nan if c is None else block_sum(e * c.to(e.dtype), px) / block_sum(c.to(e.dtype), px))
        rows += [(e < t).sum((1, 2)).double() / hw for t in thresholds]
    return torch.stack(rows, -1).float()


def restate(case, cams, gravs, data, thresholds=THRESHOLDS, mutant=None):
    """A float32 CPU restatement of the kernel: {"stats", "up_err", "lat_err"}.  `mutant` (CPU self-check only) names one
    deliberate error: acos32, nomask, unmasked_mean, radians, swapconf, renorm, halfpx."""
    model, B, H, W, _, off = case
    f = pg.fields(model, cams, gravs, H, W, torch.float32, mutant=mutant if mutant in ("renorm", "halfpx") else None)
    deg = torch.tensor(1.0 if mutant == "radians" else DEG, dtype=torch.float32)
    e_up = e_lat = None
    if "up_field" in data:
        p = data["up_field"]
        if mutant == "acos32":
            e_up = torch.acos(F.cosine_similarity(p, f["up"].permute(0, 3, 1, 2), dim=1).clamp(-1, 1)) * deg
        else:
            e_up = _angle32(p[:, 0], p[:, 1], f["up"][..., 0], f["up"][..., 1]) * (deg / torch.tensor(DEG, dtype=torch.float32))
        if mutant != "nomask":
            e_up = e_up * (p[:, 0] + p[:, 1] != 0)
    if "latitude_field" in data:
        e_lat = (data["latitude_field"][:, 0] - f["lat"]).abs() * deg
    return {"stats": _stats(e_up, e_lat, data, pixels_per_lane(W, off), thresholds, mutant), "up_err": e_up, "lat_err": e_lat}


def yardstick(case, cams, gravs, data, thresholds=THRESHOLDS):
    """The float64 errors and statistics of one case with their gates: a dict of e_up, e_lat (B, H, W), stats (B, S) float64,
    g_up, g_lat (per-pixel gates), g_stats (B, S) (gates of the means; NaN in the recall columns), lo / hi (B, S) (the recall
    intervals as counts; NaN elsewhere)."""
    model, B, H, W, _, off = case
    px = pixels_per_lane(W, off)
    ref = pg.fields(model, cams, gravs, H, W)
    b_up, _, b_lat = pg.gates(ref, *pg.kappas(model, cams, gravs, H, W, ref=ref))
    r32 = restate(case, cams, gravs, data, thresholds)
    y = {"e_up": None, "e_lat": None, "g_up": None, "g_lat": None}

    def kappa(e32, e64, base):
        return max(1.0, 4 * ((e32.double() - e64).abs() / base).max().item())

    def kappa_sum(v32):
        return max(1.0, 4 * ((block_sum(v32, px) - v32.double().sum((1, 2))).abs()
                             / (12 * U * v32.double().abs().sum((1, 2))).clamp(min=1e-300)).max().item())

    if "up_field" in data:
        p = data["up_field"]
        cos = F.cosine_similarity(p.double(), ref["up"].permute(0, 3, 1, 2), dim=1).clamp(-1, 1)
        y["e_up"] = torch.acos(cos) * DEG * (p[:, 0] + p[:, 1] != 0)            # the mask on the float32 sum
        base = (torch.asin(b_up.norm(dim=-1).clamp(max=1)) + 8 * U + 4 * U * torch.acos(cos)) * DEG
        y["g_up"] = kappa(r32["up_err"], y["e_up"], base) * base * (p[:, 0] + p[:, 1] != 0)
        y["ks_up"] = kappa_sum(r32["up_err"])
    if "latitude_field" in data:
        lat = data["latitude_field"][:, 0].double()
        y["e_lat"] = (lat - ref["lat"]).abs() * DEG
        base = (b_lat + 2 * pg.ulp32(lat)) * DEG + 2 * pg.ulp32(y["e_lat"])
        y["g_lat"] = kappa(r32["lat_err"], y["e_lat"], base) * base
        y["ks_lat"] = kappa_sum(r32["lat_err"])
    y["stats"] = _stats(y["e_up"], y["e_lat"], {k: v.double() for k, v in data.items()}, px, thresholds).double()
    # (float64 statistics, rounded once: recompute the means without the rounding)
    S, per = 2 * (2 + len(thresholds)), 2 + len(thresholds)
    g_stats, lo, hi = (torch.full((B, S), math.nan, dtype=torch.float64) for _ in range(3))
    for i, (e, g, c, ks) in enumerate(((y["e_up"], y["g_up"], data.get("up_confidence"), y.get("ks_up")),
                                       (y["e_lat"], y["g_lat"], data.get("latitude_confidence"), y.get("ks_lat")))):
        if e is None:
            continue
        mean = e.mean((1, 2))
        y["stats"][:, i * per] = mean
        g_stats[:, i * per] = g.mean((1, 2)) + (12 * ks + 2) * U * mean
        if c is not None:
            c = c.double()
            w = (e * c).sum((1, 2)) / c.sum((1, 2))
            ksw = max(ks, kappa_sum((r32["up_err"] if i == 0 else r32["lat_err"]) * c.float()), kappa_sum(c.float()))
            y["stats"][:, i * per + 1] = w
            g_stats[:, i * per + 1] = (g * c).sum((1, 2)) / c.sum((1, 2)) + (25 * ksw + 2) * U * w
        for j, t in enumerate(thresholds):
            y["stats"][:, i * per + 2 + j] = (e < t).sum((1, 2)).double() / (H * W)
            lo[:, i * per + 2 + j] = (e < t - g).sum((1, 2))
            hi[:, i * per + 2 + j] = (e < t + g).sum((1, 2))
    y.update(g_stats=g_stats, lo=lo, hi=hi, hw=H * W)
    return y


def verdict(y, out):
    """Worst ratios of `out` ({"stats" (B, S), optional "up_err", "lat_err"}) to the gates of yardstick `y`: up_px, lat_px
    (per-pixel maps, when given), means (mean and weighted mean columns), recalls (counts outside their interval, or
    recalls that are no count / (H W)), nan (entries whose NaN-ness differs from the yardstick's).  All <= 1 / == 0: pass."""
    v = {"up_px": 0.0, "lat_px": 0.0}
    for key, e, g in (("up_px", "e_up", "g_up"), ("lat_px", "e_lat", "g_lat")):
        m = out.get(key.replace("_px", "_err"))
        if m is not None:
            d = (m.double().cpu() - y[e]).abs()
            d = torch.where(torch.isfinite(d), d, torch.full_like(d, math.inf))
            # a gate of 0 (a masked pixel) asks for exactly 0
            v[key] = torch.where(d == 0, torch.zeros_like(d), d / y[g].clamp(min=1e-300)).max().item()
    s = out["stats"].double().cpu()
    assert s.shape == y["stats"].shape, (s.shape, y["stats"].shape)
    v["nan"] = int((s.isnan() != y["stats"].isnan()).sum())
    is_mean = ~y["g_stats"].isnan() & ~s.isnan()
    d = (s - y["stats"]).abs() / y["g_stats"].clamp(min=1e-300)
    v["means"] = d[is_mean].max().item() if is_mean.any() else 0.0
    is_rec = ~y["lo"].isnan() & ~s.isnan()
    count = (s * y["hw"]).round()
    off_grid = (count / y["hw"] - s).abs() > 2 * U * s.abs()
    v["recalls"] = int((((count < y["lo"]) | (count > y["hi"]) | off_grid) & is_rec).sum())
    return v


def passes(v):
    return v["up_px"] <= 1 and v["lat_px"] <= 1 and v["means"] <= 1 and v["recalls"] == 0 and v["nan"] == 0


def subset(data, which):
    """The four ways a shape is scored: all (both fields, both confidences), noconf, up, lat (one field with its confidence)."""
    if which == "noconf":
        return {k: v for k, v in data.items() if "confidence" not in k}
    if which in ("up", "lat"):
        return {k: v for k, v in data.items() if k.startswith("up" if which == "up" else "latitude")}
    return dict(data)
