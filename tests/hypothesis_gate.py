"""Float64 yardstick and gates of gclm_hypothesis_scores (metrics.rank_calibrations on the HIP path), shared by the CPU
self-check (test_hypothesis_scores_abi.py) and the GPU parity test (test_hypothesis_scores.py).  Built on
field_error_gate.py, imported and not edited.

Cases are field_error_gate's: predictions and confidences from make_case.  The hypotheses of image b are its calibration
moved by field_error_gate._perturbed(cams, gravs, s), s from SCALES and, beyond its seven entries, from further scales
(`scale`); entries 2 and 6 (both 0.0) are identical rows, so the lower index must win between them.

Yardstick: for hypothesis n, field_error_gate.yardstick(case, cams[:, n], gravs[:, n], data) gives the float64 errors e and
the per-pixel gates g of that calibration.  With c = confidence x mask in float64 (a missing one is 1) and t the threshold,
a field's score must lie in
    [ sum c [e < t - g],  sum c [e < t + g] ]    widened by    kappa_s K_ROUND U sum |c|,
no pixel exempt.  K_ROUND = 14 counts the float32 roundings of one value on its way into a score: the product confidence x
mask (1), the pixels of a lane (at most 3 additions), six butterfly levels, the four waves (3) -- 13 before the float64
part -- and the rounding of the float64 sum to the float32 score (1).  kappa_s is derived as field_error_gate's: 4 x the
worst ratio of the restated block-then-float64 sum (field_error_gate.block_sum, whose order is the kernel's) of the SAME
float32 values against their float64 sum, to K_ROUND U sum |c|, at least 1.
total is held to up_weight x (up interval) + lat_weight x (latitude interval), plus 2 U |total| (the product-sum is formed in
float64 and rounded once).
best must (a) equal the first argmax of the returned float32 totals, exactly (NaN the maximum), and (b) lie in the
admissible set: the indices whose upper bound reaches the largest lower bound of that image."""
import math

import torch

import field_error_gate as fg

U = fg.U
K_ROUND = 14
SCALES = (1.2, 0.1, 0.0, 0.4, 0.05, -0.3, 0.0)
PAIR = (2, 6)                                 # the identical rows


def scale(i):
    """The perturbation scale of hypothesis i: SCALES, then further values between -1.5 and 1.5, none of them repeated."""
    if i < len(SCALES):
        return SCALES[i]
    j = i - len(SCALES)
    return (-1) ** j * (0.15 + 0.045 * j)


def hypotheses(cams, gravs, N):
    """(B, N, 8) cameras and (B, N, 3) gravities, float32: the calibration moved by scale(0) .. scale(N - 1)."""
    rows = [fg._perturbed(cams, gravs, scale(i)) for i in range(N)]
    return torch.stack([r[0] for r in rows], 1).contiguous(), torch.stack([r[1] for r in rows], 1).contiguous()


def make_mask(case, seed=5):
    """A mask (B, H, W) of zeros and ones with a few fractional weights (0.5 and 0.3: the product with a confidence then
    rounds)."""
    _, B, H, W, _, _ = case
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(B, H, W, generator=g)
    m = (r > 0.35).float()
    m[(r > 0.9)] = 0.5
    m[(r > 0.95)] = 0.3
    return m


def weights_of(data, mask, B, H, W, dtype):
    """(c_up, c_lat): confidence x mask per field in `dtype` (float32: the kernel's one rounded product)."""
    out = []
    for key in ("up_confidence", "latitude_confidence"):
        c = data[key].to(dtype) if key in data else torch.ones(B, H, W, dtype=dtype)
        out.append(c if mask is None else c * mask.to(dtype))
    return out


def first_argmax(total):
    """The first index of the largest total per row, NaN the maximum (torch.argmax's rule, stated explicitly)."""
    t = total.clone()
    key = torch.where(t.isnan(), torch.full_like(t, math.inf), t)
    both = torch.where(t.isnan(), torch.ones_like(t), torch.zeros_like(t))       # NaN ahead of +inf
    best = []
    for b in range(t.shape[0]):
        order = sorted(range(t.shape[1]), key=lambda i: (-both[b, i].item(), -key[b, i].item(), i))
        best.append(order[0])
    return torch.tensor(best)


def restate(case, hyp_c, hyp_g, data, thresholds=(1.0, 1.0), weights=(1.0, 1.0), mask=None, mutant=None):
    """A float32 CPU restatement of the kernel: {"scores" (B, N, 3) float32, "best" (B,)}.  `mutant` (CPU self-check only)
    names one deliberate error: le, nomask, radians, swapconf, dropmask, swapweights, transposed, lasttie."""
    model, B, H, W, _, off = case
    N, px = hyp_c.shape[1], fg.pixels_per_lane(W, off)
    if mutant == "transposed":                   # rows read in n B + b order
        hyp_c = hyp_c.reshape(B * N, 8).reshape(N, B, 8).transpose(0, 1)
        hyp_g = hyp_g.reshape(B * N, 3).reshape(N, B, 3).transpose(0, 1)
    d = dict(data)
    if mutant == "swapconf" and "up_confidence" in d and "latitude_confidence" in d:
        d["up_confidence"], d["latitude_confidence"] = d["latitude_confidence"], d["up_confidence"]
    w_up, w_lat = weights_of(d, None if mutant == "dropmask" else mask, B, H, W, torch.float32)
    wu, wl = weights[::-1] if mutant == "swapweights" else weights
    t32 = [torch.tensor(t, dtype=torch.float32) for t in thresholds]
    scores = torch.zeros(B, N, 3, dtype=torch.float64)
    for n in range(N):
        r = fg.restate(case, hyp_c[:, n], hyp_g[:, n], d, (), mutant if mutant in ("nomask", "radians") else None)
        for i, (e, w) in enumerate(((r["up_err"], w_up), (r["lat_err"], w_lat))):
            if e is not None:
                hit = (e <= t32[i]) if mutant == "le" else (e < t32[i])
                scores[:, n, i] = fg.block_sum(hit.float() * w, px)
    scores[..., 2] = wu * scores[..., 0] + wl * scores[..., 1]
    scores = scores.float()
    best = first_argmax(scores[..., 2])
    if mutant == "lasttie":
        best = torch.tensor([max(i for i in range(N) if scores[b, i, 2] == scores[b, best[b], 2]) for b in range(B)])
    return {"scores": scores, "best": best}


def yardstick(case, hyp_c, hyp_g, data, thresholds=(1.0, 1.0), weights=(1.0, 1.0), mask=None):
    """The float64 intervals of one case: a dict of lo, hi (B, N, 3) (up, lat, total; the summation term included), csum
    (B, 2) = sum |c| per field, width (B, N, 2) = (hi - lo) / csum of the two fields, admissible (B, N) bool, ks."""
    model, B, H, W, _, off = case
    N, px = hyp_c.shape[1], fg.pixels_per_lane(W, off)
    c64 = weights_of(data, mask, B, H, W, torch.float64)
    c32 = weights_of(data, mask, B, H, W, torch.float32)
    t32 = [torch.tensor(t, dtype=torch.float32) for t in thresholds]
    has = ("up_field" in data, "latitude_field" in data)
    csum = torch.stack([c.abs().sum((1, 2)) for c in c64], -1)
    lo, hi = torch.zeros(B, N, 3, dtype=torch.float64), torch.zeros(B, N, 3, dtype=torch.float64)
    ks = 1.0
    for n in range(N):
        y = fg.yardstick(case, hyp_c[:, n], hyp_g[:, n], data, thresholds=(float(t32[0]),))
        r = fg.restate(case, hyp_c[:, n], hyp_g[:, n], data, ())
        for i, (e, g, e32) in enumerate(((y["e_up"], y["g_up"], r["up_err"]), (y["e_lat"], y["g_lat"], r["lat_err"]))):
            if not has[i]:
                continue
            t = float(t32[i])
            lo[:, n, i] = (c64[i] * (e < t - g)).sum((1, 2))
            hi[:, n, i] = (c64[i] * (e < t + g)).sum((1, 2))
            v32 = (e32 < t32[i]).float() * c32[i]
            ratio = (fg.block_sum(v32, px) - v32.double().sum((1, 2))).abs() / (K_ROUND * U * csum[:, i]).clamp(min=1e-300)
            ks = max(ks, 4 * ratio.max().item())
    width = (hi[..., :2] - lo[..., :2]) / csum[:, None, :].clamp(min=1e-300)
    for i in range(2):
        if has[i]:
            slack = (ks * K_ROUND * U * csum[:, i])[:, None]
            lo[..., i], hi[..., i] = lo[..., i] - slack, hi[..., i] + slack
    wu, wl = weights
    ends = [wu * lo[..., 0], wu * hi[..., 0]], [wl * lo[..., 1], wl * hi[..., 1]]
    t_lo = torch.minimum(*ends[0]) + torch.minimum(*ends[1])
    t_hi = torch.maximum(*ends[0]) + torch.maximum(*ends[1])
    pad = 2 * U * torch.maximum(t_lo.abs(), t_hi.abs())
    lo[..., 2], hi[..., 2] = t_lo - pad, t_hi + pad
    admissible = hi[..., 2] >= lo[..., 2].max(1, keepdim=True).values
    return {"lo": lo, "hi": hi, "csum": csum, "width": width, "admissible": admissible, "ks": ks}


def verdict(y, out):
    """How `out` ({"scores" (B, N, 3), "best" (B,)}) stands against yardstick `y`: up, lat, total -- scores outside their
    interval (a NaN counts), best_a -- images whose best is not the first argmax of the returned totals, best_b -- images
    whose best is not admissible.  All 0: pass."""
    s = out["scores"].double().cpu()
    best = out["best"].cpu().long()
    assert s.shape == y["lo"].shape and best.shape == (s.shape[0],), (s.shape, best.shape)
    outside = ~((s >= y["lo"]) & (s <= y["hi"]))
    v = {k: int(outside[..., i].sum()) for i, k in enumerate(("up", "lat", "total"))}
    v["best_a"] = int((best != first_argmax(out["scores"].float().cpu()[..., 2])).sum())
    inside = (best >= 0) & (best < s.shape[1])
    v["best_b"] = int((~inside).sum()) + int((~y["admissible"][torch.arange(s.shape[0])[inside], best[inside]]).sum())
    return v


def passes(v):
    return all(n == 0 for n in v.values())


def decisive(y):
    """Whether at least one image's admissible set is one index, or indices that tie in the yardstick itself: the identical
    pair, or hypotheses that hit exactly the same pixels (equal float64 intervals of both fields -- in simple_divisional 2 x 30
    x 200, scales 0.1 and 0.4 both hit the first two column bands of image 0 and nothing else).  Among those (a) alone
    decides, by the lower index."""
    for b, row in enumerate(y["admissible"]):
        idx = row.nonzero().flatten().tolist()
        if all(torch.equal(y["lo"][b, i], y["lo"][b, idx[0]]) and torch.equal(y["hi"][b, i], y["hi"][b, idx[0]]) for i in idx):
            return True
    return False
