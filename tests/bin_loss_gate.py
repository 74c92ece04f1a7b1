"""Inputs, float64 yardstick and gates of gclm_bin_loss / gclm_bin_loss_grad (losses.perspective_bin_loss on the HIP path),
shared by the CPU tests (test_bin_loss_host.py) and the GPU tests (test_bin_loss.py).  A plain module, like the other *_gate.py.

Inputs of a case (model, H, W, Ku, Kl, dtype, conf, heads, seed, planted): B = 3 images; roll +-0.6 rad, pitch +-0.5 rad, vfov
0.5 - 1.4 rad, k1 +-0.15, k2 +-0.05 from a seeded CPU generator, rounded to float32 as the kernels read them; logits 3 randn
plus up to 4 at the true bin, rounded to `dtype`; confidences in [0.1, 1).  `planted` makes one channel of each head -inf
everywhere (the last one that is no pixel's target: a target of -inf has an infinite loss) and gives one pixel of every image logits of +-30: the rescale step meets an infinite and a far maximum.

Yardstick: the definition in float64 on the CPU, on the same logits widened -- the fields of perspective_gate.fields(float64),
the encoders of perspective_encoding (the latitude's edges cast to float64), logsumexp - z_t, the weighting of
losses.field_loss, torch.argmax.

Targets.  A pixel is UNDECIDED for a head when its float64 direction (latitude) lies within EPS_DEG = 1e-3 degrees of a bin
boundary; there the neighbouring bin is accepted as well (cyclically for up).  1e-3 degrees is 40 - 160 x the float32 field
error (<= 4.3e-7 rad).  The tests hold the undecided share to 1 % of an image per head.

Loss and gradients are gated against float64 evaluated WITH THE KERNEL'S OWN BINS, in units: the error of the float32 torch
composition (CPU) on the same tensors and bins, but at least
    loss       2^-23 mean(|lse| + |z_t|) / |loss|           (relative to the image's loss)
    gradient   2^-24 max |z - lse| over the finite entries  (per image, max-norm of the error over max-norm of the gradient)
and the gate is GATE = 4 units (the project's convention).  16-bit gradients are held to one ulp of the dtype at
the float64 gradient, on top of that float32 gate: the float32 value the kernel rounds carries the float32 error, which at
k = t is absolute (p - 1 cancels), so next to a target whose p is 1 - 1e-5 no float32 evaluation is within a 16-bit ulp."""
import functools
import math

import torch

import perspective_gate as pg
from geocalib_amd import losses, perspective_encoding as pe

B = 3
EPS_DEG = 1e-3
GATE = 4.0
WEIGHTS = {"up": 0.75, "latitude": 2.0}          # up_loss_weight, latitude_loss_weight of every gated call
GOUT = (0.5, -2.0, 1.25)                         # grad_output of image b
HEADS = ("up", "latitude")
ULP_BITS = {torch.float32: 23, torch.float16: 10, torch.bfloat16: 7}
MIN_EXP = {torch.float32: -126, torch.float16: -14, torch.bfloat16: -126}

P, SR, R, SD = "pinhole", "simple_radial", "radial", "simple_divisional"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
# (model, H, W, Ku, Kl, dtype, conf, heads, seed, planted)
#   13 x 19: scalar path, ragged tile;  24 x 40: vector path for both widths;  67 x 65: 34 tiles, two records in a chain, a second
#   tile column one pixel wide;  5 x 264 / 3 x 520: a second tile column of 8 pixels at 4 / at 8 pixels per lane (and the other
#   width's path beside it).  The thin shapes run the pinhole model: at |u| ~ 100 a distorted model's fields say nothing.
#   Counts: the groups of 8 channels leave remainders 1, 4 (73, 180), 1, 0 (9, 8), only a remainder (5, 4), the smallest (2, 1).
CASES = [
    (P, 13, 19, 73, 180, F32, True, "both", 13, False),
    (SR, 24, 40, 73, 180, F32, True, "both", 12, False),
    (R, 67, 65, 73, 180, F32, False, "both", 13, False),
    (P, 5, 264, 73, 180, F32, True, "both", 11, False),
    (P, 3, 520, 73, 180, BF16, True, "both", 12, False),
    (P, 3, 520, 9, 8, F16, False, "both", 13, False),
    (R, 24, 40, 9, 8, BF16, True, "both", 11, False),
    (SD, 13, 19, 5, 4, F16, True, "both", 12, False),
    (P, 24, 40, 2, 1, F32, True, "both", 13, False),
    (R, 24, 40, 9, 8, F32, False, "both", 12, True),
    (SR, 67, 65, 2, 1, BF16, True, "both", 11, False),
    (SD, 24, 40, 73, 180, F16, True, "both", 13, False),
    (SR, 13, 19, 73, 180, F32, True, "up", 12, False),
    (R, 24, 40, 73, 180, BF16, False, "latitude", 11, False),
    (P, 5, 264, 9, 8, BF16, True, "both", 13, False),
    (P, 3, 520, 5, 4, F32, True, "both", 12, False),
]


def case_id(case):
    model, H, W, Ku, Kl, dtype, conf, heads, seed, planted = case
    return f"{model}-{H}x{W}-{Ku}+{Kl}-{str(dtype).split('.')[-1]}-{'conf' if conf else 'noconf'}-{heads}-s{seed}{'-planted' if planted else ''}"


def heads_of(case):
    return HEADS if case[7] == "both" else (case[7],)


def calibration(model, H, W, seed):
    """(cams (B, 8), gravs (B, 3)) float32: rows [w, h, f, f, w / 2, h / 2, k1, k2] and Gravity.from_rp's vector."""
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(B, generator=g, dtype=torch.float64)  # noqa: E731
    roll, pitch, vfov, k1, k2 = u(-0.6, 0.6), u(-0.5, 0.5), u(0.5, 1.4), u(-0.15, 0.15), u(-0.05, 0.05)
    # a level camera puts the horizon on a pixel row, a whole row of undecided latitudes
    roll = torch.where(roll.abs() < 0.05, roll + 0.1, roll)
    f = H / 2 / torch.tan(vfov / 2)
    zero, one = torch.zeros(B, dtype=torch.float64), torch.ones(B, dtype=torch.float64)
    k1 = zero if model == "pinhole" else k1
    k2 = k2 if model == "radial" else zero
    cams = torch.stack([W * one, H * one, f, f, W / 2 * one, H / 2 * one, k1, k2], -1).to(torch.float32)
    h = -torch.cos(pitch)
    gravs = torch.stack([torch.sin(roll) * h, torch.cos(roll) * h, torch.sin(pitch)], -1).to(torch.float32)
    return cams, gravs


def up_bins_of_degrees(degrees, Ku):
    """encode_up_bin's rule on degrees in [0, 360): round half to even over the bin width, a full turn wraps to bin 0."""
    bins = torch.round((degrees % 360) / (360 / (Ku - 1))).long()
    return torch.where(bins == Ku - 1, torch.zeros_like(bins), bins)


def lat_bins_of_degrees(degrees, Kl):
    return torch.bucketize(degrees, pe._latitude_edges(Kl)[1:].to(degrees.dtype), right=False).long()


def targets_of_fields(fields, Ku, Kl):
    """{head: (bins (B, H, W) long, also-accepted bins below, above, undecided (B, H, W) bool)} of perspective_gate.fields."""
    up, lat = fields["up"].double(), fields["lat"].double()
    deg = torch.atan2(up[..., 1], up[..., 0]) / math.pi * 180 + 180
    out = {}
    if Ku:
        t = torch.stack([pe.encode_up_bin(u.permute(2, 0, 1), Ku) for u in up])
        lo, hi = up_bins_of_degrees(deg - EPS_DEG, Ku), up_bins_of_degrees(deg + EPS_DEG, Ku)
        out["up"] = (t, lo, hi, lo != hi)
    if Kl:
        ldeg = lat / math.pi * 180
        t = lat_bins_of_degrees(ldeg, Kl)
        lo, hi = lat_bins_of_degrees(ldeg - EPS_DEG, Kl), lat_bins_of_degrees(ldeg + EPS_DEG, Kl)
        out["latitude"] = (t, lo, hi, lo != hi)
    return out


@functools.lru_cache(maxsize=None)
def inputs(case):
    """What every evaluation of a case shares, computed once and left unchanged: cams, gravs, the float64 targets with their
    undecided masks, `pred` (CPU tensors: logits in the case's dtype, float32 confidences)."""
    model, H, W, Ku, Kl, dtype, conf, heads, seed, planted = case
    cams, gravs = calibration(model, H, W, seed)
    counts = {"up": Ku if heads in ("both", "up") else 0, "latitude": Kl if heads in ("both", "latitude") else 0}
    targets = targets_of_fields(pg.fields(model, cams, gravs, H, W), counts["up"], counts["latitude"])
    g = torch.Generator().manual_seed(1000 + seed)
    pred = {}
    for n in heads_of(case):
        K, t = counts[n], targets[n][0]
        z = 3 * torch.randn(B, K, H, W, generator=g)
        z.scatter_add_(1, t[:, None], 4 * torch.rand(B, 1, H, W, generator=g))
        if planted:
            free = [k for k in range(K) if not any((b == k).any() for b in targets[n][:3])]
            assert free, "the planted case needs a channel that is no pixel's target"
            y, x = H // 2, W // 3
            z[:, :, y, x] = 30.0 * (1 - 2 * (torch.arange(K) % 2).float())[None]
            z[:, free[-1]] = -math.inf
        pred[f"{n}_logits"] = z.to(dtype).contiguous()
        if conf:
            pred[f"{n}_confidence"] = 0.1 + 0.9 * torch.rand(B, H, W, generator=g)
    return {"cams": cams, "gravs": gravs, "targets": targets, "pred": pred, "counts": counts}


def bins_verdict(case, head, d_bins):
    """(wrong, undecided share): how many pixels of `d_bins` (B, H, W) hold neither the float64 bin nor, at an undecided pixel,
    one of its neighbours; and the worst share of undecided pixels of an image."""
    t, lo, hi, und = inputs(case)["targets"][head]
    d = d_bins.long().cpu()
    ok = (d == t) | (und & ((d == lo) | (d == hi)))
    return int((~ok).sum()), und.double().mean((1, 2)).max().item()


def composition(case, bins, dtype):
    """The definition in `dtype` on the CPU with the target bins given ({head: (B, H, W)}): {"loss" {head: (B,)} weighted,
    "grad" {head: (B, K, H, W)} of sum_b GOUT[b] sum_heads loss, "lse", "zt" {head: (B, H, W)}, "hits" {head: (B,)}}."""
    pred = inputs(case)["pred"]
    out = {"loss": {}, "grad": {}, "lse": {}, "zt": {}, "hits": {}}
    gout = torch.tensor(GOUT, dtype=dtype)
    for n in heads_of(case):
        z = pred[f"{n}_logits"].detach().clone().to(dtype).requires_grad_(True)      # (never the shared tensor itself)
        c = pred.get(f"{n}_confidence")
        t = bins[n].long()
        loss = losses.bin_loss(z, t, None if c is None else c.to(dtype)) * WEIGHTS[n]
        (gout * loss).sum().backward()
        zd = z.detach()
        out["loss"][n], out["grad"][n] = loss.detach(), z.grad
        out["lse"][n], out["zt"][n] = torch.logsumexp(zd, 1), zd.gather(1, t[:, None])[:, 0]
        out["hits"][n] = (zd.argmax(1) == t).sum((1, 2))
    return out


def _finite_max(x):
    return torch.where(torch.isfinite(x), x, torch.zeros_like(x)).flatten(1).max(1).values


def units(case, bins):
    """(y64, {"loss" {head: (B,)}, "grad" {head: (B,)}}): the float64 yardstick with these bins and the unit of each gate, as
    absolute errors: of the image's loss, and of the max-norm of the image's gradient."""
    y64, y32 = composition(case, bins, torch.float64), composition(case, bins, torch.float32)
    pred = inputs(case)["pred"]
    u = {"loss": {}, "grad": {}}
    for n in heads_of(case):
        L, G = y64["loss"][n], y64["grad"][n]
        lse, zt = y64["lse"][n], y64["zt"][n]
        floor = 2.0 ** -23 * (lse.abs() + zt.abs()).mean((1, 2)) * WEIGHTS[n]
        u["loss"][n] = torch.maximum((y32["loss"][n].double() - L).abs(), floor)
        z = pred[f"{n}_logits"].double()
        floor = 2.0 ** -24 * _finite_max((z - lse[:, None]).abs()) * G.abs().flatten(1).max(1).values
        u["grad"][n] = torch.maximum((y32["grad"][n].double() - G).abs().flatten(1).max(1).values, floor)
    return y64, u


def ulp_of(x, dtype):
    """ulp of |x| (float64) in `dtype`."""
    e = torch.floor(torch.log2(x.abs().clamp(min=2.0 ** MIN_EXP[dtype]))).clamp(min=MIN_EXP[dtype])
    return torch.exp2(e - ULP_BITS[dtype])


def _ratio(d, gate):
    """|difference| / gate; a difference of exactly 0 passes any gate (a gate of 0 asks for exactly 0); a NaN or inf fails."""
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, math.inf))
    return torch.where(d == 0, torch.zeros_like(d), d / gate.clamp(min=1e-300))


def verdict(case, y64, u, head, loss, grad):
    """Ratios to the units of one head's device results: loss (B,) weighted and grad (B, K, H, W) in the logits' dtype.
    {"loss": worst |L - L64| in units, "grad": worst max-norm error in units (float32 gradients), "grad_ulp": for 16-bit
    gradients the worst |g - G64| over (one ulp of the dtype at G64 + the float32 gate), else 0}.  Pass: <= GATE, <= GATE, <= 1."""
    dtype = case[5]
    L, G = y64["loss"][head], y64["grad"][head]
    v = {"loss": _ratio((loss.double().cpu() - L).abs(), u["loss"][head]).max().item(), "grad": 0.0, "grad_ulp": 0.0}
    g = grad.double().cpu()
    if dtype == torch.float32:
        v["grad"] = _ratio((g - G).abs().flatten(1).max(1).values, u["grad"][head]).max().item()
    else:
        # the float32 value that is rounded carries the float32 gate's error (absolute at k = t, where p - 1 cancels); the
        # rounding adds at most half an ulp of the dtype
        v["grad_ulp"] = _ratio((g - G).abs(), ulp_of(G, dtype) + (GATE * u["grad"][head])[:, None, None, None]).max().item()
    return v


def passes(v):
    return v["loss"] <= GATE and v["grad"] <= GATE and v["grad_ulp"] <= 1
