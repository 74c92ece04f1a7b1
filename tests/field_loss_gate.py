"""Float64 yardstick and gates of gclm_field_loss / gclm_field_loss_grad (losses.perspective_field_loss on the HIP path), shared
by the CPU self-check (test_field_loss_abi.py) and the GPU parity test (test_field_loss.py).  Built on perspective_gate.py
and on field_error_gate.py's cases, inputs and summation order.

Yardstick: the formulas of include/gclm.h in float64 on the float32 inputs -- the target fields from perspective_gate.fields(...,
float64), r = p - t, the per-pixel loss l of the loss type, per image L = weight sum(l c) / sum c (or weight sum l / (H W)
without a confidence) -- and the gradient of sum_b grad_output[b] L_b with respect to p from torch autograd in float64.

Gates.  With b_c perspective_gate's bound on component c of the target (its kappa included) and e_c = b_c + ulp(p_c) the
bound on the float32 residual, to first order (second-order terms kept where the first vanishes at r = 0):
    l:        sum_c (|dl/dr_c| e_c + h e_c^2 / 2) + 8 U |l|         h the bound on the second derivative: l1 0, l2 2, dot 2,
                                                                    cauchy 1, huber 1;  dot: dl/dt_c = 2 t_c - p_c
    dl/dp_c:  D_c + 4 U |dl/dp_c|,  D_c = 0 (l1), 2 e_c (l2), e_c (dot: -t_c; huber), 1.25 sum_c' e_c' (cauchy)
each scaled by a kappa DERIVED per case, field and loss type: 4 x the worst ratio of a float32 CPU restatement of the kernel
(`restate`) against the yardstick to that base, at least 1.
    L:        weight (sum(gate_l w) + (25 ks + 2) U sum(|l| w)) + 2 U |L|,  w = c / sum c  (or 12 ks and w = 1 / (H W)), ks derived
              as field_error_gate derives it: 4 x the worst ratio of the block-then-float64 sum of the same float32 values against
              their float64 sum to 12 U sum |.|, at least 1 (numerator, denominator and their product, as field_error_gate).
    gradient: |scale| c kappa (D_c + 4 U |dl/dp_c|) + |G| (rel + 4 U),  scale = grad_output weight / denominator in float64,
              rel = (12 ks + 8) U with a confidence (the float32 denominator and two float32 operations), 4 U without.
              A gate of 0 (grad_output = 0) asks for exactly 0.
The l1 derivative is a sign: a component is UNDECIDED where |r64_c| <= e_c; there the device value must be one of
{-1, 0, 1} scale c (to the relative part of the gate), everywhere else the sign is exact.  `yardstick` reports the share of
undecided components per image; the tests hold it to 1 % except on the designated exact-target image (the last)."""
import functools
import math

import torch

import field_error_gate as fg
import perspective_gate as pg

U = pg.U
LOSS_IDS = {"l1": 0, "l2": 1, "dot": 2, "cauchy": 3, "huber": 4}
CAUCHY_C2 = 0.007 ** 2
HUBER_DELTA = math.pi / 180
WEIGHTS = (0.75, 2.0)                   # up_loss_weight, latitude_loss_weight of every gated call
# grad_output of image b: entry b % 3.  The last image of a case is the exact-target one, whose gradients say little: in a
# batch of two the first image carries a non-zero grad_output for both fields, in a batch of three the first two do for up
# and images 0 and 2 for the latitude
GOUT_UP, GOUT_LAT = (0.5, -2.0, 0.0), (1.25, 0.0, -0.75)

# field_error_gate's shapes and 4-byte-offset variants for all four models, one width that takes two pixels per lane, and
# the gravity extremes
PX2 = [(m, 2, 11, 70, "random", False) for m in pg.MODELS]
CASES = fg.CASES + PX2 + fg.EXTREMES
case_id = fg.case_id
SUBSETS = ("all", "noconf", "up", "lat")


def loss_types(case):
    """The (up, latitude) loss types a case runs with: l1 and huber everywhere, the others on each model's first shape."""
    extra = [("l2", "l2"), ("dot", "cauchy"), ("cauchy", "l1")] if case[1:4] == fg.SHAPES[0] and not case[5] else []
    return [("l1", "l1"), ("huber", "huber")] + extra


def grad_output(B):
    """(B, 2) float32: a non-uniform grad_output per image and key, with zeros."""
    return torch.tensor([[GOUT_UP[b % 3], GOUT_LAT[b % 3]] for b in range(B)], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def target(case):
    """What every evaluation of a case shares, computed once and left unchanged: cams, gravs, data (field_error_gate.make_case),
    the float64 target with perspective_gate's bounds and the float32 restatement of the target, as (B, C, H, W) planes."""
    model, B, H, W, _, _ = case
    cams, gravs, data = fg.make_case(case)
    ref = pg.fields(model, cams, gravs, H, W)
    b_up, _, b_lat = pg.gates(ref, *pg.kappas(model, cams, gravs, H, W, ref=ref))
    f32 = pg.fields(model, cams, gravs, H, W, torch.float32)
    planes = lambda t: t.permute(0, 3, 1, 2).contiguous()  # noqa: E731
    return {"cams": cams, "gravs": gravs, "data": data,
            "t64": {"up": planes(ref["up"]), "lat": ref["lat"][:, None]}, "b": {"up": planes(b_up), "lat": b_lat[:, None]},
            "t32": {"up": planes(f32["up"]), "lat": f32["lat"][:, None], "q": planes(f32["q"])}}


def pixel_loss(kind, p, t, mutant=None):
    """(l (B, H, W), dl/dp (B, C, H, W)) of the loss type in the dtype of p and t, by the formulas of include/gclm.h."""
    r = p - t
    s = (r * r).sum(1)
    if kind == "l1":
        sign = torch.sign(r)
        return r.abs().sum(1), -sign if mutant == "l1flip" else sign
    if kind == "l2":
        return s, 2 * r
    if kind == "dot":
        return 1 - ((p if mutant == "dot_pt" else r) * t).sum(1), -t
    if kind == "cauchy":
        half = 1.0 if mutant == "cauchy_nohalf" else 0.5
        return half * CAUCHY_C2 * torch.log1p(s / CAUCHY_C2), 2 * half * r / (1 + s / CAUCHY_C2)[:, None]
    delta = 1.0 if mutant == "huber1" else HUBER_DELTA
    a = r.abs()
    return torch.where(a < delta, 0.5 * r * r, delta * (a - 0.5 * delta)).sum(1), r.clamp(-delta, delta)


def _fields_of(data):
    return [(i, k, f"{n}_field", f"{n}_confidence") for i, (k, n) in enumerate((("up", "up"), ("lat", "latitude"))) if f"{n}_field" in data]


def restate(case, which, types, mutant=None, data=None, gout=None):
    """A float32 CPU restatement of the two kernels and of the wrapper's scale: {"loss" (B, 2) weighted, NaN for an absent
    field, "den" (B, 2), "g_up", "g_lat", "l_up", "l_lat" (the per-pixel losses, for the kappas)}.  `mutant` (CPU self-check
    only) names one deliberate error: plainmean, grad_hw, l1flip, huber1, cauchy_nohalf, dot_pt, unnorm, scale0, upscale_lat,
    lastcol."""
    model, B, H, W, _, off = case
    T = target(case)
    data, px = fg.subset(T["data"] if data is None else data, which), fg.pixels_per_lane(W, off)
    gout, f32 = grad_output(B) if gout is None else gout, torch.float32
    out = {"loss": torch.full((B, 2), math.nan), "den": torch.full((B, 2), math.nan)}
    keep = torch.ones(W, dtype=torch.bool)
    if mutant == "lastcol":
        ntx = -(-W // (64 * px))
        assert ntx > 1, "the mutant needs more than one tile column"
        keep = torch.arange(W) < 64 * px * (ntx - 1)
    scales, parts = torch.zeros(B, 2), {}
    for i, k, fkey, ckey in _fields_of(data):
        p, t = data[fkey], T["t32"]["q" if (mutant == "unnorm" and k == "up") else k]
        l, d = pixel_loss(types[i], p, t, mutant)
        c = data.get(ckey)
        lw = (l if c is None else l * c) * keep
        num = fg.block_sum(lw, px)
        den = torch.full((B,), float(H * W), dtype=torch.float64) if c is None else fg.block_sum(c * keep, px)
        loss_den = torch.full((B,), float(H * W), dtype=torch.float64) if mutant == "plainmean" else den
        if mutant == "plainmean":
            num = fg.block_sum(l * keep, px)
        out["loss"][:, i] = (num / loss_den).to(f32) * torch.tensor(WEIGHTS[i], dtype=f32)
        out["den"][:, i] = den.to(f32)
        gden = torch.full((B,), float(H * W)) if mutant == "grad_hw" else out["den"][:, i]
        scales[:, i] = gout[:, i] * torch.tensor(WEIGHTS[i], dtype=f32) / gden
        parts[k] = (l, d, c)
    if mutant == "scale0":
        scales = scales[:1].expand(B, 2)
    if mutant == "upscale_lat":
        scales = scales[:, :1].expand(B, 2)
    for i, k, _, _ in _fields_of(data):
        l, d, c = parts[k]
        g = scales[:, i, None, None, None] * d
        out[f"g_{k}"] = (g if c is None else g * c[:, None]) * keep
        out[f"l_{k}"] = l
    return out


def _kappa_sum(v32, px):
    return max(1.0, 4 * ((fg.block_sum(v32, px) - v32.double().sum((1, 2))).abs()
                         / (12 * U * v32.double().abs().sum((1, 2))).clamp(min=1e-300)).max().item())


def _ratio(d, gate):
    """|difference| / gate; a difference of exactly 0 passes any gate (a gate of 0 asks for exactly 0); a NaN or inf fails."""
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, math.inf))
    return torch.where(d == 0, torch.zeros_like(d), d / gate.clamp(min=1e-300))


SECOND = {"l1": 0.0, "l2": 2.0, "dot": 2.0, "cauchy": 1.0, "huber": 1.0}


def yardstick(case, which, types, data=None, gout=None):
    """The float64 losses and gradients of one case, subset and pair of loss types, with their gates: "loss", "g_loss", "den",
    "g_den" (B, 2) (NaN for an absent field), and per field k in (up, lat): "G_k" (B, C, H, W), "gate_k", "und_k" (bool: the
    undecided l1 components), "step_k" (|scale| c: what an undecided component may be +-1 or 0 times), "rel_k" (the relative
    part of its gate) and "undecided_k" (B,) (their share per image)."""
    model, B, H, W, _, off = case
    T = target(case)
    data, px = fg.subset(T["data"] if data is None else data, which), fg.pixels_per_lane(W, off)
    r32 = restate(case, which, types, data=data, gout=gout)
    gout = (grad_output(B) if gout is None else gout).double()
    nan = lambda: torch.full((B, 2), math.nan, dtype=torch.float64)  # noqa: E731
    y = {"loss": nan(), "g_loss": nan(), "den": nan(), "g_den": nan()}
    for i, k, fkey, ckey in _fields_of(data):
        kind, weight = types[i], WEIGHTS[i]
        p = data[fkey].double().requires_grad_(True)
        t, b = T["t64"][k], T["b"][k]
        c32 = data.get(ckey)
        c = None if c32 is None else c32.double()
        l, d = pixel_loss(kind, p, t)
        den = torch.full((B,), float(H * W), dtype=torch.float64) if c is None else c.sum((1, 2))
        L = ((l if c is None else l * c).sum((1, 2)) / den) * weight
        (gout[:, i] * L).sum().backward()
        G, l, d, p = p.grad, l.detach(), d.detach(), p.detach()
        # ---- per pixel
        e = b + pg.ulp32(p)
        r = p - t
        first = {"l1": torch.ones_like(r), "l2": 2 * r.abs(), "dot": (2 * t - p).abs(), "cauchy": d.abs(), "huber": d.abs()}[kind]
        base_l = (first * e + SECOND[kind] * e * e / 2).sum(1) + 8 * U * l.abs()
        k_l = max(1.0, 4 * _ratio((r32[f"l_{k}"].double() - l).abs(), base_l).max().item())
        D = {"l1": torch.zeros_like(e), "l2": 2 * e, "dot": e, "huber": e, "cauchy": 1.25 * e.sum(1, keepdim=True).expand_as(e)}[kind]
        und = (r.abs() <= e) if kind == "l1" else torch.zeros_like(r, dtype=torch.bool)
        # ---- per image
        w = (torch.ones_like(l) if c is None else c) / den[:, None, None]
        ks = _kappa_sum(r32[f"l_{k}"], px) if c is None else max(_kappa_sum(r32[f"l_{k}"] * c32, px), _kappa_sum(c32, px))
        y["loss"][:, i] = L.detach()
        y["g_loss"][:, i] = weight * ((k_l * base_l * w).sum((1, 2)) + ((12 if c is None else 25) * ks + 2) * U * (l.abs() * w).sum((1, 2))) \
            + 2 * U * L.detach().abs()
        y["den"][:, i] = den
        y["g_den"][:, i] = 0.0 if c is None else (12 * ks + 2) * U * den
        # ---- the gradient
        rel = 4 * U if c is None else (12 * ks + 8) * U
        step = (gout[:, i] * weight / den).abs()[:, None, None, None] * (torch.ones_like(r) if c is None else c[:, None].expand_as(r))
        base_g = step * (D + 4 * U * d.abs()) + G.abs() * (rel + 4 * U)
        k_g = max(1.0, 4 * _ratio((r32[f"g_{k}"].double() - G).abs() * ~und, base_g).max().item())
        y.update({f"G_{k}": G, f"gate_{k}": step * k_g * (D + 4 * U * d.abs()) + G.abs() * (rel + 4 * U), f"und_{k}": und,
                  f"step_{k}": step, f"rel_{k}": rel + 4 * U, f"undecided_{k}": und.double().mean((1, 2, 3)),
                  f"kappa_l_{k}": k_l, f"kappa_g_{k}": k_g, f"kappa_s_{k}": ks})
    return y


def verdict(y, out):
    """Worst ratios of `out` ({"loss" (B, 2) weighted, optional "den" (B, 2), "g_up", "g_lat"}) to the gates of yardstick `y`:
    loss, den, g_up, g_lat, and nan (entries whose NaN-ness differs from the yardstick's).  All <= 1 and nan == 0: pass.
    A gradient plane the yardstick has and `out` lacks counts as inf."""
    v = {"loss": 0.0, "den": 0.0, "g_up": 0.0, "g_lat": 0.0, "nan": 0}
    for key, gate in (("loss", "g_loss"), ("den", "g_den")):
        if out.get(key) is None:
            continue
        s = out[key].double().cpu()
        assert s.shape == y[key].shape, (s.shape, y[key].shape)
        v["nan"] += int((s.isnan() != y[key].isnan()).sum())
        both = ~s.isnan() & ~y[key].isnan()
        if both.any():
            v[key] = _ratio((s - y[key]).abs(), y[gate])[both].max().item()
    for k in ("up", "lat"):
        if f"G_{k}" not in y:
            assert out.get(f"g_{k}") is None, f"a gradient for the absent field {k}"
            continue
        if out.get(f"g_{k}") is None:
            v[f"g_{k}"] = math.inf
            continue
        g = out[f"g_{k}"].double().cpu().reshape(y[f"G_{k}"].shape)
        ratio = _ratio((g - y[f"G_{k}"]).abs(), y[f"gate_{k}"])
        und, step = y[f"und_{k}"], y[f"step_{k}"]
        if und.any():                 # an undecided sign: -1, 0 or 1 times |scale| c
            near = torch.stack([_ratio((g - s * step).abs(), step * y[f"rel_{k}"]) for s in (-1.0, 0.0, 1.0)]).min(0).values
            ratio = torch.where(und, near, ratio)
        v[f"g_{k}"] = ratio.max().item()
    return v


def passes(v):
    return v["loss"] <= 1 and v["den"] <= 1 and v["g_up"] <= 1 and v["g_lat"] <= 1 and v["nan"] == 0
