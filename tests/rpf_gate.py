"""Float64 yardstick and gate of the three-pixel minimal solver (gclm_rpf_hypotheses, ransac.solve_rpf), shared by the CPU
self-check (test_rpf_solver_abi.py) and the GPU tests (test_rpf_solver.py).  A plain module, like the other *_gate.py files.

The solver's definition (include/gclm.h) is restated here, once, for any dtype: `solve` in float64 from the sampled float32
values is the yardstick; in float32 with a `mutant` it is a deliberately wrong solver the gate must reject.

Forward agreement per row is not a usable gate: near-parallel up lines and a2 = L^2 R S - D^2 cancel, and a float32 solver
then differs from float64 by far more than any fixed number of ulps on a fraction of a percent of the rows.  The gate is
BACKWARD, on every row the solver under test calls valid, evaluated in float64 at the (f, g) it returned:
    | |g| - 1 | <= 4 float32 ulps of 1;   f inside the focal range;   the camera row is {W, H, f, f, W / 2, H / 2, 0, 0}
    the up direction (g_x - g_z u, g_y - g_z v) at pixels 0 and 1 is within ANGLE_DEG of the sampled one, same sense
    |asin(sin latitude of (f, g) at pixel 2) - sampled latitude| <= ANGLE_DEG   (not with a prior focal: nothing was fitted)
and an invalid row is NaN throughout.  Rows over ANGLE_DEG are capped at OVER_CAP of the valid rows of an image (a minimal
solver fits its three pixels exactly, so what is left is float32 conditioning: 0.01 degrees is 1.7e-4 rad, a thousand
float32 ulps; noise can also turn the two up vectors against each other, so that no gravity has both senses right).
Validity: rows valid for one of (solver, float64 yardstick) and not the other are capped at VALIDITY_CAP of an image's rows.
Both caps are per image, the strictest reading of "per case"."""
import math

import torch

ANGLE_DEG = 0.01
OVER_CAP = 0.02
VALIDITY_CAP = 0.005
NORM_ULPS = 4 * 2.0 ** -23
TAN_MAX, TAN_MIN = 3.7320504, 0.043660942     # the float32 constants of the LM's focal clamp (csrc/gclm_device.h)
SALT = 0x5250465F44524157                     # GCLM_RPF_DRAW_SALT
M64 = (1 << 64) - 1

# (roll, pitch) of section 1 of DESIGN 3.11, at vfov 60
POSES = ((10, 20), (10, -20), (-30, -35), (0, 0), (40, 40), (0, 15), (25, 0))
MUTANTS = ("divide_vz", "swap_pp", "sign_from_vz", "keep_spurious", "no_range", "textbook")


def focal_range(H):
    h = torch.tensor(H, dtype=torch.float32) * 0.5
    return float(h / torch.tensor(TAN_MAX, dtype=torch.float32)), float(h / torch.tensor(TAN_MIN, dtype=torch.float32))


def truth(roll, pitch, vfov, H):
    """(f, g) of a pose in degrees: g = (-sin r cos p, -cos r cos p, sin p)."""
    r, p = math.radians(roll), math.radians(pitch)
    return H / 2 / math.tan(math.radians(vfov) / 2), (-math.sin(r) * math.cos(p), -math.cos(r) * math.cos(p), math.sin(p))


def render(poses, H, W, noise=0.0, seed=0):
    """Perspective fields of pinhole cameras, rendered here in float64 and rounded: ({"up_field" (B, 2, H, W),
    "latitude_field" (B, 1, H, W)} float32, f (B,), g (B, 3) float64).  `poses`: (roll, pitch, vfov) in degrees.  Noise is
    Gaussian on both fields, the up field renormalised, as the package's synthetic generator has it."""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    ups, lats, fs, gs = [], [], [], []
    gen = torch.Generator().manual_seed(seed)
    for roll, pitch, vfov in poses:
        f, (a, b, c) = truth(roll, pitch, vfov, H)
        u, v = (xs - W / 2) / f, (ys - H / 2) / f
        up = torch.stack([a - c * u, b - c * v])
        up = up / up.norm(dim=0, keepdim=True)
        lat = torch.asin((a * u + b * v + c) / torch.sqrt(u * u + v * v + 1))
        if noise:
            up = up + noise * torch.randn(up.shape, generator=gen, dtype=torch.float64)
            up = up / up.norm(dim=0, keepdim=True)
            lat = (lat + noise * torch.randn(lat.shape, generator=gen, dtype=torch.float64)).clamp(-math.pi / 2 + 1e-3, math.pi / 2 - 1e-3)
        ups.append(up), lats.append(lat[None]), fs.append(f), gs.append((a, b, c))
    data = {"up_field": torch.stack(ups).float().contiguous(), "latitude_field": torch.stack(lats).float().contiguous()}
    return data, torch.tensor(fs, dtype=torch.float64), torch.tensor(gs, dtype=torch.float64)


def _mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, first_index, B, N, H, W):
    """The in-kernel draw of include/gclm.h, restated with Python integers: (B, N, 3, 2) int32 = (x, y)."""
    out = torch.empty((B, N, 3, 2), dtype=torch.int32)
    for b in range(B):
        i = (first_index + b) & M64
        base = _mix(((seed ^ SALT) & M64) ^ _mix((i * 0xD1342543DE82EF95 + 1) & M64))
        for n in range(N):
            for k in range(3):
                h = _mix((base + 4 * n + k) & M64)
                out[b, n, k, 0] = ((h >> 32) * W) >> 32
                out[b, n, k, 1] = ((h & 0xFFFFFFFF) * H) >> 32
    return out


def sampled(data, samples):
    """The float32 values the solver reads: d0, d1 (B, N, 2), latitude at pixel 2 (B, N), and the pixel coordinates."""
    up = data["up_field"].cpu()
    B, _, H, W = up.shape
    s = samples.cpu().long()
    rows = torch.arange(B)[:, None]
    o = s[..., 1] * W + s[..., 0]
    flat = up.reshape(B, 2, H * W)
    d = [torch.stack([flat[rows, 0, o[..., k]], flat[rows, 1, o[..., k]]], -1) for k in (0, 1)]
    lat = data["latitude_field"].cpu().reshape(B, H * W)[rows, o[..., 2]] if "latitude_field" in data else None
    return d[0], d[1], lat, s


def solve(data, samples, prior=None, dtype=torch.float64, mutant=None):
    """The definition, from the sampled float32 values, in `dtype`: (f (B, N, Rn), g (B, N, Rn, 3), valid (B, N, Rn)).
    `mutant` (CPU self-check only) names one deliberate error, see MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    B, _, H, W = data["up_field"].shape
    d0, d1, lat, s = sampled(data, samples)
    d0, d1 = d0.to(dtype), d1.to(dtype)
    x, y = s[..., 0].to(dtype), s[..., 1].to(dtype)
    cx, cy = (H / 2, W / 2) if mutant == "swap_pp" else (W / 2, H / 2)
    l0 = torch.stack([-d0[..., 1], d0[..., 0], x[..., 0] * d0[..., 1] - y[..., 0] * d0[..., 0]], -1)
    l1 = torch.stack([-d1[..., 1], d1[..., 0], x[..., 1] * d1[..., 1] - y[..., 1] * d1[..., 0]], -1)
    V = torch.cross(l0, l1, dim=-1)
    if mutant == "divide_vz":
        V = V / V[..., 2:]
    v = torch.stack([V[..., 0] - cx * V[..., 2], V[..., 1] - cy * V[..., 2], V[..., 2]], -1)
    v = v / v.norm(dim=-1, keepdim=True)
    vx, vy, vz = v.unbind(-1)
    U, Vp, U0, V0 = x[..., 2] - cx, y[..., 2] - cy, x[..., 0] - cx, y[..., 0] - cy
    if prior is not None:
        p = prior.cpu().to(dtype).reshape(B, 1).expand_as(vx)
        roots, L = [p * p], None
    else:
        L = torch.sin(lat).to(dtype) if dtype == torch.float32 else torch.sin(lat.to(dtype))
        L2, R, S, D = L * L, U * U + Vp * Vp, vx * vx + vy * vy, vx * U + vy * Vp
        a0, a1, a2 = (L2 - 1) * vz * vz, L2 * (R * vz * vz + S) - 2 * D * vz, L2 * R * S - D * D
        root = torch.sqrt(a1 * a1 - 4 * a0 * a2)
        if mutant == "textbook":
            roots = [-a1 / (2 * a0) + root / (2 * a0), -a1 / (2 * a0) - root / (2 * a0)]
        else:
            q = -(a1 + torch.where(a1 >= 0, root, -root)) / 2
            roots = [a2 / q, q / a0]
    fmin, fmax = focal_range(H)
    fs, gs, valids = [], [], []
    for F in roots:
        f = torch.sqrt(F)
        g = torch.stack([vx / f, vy / f, vz], -1)
        g = g / g.norm(dim=-1, keepdim=True)
        if mutant == "sign_from_vz":
            flip = g[..., 2] < 0
        else:
            flip = (g[..., 0] - g[..., 2] * (U0 / f)) * d0[..., 0] + (g[..., 1] - g[..., 2] * (V0 / f)) * d0[..., 1] < 0
        g = torch.where(flip[..., None], -g, g)
        valid = torch.isfinite(f) & torch.isfinite(g).all(-1)
        if mutant != "no_range":
            valid = valid & (f >= fmin) & (f <= fmax)
        if L is not None and mutant != "keep_spurious":
            valid = valid & (L * (g[..., 0] * (U / f) + g[..., 1] * (Vp / f) + g[..., 2]) >= 0)
        fs.append(f), gs.append(g), valids.append(valid)
    return torch.stack(fs, -1), torch.stack(gs, -2), torch.stack(valids, -1)


def as_rows(f, g, valid, H, W):
    """A solver's (f, g, valid) as the rows the kernel writes: cam (B, N Rn, 8), grav (B, N Rn, 3) float32, invalid rows NaN."""
    B, N, Rn = f.shape
    f32 = f.float()
    one = torch.ones_like(f32)
    cam = torch.stack([one * W, one * H, f32, f32, one * (W / 2), one * (H / 2), one * 0, one * 0], -1)
    nan = torch.full_like(f32, math.nan)[..., None]
    cam = torch.where(valid[..., None], cam, nan).reshape(B, N * Rn, 8)
    return cam, torch.where(valid[..., None], g.float(), nan).reshape(B, N * Rn, 3)


def _angle_deg(px, py, qx, qy):
    return torch.rad2deg(torch.atan2((px * qy - py * qx).abs(), px * qx + py * qy))


def verdict(data, samples, cam, grav, prior=None):
    """How the rows `cam` (B, N Rn, 8), `grav` (B, N Rn, 3) stand against the gate.  Per image (lists of B numbers):
    valid -- rows called valid; over -- the share of them over ANGLE_DEG in an up direction or the latitude; worst_deg -- the
    largest latitude residual of a valid row within the cap's reach (reported, not gated); mismatch -- the share of all rows
    whose validity differs from the float64 yardstick's.  Counted over all images, any of them non-zero fails: structure --
    invalid rows not NaN throughout or valid camera rows not {W, H, f, f, W / 2, H / 2, 0, 0}; norm; range."""
    B, _, H, W = data["up_field"].shape
    cam, grav = cam.detach().cpu(), grav.detach().cpu()
    d0, d1, lat, s = sampled(data, samples)
    N = s.shape[1]
    Rn = cam.shape[1] // N
    assert cam.shape == (B, N * Rn, 8) and grav.shape == (B, N * Rn, 3) and Rn == (1 if prior is not None else 2), (cam.shape, grav.shape)
    cam, grav = cam.reshape(B, N, Rn, 8), grav.reshape(B, N, Rn, 3)
    valid = ~cam[..., 2].isnan()
    nan_rows = cam.isnan().all(-1) & grav.isnan().all(-1)
    want = torch.tensor([W, H, 0, 0, W / 2, H / 2, 0, 0], dtype=torch.float32)
    shaped = (cam[..., [0, 1, 4, 5, 6, 7]] == want[[0, 1, 4, 5, 6, 7]]).all(-1) & (cam[..., 2] == cam[..., 3]) & ~grav.isnan().any(-1)
    structure = int((~torch.where(valid, shaped, nan_rows)).sum())
    f, g = cam[..., 2].double(), grav.double()
    norm = int((valid & ~((g.norm(dim=-1) - 1).abs() <= NORM_ULPS)).sum())
    fmin, fmax = focal_range(H)
    rng = int((valid & ~((f >= fmin) & (f <= fmax))).sum())
    x, y = s[..., 0].double(), s[..., 1].double()
    over = torch.zeros_like(valid)
    for k, d in ((0, d0.double()), (1, d1.double())):
        u, v = ((x[..., k] - W / 2)[..., None] / f, (y[..., k] - H / 2)[..., None] / f)
        e = _angle_deg(g[..., 0] - g[..., 2] * u, g[..., 1] - g[..., 2] * v, d[..., None, 0], d[..., None, 1])
        over |= ~(e <= ANGLE_DEG)
    worst = torch.zeros(B, dtype=torch.float64)
    if prior is None:
        u, v = ((x[..., 2] - W / 2)[..., None] / f, (y[..., 2] - H / 2)[..., None] / f)
        sl = (g[..., 0] * u + g[..., 1] * v + g[..., 2]) / torch.sqrt(u * u + v * v + 1)
        e = torch.rad2deg((torch.asin(sl.clamp(-1, 1)) - lat.double()[..., None]).abs())
        over |= ~(e <= ANGLE_DEG)
        inside = torch.where(valid & (e <= ANGLE_DEG), e, torch.zeros_like(e))
        worst = inside.reshape(B, -1).max(1).values
    over &= valid
    _, _, valid64 = solve(data, samples, prior)
    n_valid = valid.reshape(B, -1).sum(1)
    return {"valid": n_valid.tolist(), "over": (over.reshape(B, -1).sum(1) / n_valid.clamp(min=1)).tolist(), "worst_deg": worst.tolist(),
            "mismatch": ((valid != valid64).reshape(B, -1).sum(1) / (N * Rn)).tolist(), "structure": structure, "norm": norm, "range": rng}


def passes(v):
    return v["structure"] == v["norm"] == v["range"] == 0 and max(v["over"]) <= OVER_CAP and max(v["mismatch"]) <= VALIDITY_CAP


def good_rate(cam, grav, f_true, g_true, N):
    """Per image, the share of samples with a valid row within 0.5 degrees and 2 % of the truth."""
    B = cam.shape[0]
    cam, grav = cam.cpu().double().reshape(B, N, -1, 8), grav.cpu().double().reshape(B, N, -1, 3)
    ferr = (cam[..., 2] / f_true[:, None, None] - 1).abs()
    ang = torch.rad2deg(torch.acos((grav * g_true[:, None, None, :]).sum(-1).clamp(-1, 1)))
    return ((ferr < 0.02) & (ang < 0.5)).any(-1).double().mean(1)


# ------------------------------------------------------------------ the cases both test files run
EXTRA = ((-44, 44, 30), (-44, 44, 100))
ALL_POSES = tuple((r, p, 60) for r, p in POSES) + EXTRA
SHAPES = ((30, 44), (48, 64), (64, 64))
CASES = [(H, W, noise) for H, W in SHAPES for noise in (0.0, 0.02)]
N_GATE = 4000
_cache = {}


def case_id(case):
    return f"{case[0]}x{case[1]}-noise{case[2]}"


def make_case(case):
    """(data, samples (9, N_GATE, 3, 2) int32, f_true, g_true) of a case: the nine poses of ALL_POSES, computed once and left
    unchanged.  The samples are seeded uniform draws (the in-kernel draw has a test of its own)."""
    if case not in _cache:
        H, W, noise = case
        data, f, g = render(ALL_POSES, H, W, noise, seed=17)
        gen = torch.Generator().manual_seed(H * 1000 + W)
        B = len(ALL_POSES)
        samples = torch.stack([torch.randint(0, W, (B, N_GATE, 3), generator=gen), torch.randint(0, H, (B, N_GATE, 3), generator=gen)], -1)
        _cache[case] = (data, samples.to(torch.int32), f, g)
    return _cache[case]
