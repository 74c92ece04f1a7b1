"""Float64 statement of gclm_param_opt (include/gclm.h), shared by the CPU tests (test_param_opt_abi.py) and the GPU tests
(test_param_opt.py).  A plain module, like the other *_gate.py files.  NumPy only: the closed-form cost and gradient the
kernel evaluates, the initial estimate, and the Adam / ReduceLROnPlateau / check_convergence state machine.  The CPU tests pin
the first to the reference's float64 autograd (tests/golden/param_opt_reference.npz, written by
tests/golden/make_golden_param_opt.py) and the last to torch.optim run live.

Second half: the pass per pixel in float64 and in the kernel's float32 evaluation order (per_pixel), the bound derived from
the two (gate: nothing the device computes enters it), the condition under which a case says anything about a kernel
(indecisive, make_decisive), and the cases at the branch edges and ragged tiles of the pass -- seeded here (RAGGED, batch3,
batch70, INIT_EDGES) or recorded from the reference (tests/golden/param_opt_edges.npz, written by
tests/golden/make_golden_param_opt_edges.py)."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "param_opt_reference.npz")
THETA_CLIP = math.acos(1 - 1e-7)
LAT_HI = float(np.float32(1 - 1e-6))          # the reference's clamp bound as torch rounds it to float32 (gclm_render.h: kLatHi)
COS_EPS = 1e-8
DEFAULT = dict(max_steps=1000, lr=0.01, patience=3, abs_tol=1e-7, rel_tol=1e-9, lamb=0.5, use_scheduler=1, sched_patience=3,
               sched_cooldown=0, sched_factor=0.1, sched_threshold=1e-4, sched_min_lr=0.0, sched_eps=1e-8)
_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def fields(i):
    g = golden()
    return g[f"up_field_{i}"], g[f"latitude_field_{i}"]


def cost_and_gradient(up, lat, rpv, clamp_hi=LAT_HI):
    """[up, lat, d up / d(r, p, v), d lat / d(r, p, v)] of one image's fields `up` (2, H, W), `lat` (1, H, W) at (r, p, v).
    `clamp_hi`: the bound of the latitude clamp -- the kernel's float32 one, or the double 1 - 1e-6 of the reference run in
    float64 (as perspective_gate.fields has it)."""
    up, lat = np.asarray(up, np.float64).reshape(2, *up.shape[-2:]), np.asarray(lat, np.float64).reshape(lat.shape[-2:])
    H, W = lat.shape
    r, p, v = (float(s) for s in rpv)
    sr, cr, sp, cp = math.sin(r), math.cos(r), math.sin(p), math.cos(p)
    a, b, c = -sr * cp, -cr * cp, sp
    dg = {"r": (-cr * cp, sr * cp, 0.0), "p": (sr * sp, cr * sp, cp)}
    f = 0.5 * H / math.tan(0.5 * v)
    dfdv = -0.25 * H / math.sin(0.5 * v) ** 2
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    u, w = (x - W / 2) / f, (y - H / 2) / f
    # up
    qx, qy = a - c * u, b - c * w
    nq = np.maximum(np.hypot(qx, qy), 1e-12)
    ux, uy = qx / nq, qy / nq
    raw = np.hypot(up[0], up[1])
    tn = np.maximum(raw, COS_EPS)
    tx, ty = up[0] / tn, up[1] / tn
    dot, crs = ux * tx + uy * ty, ux * ty - uy * tx
    # a target shorter than eps stays shorter than 1: acos of its cosine, written without the cancellation
    sn = np.where(raw >= COS_EPS, np.abs(crs), np.sqrt(np.maximum(1 - (tx * tx + ty * ty), 0) + crs * crs))
    th = np.arctan2(sn, dot)
    clipped = (th < THETA_CLIP) | (th > math.pi - THETA_CLIP)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(clipped, 0.0, -crs / sn / nq)
    th = np.clip(th, THETA_CLIP, math.pi - THETA_CLIP)
    dq = {k: (d[0] - d[2] * u, d[1] - d[2] * w) for k, d in dg.items()}
    dq["v"] = (c * u / f * dfdv, c * w / f * dfdv)
    g_up = [float((m * (ux * dq[k][1] - uy * dq[k][0])).mean()) for k in "rpv"]
    # latitude
    n = np.sqrt(u * u + w * w + 1)
    s = (a * u + b * w + c) / n
    clamped = (s < -clamp_hi) | (s > clamp_hi)
    e = np.arcsin(np.clip(s, -clamp_hi, clamp_hi)) - lat
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(clamped, 0.0, np.sign(e) / np.sqrt((1 - s) * (1 + s)))
    ds = {q: (d[0] * u + d[1] * w + d[2]) / n for q, d in dg.items()}
    ds["v"] = -((a * u + b * w) - s * (u * u + w * w) / n) / (f * n) * dfdv
    g_lat = [float((k * ds[q]).mean()) for q in "rpv"]
    return np.array([th.mean(), np.abs(e).mean()] + g_up + g_lat)


def initial_estimate(up, lat, r0=None):
    """_get_init_params as the reference's optimize() reads it back: through Gravity.from_rp(...).roll / .pitch and the focal.
    `r0`: the roll of the centre pixel's up vector, where the caller moves it (initial_interval)."""
    H, W = lat.shape[-2:]
    up, lat = np.asarray(up, np.float64).reshape(2, H, W), np.asarray(lat, np.float64).reshape(H, W)
    if r0 is None:
        r0 = -math.atan2(up[0, H // 2, W // 2], -up[1, H // 2, W // 2])
    p0 = lat[H // 2, W // 2]
    v0 = min(max(abs(lat[0, W // 2] - lat[H - 1, W // 2]), float(np.float32(math.radians(20)))), float(np.float32(math.radians(120))))
    g = np.array([-math.sin(r0) * math.cos(p0), -math.cos(r0) * math.cos(p0), math.sin(p0)])
    g /= np.linalg.norm(g)
    roll = math.asin(-g[0] / (math.sqrt(1 - g[2] ** 2) + 1e-4))
    if not g[1] < 0:
        roll = -roll - math.pi * np.sign(g[0])
    f = H / 2 / math.tan(v0 / 2)
    return np.array([roll, math.asin(g[2]), 2 * math.atan(H / (2 * f))])


def total_of(cost, lamb):
    """(loss, gradient) as the update forms them: float64 from the float32 numbers of the pass, rounded once to float32."""
    cost = np.asarray(cost, np.float32).astype(np.float64)
    loss = np.float32(lamb * cost[1] + (1 - lamb) * cost[0])
    return float(loss), (lamb * cost[5:8] + (1 - lamb) * cost[2:5]).astype(np.float32).astype(np.float64)


class StateMachine:
    """One image's update, in float64 throughout (the kernel rounds parameters and moments to float32 once per step)."""

    def __init__(self, rpv, **conf):
        self.c = {**DEFAULT, **conf}
        self.p, self.m, self.v = np.array(rpv, np.float64), np.zeros(3), np.zeros(3)
        self.t, self.lr, self.best, self.bad, self.cool, self.window, self.done = 0, self.c["lr"], math.inf, 0, 0, [], False
        self.reductions = []

    def step(self, cost):
        c = self.c
        loss, g = total_of(cost, c["lamb"])
        self.t += 1
        self.m = self.m + (g - self.m) * (1 - 0.9)
        self.v = self.v * 0.999 + (1 - 0.999) * g * g
        bc1, bc2 = 1 - 0.9 ** self.t, 1 - 0.999 ** self.t
        self.p = self.p - self.lr / bc1 * (self.m / (np.sqrt(self.v) / math.sqrt(bc2) + 1e-8))
        if c["use_scheduler"]:
            if loss < self.best * (1 - c["sched_threshold"]):
                self.best, self.bad = loss, 0
            else:
                self.bad += 1
            if self.cool > 0:
                self.cool, self.bad = self.cool - 1, 0
            if self.bad > c["sched_patience"]:
                new = max(self.lr * c["sched_factor"], c["sched_min_lr"])
                if self.lr - new > c["sched_eps"]:
                    self.lr = new
                    self.reductions.append(self.t)
                self.cool, self.bad = c["sched_cooldown"], 0
        if loss <= c["abs_tol"]:
            self.done = True
        elif len(self.window) < c["patience"]:
            self.window.append(loss)
        elif abs(loss - self.window[0]) < c["rel_tol"]:
            self.done = True
        else:
            self.window = (self.window + [loss])[-c["patience"]:]
        return self.done


def replay(sequence, rpv, **conf):
    """The state machine over a recorded (steps, 8) sequence: (parameters, lr after each step, step of the stop or 0)."""
    sm = StateMachine(rpv, **conf)
    params, lrs, stop = [], [], 0
    for cost in sequence:
        done = sm.step(cost)
        params.append(sm.p.copy()), lrs.append(sm.lr)
        if done:
            stop = sm.t
            break
    return np.array(params), np.array(lrs), stop, sm


def torch_replay(sequence, rpv, **conf):
    """The same sequence through torch.optim.Adam + ReduceLROnPlateau on CPU float64 tensors and the reference's
    check_convergence, restated: what `replay` is pinned to."""
    import torch
    c = {**DEFAULT, **conf}
    ps = [torch.tensor([float(s)], dtype=torch.float64, requires_grad=True) for s in rpv]
    opt = torch.optim.Adam(ps, lr=c["lr"])
    sched = None
    if c["use_scheduler"]:
        sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", patience=c["sched_patience"], factor=c["sched_factor"],
                                                           threshold=c["sched_threshold"], cooldown=c["sched_cooldown"],
                                                           min_lr=c["sched_min_lr"], eps=c["sched_eps"])
    params, lrs, stop, window = [], [], 0, []
    for t, cost in enumerate(sequence, 1):
        loss, g = total_of(cost, c["lamb"])
        for p, gi in zip(ps, g):
            p.grad = torch.tensor([gi], dtype=torch.float64)
        opt.step()
        if sched is not None:
            sched.step(loss)
        params.append([p.item() for p in ps]), lrs.append(opt.param_groups[0]["lr"])
        if loss <= c["abs_tol"]:
            stop = t
        elif len(window) < c["patience"]:
            window.append(loss)
        elif abs(loss - window[0]) < c["rel_tol"]:
            stop = t
        else:
            window.append(loss)
            window = window[-c["patience"]:]
        if stop:
            break
    return np.array(params), np.array(lrs), stop


def fresh_state(rpv, lr):
    """B state records as gclm_param_opt_step takes them: (B, 32) uint32."""
    rpv = np.asarray(rpv, np.float32).reshape(-1, 3)
    s = np.zeros((rpv.shape[0], 32), np.uint32)
    s[:, 0:3] = rpv.view(np.uint32)
    s[:, 14:16] = np.array([lr], np.float64).view(np.uint32)
    s[:, 16] = np.array([np.inf], np.float32).view(np.uint32)
    return s


def read_state(s):
    s = np.ascontiguousarray(s, np.uint32)
    f = s.view(np.float32)
    return {"rpv": f[:, 0:3].astype(np.float64), "steps": s[:, 9].astype(np.int64), "done": s[:, 10].astype(np.int64),
            "lr": np.ascontiguousarray(s[:, 14:16]).view(np.float64)[:, 0], "best": f[:, 16], "total": f[:, 17]}


# ------------------------------------------------------------------ the pass per pixel, the derived bound, the edge cases
EDGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "param_opt_edges.npz")
LAT_HI64 = 1 - 1e-6                           # the clamp bound of the reference run in float64
OFFSET = (0.05, -0.04, 0.06)                  # state = truth + OFFSET, as tests/golden/make_golden_param_opt.py has it
NOISE = 0.02
ULP32 = 2.0 ** -23
MARGIN = 4                                    # perspective_gate.kappas' margin over a float32 restatement
SWITCH = 1e-5                                 # how far every pixel of a case stays from a switch (decisive())
CLAMP_MARGIN = 5e-7
DELIBERATE_SHORT = 5e-9                       # the one target length allowed inside [1e-9, 1e-7]
NUDGE = 1e-3
PER_PIXEL_MUTANTS = ("principal point", "dg/dr swapped", "dcp w dropped", "clip off", "clamp off", "short target by |crs|",
                     "sign(0) = 1")
_edges = None


def per_pixel(up, lat, rpv, dtype=np.float64, clamp_hi=LAT_HI, mutant=None):
    """The pass per pixel: ((8, H, W) float64 term planes whose means are the eight numbers, a dict of the deciding
    quantities).  dtype float64 is the yardstick per pixel; float32 restates the kernel's evaluation order -- the pose record
    formed in float64 and rounded once, 1 / f once, then products; q * (1 / |q|); atan2(sn, dot); the clip; the clamp;
    sign(0) = 0 -- with the factors c / f, -1 / f and df/dv applied to the planes in float64, as the kernel applies them
    after its sums.  `mutant` (CPU self-check only) names one deliberate error of PER_PIXEL_MUTANTS."""
    assert mutant is None or mutant in PER_PIXEL_MUTANTS, mutant
    T = np.dtype(dtype).type
    H, W = lat.shape[-2:]
    up, lat = np.asarray(up, np.float32).reshape(2, H, W).astype(T), np.asarray(lat, np.float32).reshape(H, W).astype(T)
    r, p, v = (float(s) for s in rpv)
    sr, cr, sp, cp = math.sin(r), math.cos(r), math.sin(p), math.cos(p)
    f = 0.5 * H / math.tan(0.5 * v)
    dfdv = -0.25 * H / math.sin(0.5 * v) ** 2
    ga, gb, gc, ifx, dar, dbr, dap, dbp, dcp = (T(s) for s in (-sr * cp, -cr * cp, sp, 1.0 / f, -cr * cp, sr * cp, sr * sp, cr * sp, cp))
    if mutant == "dg/dr swapped":
        dar, dbr = dbr, dar
    cx, cy = (T((W - 1) / 2), T((H - 1) / 2)) if mutant == "principal point" else (T(W / 2), T(H / 2))
    x, y = np.arange(W, dtype=T)[None, :], np.arange(H, dtype=T)[:, None]
    if T is np.float64:
        u, w = (x - cx) / f, (y - cy) / f
    else:
        u, w = (x - cx) * ifx, (y - cy) * ifx
    u, w = np.broadcast_to(u, (H, W)) + T(0), np.broadcast_to(w, (H, W)) + T(0)
    one, zero, eps = T(1), T(0), T(COS_EPS)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        # up
        qx, qy = ga - gc * u, gb - gc * w
        n2 = qx * qx + qy * qy
        iq = np.where(n2 < T(1e-24), T(1e12), one / np.sqrt(n2))
        ux, uy = qx * iq, qy * iq
        tx, ty = up
        tn2 = tx * tx + ty * ty
        dot, crs = ux * tx + uy * ty, ux * ty - uy * tx
        long = tn2 >= eps * eps
        it_short = one / np.maximum(np.sqrt(tn2), eps)
        it = np.where(long, one / np.sqrt(tn2), it_short)
        gap = one - tn2 * it_short * it_short
        dot, crs = dot * it, crs * it
        sn_short = np.sqrt(np.maximum(gap, zero) + crs * crs)
        if mutant == "short target by |crs|":
            sn, wgt = np.abs(crs), -np.sign(crs)
        else:
            sn, wgt = np.where(long, np.abs(crs), sn_short), np.where(long, -np.sign(crs), -crs / sn_short)
        raw = np.arctan2(sn, dot)
        clip = T(THETA_CLIP)
        top = T(math.pi) - clip
        lo, hi = raw < clip, raw > top
        if mutant == "clip off":
            lo, hi = np.zeros_like(lo), np.zeros_like(hi)
        m = np.where(lo | hi, zero, wgt * iq)
        th = np.where(lo, clip, np.where(hi, top, raw))
        pitch_y = dbp if mutant == "dcp w dropped" else dbp - dcp * w
        t_up = [th, m * (ux * dbr - uy * dar), m * (ux * pitch_y - uy * (dap - dcp * u)), m * (ux * w - uy * u)]
        # latitude
        r2 = u * u + w * w
        inn = one / np.sqrt(r2 + one)
        lin = ga * u + gb * w
        s = (lin + gc) * inn
        chi = T(clamp_hi)
        clamped = (s < -chi) | (s > chi)
        sc = np.clip(s, -chi, chi)
        if mutant == "clamp off":
            clamped, sc = np.zeros_like(clamped), np.clip(s, -one, one)
        d = np.arcsin(sc) - lat
        sg = np.where(d == 0, one, np.sign(d)) if mutant == "sign(0) = 1" else np.sign(d)
        k = np.where(clamped, zero, sg * inn * (one / np.sqrt((one - s) * (one + s))))
        t_lat = [np.abs(d), k * (dar * u + dbr * w), k * (dap * u + dbp * w + dcp), k * (lin - s * r2 * inn)]
    t = np.stack([t_up[0], t_lat[0]] + t_up[1:] + t_lat[1:]).astype(np.float64)
    t[4] *= float(gc) * float(ifx) * dfdv
    t[7] *= -float(ifx) * dfdv
    aux = {"theta": raw.astype(np.float64), "e": d.astype(np.float64), "s": s.astype(np.float64),
           "length": np.sqrt(tn2.astype(np.float64)), "lo": lo, "hi": hi, "clamped": clamped, "long": long, "n2": n2.astype(np.float64)}
    return t, aux


def bound_of(t64, t32):
    """MARGIN * D_k + MARGIN * 2^-23 * A_k per number, from the float64 and float32 term planes: D_k the mean of
    |term32 - term64| (absolute differences: no cancellation between pixels), A_k the mean of |term64| (the device's 1-ulp
    reciprocal square root and its atan2f / asinf against NumPy's)."""
    return MARGIN * np.abs(t32 - t64).mean((1, 2)) + MARGIN * ULP32 * np.abs(t64).mean((1, 2))


def gate(up, lat, rpv):
    """(the eight float64 numbers, their bounds, the float32 restatement's eight numbers) of one image at `rpv`."""
    t64, t32 = per_pixel(up, lat, rpv)[0], per_pixel(up, lat, rpv, np.float32)[0]
    return t64.mean((1, 2)), bound_of(t64, t32), t32.mean((1, 2))


def ratios(got, want, bound):
    """|got - want| / bound per number; where the bound is exactly 0 the number must be exactly 0 (ratio 0, else inf).  A
    non-finite number counts as inf."""
    err = np.abs(np.asarray(got, np.float64) - want)
    err = np.where(np.isfinite(err), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))


def indecisive(up, lat, rpv):
    """The pixels of a case that say nothing about a kernel: {what: mask}.  In the float64 restatement at `rpv`: a latitude
    within SWITCH of its target (an exact 0 in both precisions is a deliberate pixel, not a close one), an up angle within
    SWITCH of either clip angle, |s| within CLAMP_MARGIN of the clamp, a target length in [1e-9, 1e-7] other than
    DELIBERATE_SHORT; and where the float32 restatement's angle or latitude error is further than SWITCH / 8 from float64's."""
    a64, a32 = per_pixel(up, lat, rpv)[1], per_pixel(up, lat, rpv, np.float32)[1]
    exact = (a64["e"] == 0) & (a32["e"] == 0)
    th = a64["theta"]
    return {"latitude": ((np.abs(a64["e"]) < SWITCH) & ~exact) | (np.abs(a32["e"] - a64["e"]) > SWITCH / 8),
            "up": (np.abs(th - THETA_CLIP) < SWITCH) | (np.abs(th - (math.pi - THETA_CLIP)) < SWITCH)
            | (np.abs(a32["theta"] - th) > SWITCH / 8),
            "clamp": np.abs(np.abs(a64["s"]) - LAT_HI) < CLAMP_MARGIN,
            "short": (a64["length"] >= 1e-9) & (a64["length"] <= 1e-7) & (np.abs(a64["length"] - DELIBERATE_SHORT) > 1e-12)}


def make_decisive(up, lat, rpv, rounds=20):
    """Moves every offending target by NUDGE (the latitude up, the up vector round) until no pixel is indecisive; float32
    fields in, float32 copies out, and the number of rounds it took.  The clamp and the target lengths are the case's own:
    not nudged, refused."""
    H, W = lat.shape[-2:]
    up, lat = np.array(up, np.float32).reshape(2, H, W), np.array(lat, np.float32).reshape(1, H, W)
    cs, sn = math.cos(NUDGE), math.sin(NUDGE)
    for n in range(rounds + 1):
        bad = indecisive(up, lat, rpv)
        assert not bad["clamp"].any() and not bad["short"].any(), {k: np.argwhere(v).tolist() for k, v in bad.items()}
        if not bad["latitude"].any() and not bad["up"].any():
            return up, lat, n
        lat[0][bad["latitude"]] += np.float32(NUDGE)
        x, y = up[0][bad["up"]].astype(np.float64), up[1][bad["up"]].astype(np.float64)
        up[0][bad["up"]], up[1][bad["up"]] = (cs * x - sn * y).astype(np.float32), (sn * x + cs * y).astype(np.float32)
    raise AssertionError(f"still indecisive after {rounds} rounds: { {k: int(v.sum()) for k, v in bad.items()} }")


def render(pose, H, W, noise=0.0, seed=0):
    """Fields of a pinhole camera at `pose` = (roll, pitch, vfov) in radians, in float64 and rounded: up (2, H, W), latitude
    (1, H, W) float32.  Gaussian noise on both, the up field renormalised (as rpf_gate.render; NumPy's generator here)."""
    r, p, v = (float(s) for s in pose)
    a, b, c = -math.sin(r) * math.cos(p), -math.cos(r) * math.cos(p), math.sin(p)
    f = 0.5 * H / math.tan(0.5 * v)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    u, w = (x - W / 2) / f, (y - H / 2) / f
    up = np.stack([a - c * u, b - c * w])
    up /= np.maximum(np.hypot(up[0], up[1]), 1e-300)
    lat = np.arcsin(np.clip((a * u + b * w + c) / np.sqrt(u * u + w * w + 1), -1, 1))
    if noise:
        rng = np.random.default_rng(seed)
        up = up + noise * rng.standard_normal(up.shape)
        up /= np.hypot(up[0], up[1])
        lat = np.clip(lat + noise * rng.standard_normal(lat.shape), -math.pi / 2 + 1e-3, math.pi / 2 - 1e-3)
    return up.astype(np.float32), lat[None].astype(np.float32)


def f32(x):
    """The float32 numbers a caller hands over, as float64."""
    return np.asarray(x, np.float32).astype(np.float64)


# (a) ragged tiles: name -> (H, W, floats the planes are shifted by, pixels per lane, tiles, pose in degrees, seed)
RAGGED = {"6x260": (6, 260, 0, 4, 2 * 2, (10, 20, 60), 101), "50x516": (50, 516, 0, 4, 3 * 13, (10, 20, 60), 102),
          "50x516+1": (50, 516, 1, 1, 9 * 13, (10, 20, 60), 102), "7x130": (7, 130, 0, 2, 2 * 2, (5, 3, 40), 103),
          "45x131": (45, 131, 0, 1, 3 * 12, (-20, -10, 50), 104), "2x2": (2, 2, 0, 2, 1, (10, 20, 60), 105),
          "3x3": (3, 3, 0, 1, 1, (5, 3, 40), 106)}
BATCH3 = ((10, 20, 60, 102), (5, 3, 40, 107), (-20, -10, 50, 108))         # (c), (d): three distinct 50 x 516 images
B70, B70_SIZE = 70, (6, 8)
_cases = {}


def noisy_case(H, W, pose_deg, seed, offset=OFFSET):
    """(up, latitude, state): seeded noisy fields of a pose made decisive at the state truth + offset, cached."""
    key = (H, W, tuple(pose_deg), seed, tuple(offset))
    if key not in _cases:
        truth = np.radians(np.array(pose_deg, np.float64))
        state = f32(truth + np.array(offset))
        up, lat, _ = make_decisive(*render(truth, H, W, NOISE, seed), state)
        up.setflags(write=False), lat.setflags(write=False)
        _cases[key] = (up, lat, state)
    return _cases[key]


def ragged_case(name):
    H, W, _, _, _, pose, seed = RAGGED[name]
    return noisy_case(H, W, pose, seed)


def batch3(H=50, W=516):
    """Three distinct images of one size: (up (3, 2, H, W), latitude (3, 1, H, W), states (3, 3))."""
    cases = [noisy_case(H, W, p[:3], p[3] + (0 if (H, W) == (50, 516) else H * W)) for p in BATCH3]
    return np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases])


def batch70():
    """B70 images of 6 x 8, each with its own pose, noise seed and state."""
    rng = np.random.default_rng(70)
    poses = np.stack([rng.uniform(-40, 40, B70), rng.uniform(-30, 30, B70), rng.uniform(40, 90, B70)], 1)
    offsets = rng.uniform(0.02, 0.06, (B70, 3)) * rng.choice([-1.0, 1.0], (B70, 3))
    cases = [noisy_case(*B70_SIZE, poses[b], 700 + b, offsets[b]) for b in range(B70)]
    return np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases])


def pixels_per_lane(W, up_address, lat_address):
    """gclm_param_opt.hip's choice for a call."""
    bits = up_address | lat_address
    if W % 4 == 0 and bits % 16 == 0:
        return 4
    return 2 if W % 2 == 0 and bits % 8 == 0 else 1


def tile_count(H, W, px):
    return -(-W // (64 * px)) * -(-H // 4)


def last_tile_column(W, px):
    """The first x of the last tile column."""
    return (-(-W // (64 * px)) - 1) * 64 * px


# (b) branch edges: recorded by tests/golden/make_golden_param_opt_edges.py
EDGE_NAMES = ["zenith", "nadir", "zenith_q0", "lower_clip", "upper_clip", "exact_zero", "roll80_vfov120", "vfov20", "pitch-60"]


def edges():
    global _edges
    if _edges is None:
        with np.load(EDGES) as z:
            _edges = {k: z[k] for k in z.files}
    return _edges


def edge_case(name):
    g = edges()
    return g[f"up_{name}"], g[f"lat_{name}"], g[f"state_{name}"]


# (e) the initial estimate at its edges: (roll, pitch, vfov) in degrees of noise-free 48 x 64 fields
INIT_EDGES = ((170, 10, 60), (-170, 10, 60), (95, -15, 60), (-95, -15, 60), (90, 20, 60), (10, 5, 10), (10, 5, 150))


def init_fields(pose_deg, H=48, W=64):
    up, lat = render(np.radians(np.array(pose_deg, np.float64)), H, W)
    if abs(pose_deg[0]) == 90:                # roll of exactly 90 degrees: g_y = 0, which cos(pi / 2) in float64 is not
        up[1, H // 2, W // 2] = 0.0
    return up, lat


def initial_interval(up, lat):
    """(lo, hi) per parameter for the device's initial estimate, which forms r0 with atan2f: what initial_estimate spans when
    r0 moves by +-2 float32 ulps -- near +-90 degrees Gravity.roll's asin amplifies one ulp of r0 some seventy-fold, and at
    g_y = 0 the two branches meet 0.03 rad apart -- widened by 4 float32 ulps of the result (perspective_gate.gates'
    latitude interval has this shape)."""
    H, W = lat.shape[-2:]
    r0 = -math.atan2(float(up[0, H // 2, W // 2]), -float(up[1, H // 2, W // 2]))
    step = float(np.spacing(np.float32(abs(r0))))
    span = np.array([initial_estimate(up, lat, r0 + j * step) for j in (-2, -1, 0, 1, 2)])
    lo, hi = span.min(0), span.max(0)
    return lo - 4 * np.spacing(np.abs(lo).astype(np.float32)).astype(np.float64), hi + 4 * np.spacing(np.abs(hi).astype(np.float32)).astype(np.float64)
