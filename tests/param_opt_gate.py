"""Float64 statement of gclm_param_opt (include/gclm.h), shared by the CPU tests (test_param_opt_abi.py) and the GPU tests
(test_param_opt.py).  A plain module, like the other *_gate.py files.  NumPy only: the closed-form cost and gradient the
kernel evaluates, the initial estimate, and the Adam / ReduceLROnPlateau / check_convergence state machine.  The CPU tests pin
the first to the reference's float64 autograd (tests/golden/param_opt_reference.npz, written by
tests/golden/make_golden_param_opt.py) and the last to torch.optim run live."""
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


def cost_and_gradient(up, lat, rpv):
    """[up, lat, d up / d(r, p, v), d lat / d(r, p, v)] of one image's fields `up` (2, H, W), `lat` (1, H, W) at (r, p, v)."""
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
    clamped = (s < -LAT_HI) | (s > LAT_HI)
    e = np.arcsin(np.clip(s, -LAT_HI, LAT_HI)) - lat
    k = np.where(clamped, 0.0, np.sign(e) / np.sqrt((1 - s) * (1 + s)))
    ds = {q: (d[0] * u + d[1] * w + d[2]) / n for q, d in dg.items()}
    ds["v"] = -((a * u + b * w) - s * (u * u + w * w) / n) / (f * n) * dfdv
    g_lat = [float((k * ds[q]).mean()) for q in "rpv"]
    return np.array([th.mean(), np.abs(e).mean()] + g_up + g_lat)


def initial_estimate(up, lat):
    """_get_init_params as the reference's optimize() reads it back: through Gravity.from_rp(...).roll / .pitch and the focal."""
    H, W = lat.shape[-2:]
    up, lat = np.asarray(up, np.float64).reshape(2, H, W), np.asarray(lat, np.float64).reshape(H, W)
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
