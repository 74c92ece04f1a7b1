"""Writes tests/golden/param_opt_reference.npz: what the reference's Adam optimiser on perspective fields
(siclib/models/optimization/perspective_opt.py: PerspectiveParamOpt) computes on recorded fields.  Data only: noisy fields
(sigma = 0.02, rendered by tests/rpf_gate.py) of three poses at 48 x 64 and 33 x 47 and of one pose at 120 x 160, and per image
  init64 / init32          the reference's initial estimate (roll, pitch, vfov), run in float64 and in float32
  states, cost64, cost32   (a) two states per image (the initial estimate; the truth + an offset) and at each the eight numbers
                           [up, lat, d up / d(r, p, v), d lat / d(r, p, v)] of the reference's cost under float64 and under
                           float32 autograd; a state is rejected where in float64 a pixel has |lat_pred - lat_t| < 1e-6 or an
                           up angle within 1e-6 rad of the clip angle, and retried 1e-3 further on, twice at most: `nudges`
                           counts the retries, `rejected` marks a state that stayed rejected
  fixed64, fixed_spread    (b) (roll, pitch, vfov) after K = 1, 5, 20, 100 steps with stopping off, in float64, and the largest
                           |float32 - float64| over nine float32 runs (the exact fields and eight one-ulp perturbations)
  default64, default_spread, default_steps64, default_steps32     (c) the same for the default conf
  sequence                 200 steps of [up, lat, gradient, gradient] per 48 x 64 image from the float64 run with stopping off,
                           rounded to float32, in the layout of gclm_param_opt_step's d_cost: what the state-machine tests
                           replay.  The reference differentiates the total, so both terms' slots carry the total's gradient

Runs where a checkout of the reference is available (oracle/ref_import.py says where); the tests that read the file need
neither.  siclib's optimisation package pulls in omegaconf and friends at import time; placeholder modules stand in where they
are missing, and the class's methods are bound to a plain namespace because BaseModel's constructor needs omegaconf.

    python tests/golden/make_golden_param_opt.py
"""
import importlib
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

import rpf_gate as rg  # noqa: E402
from conftest import perturbed  # noqa: E402
from make_golden_rpf import POSES, reference_solver  # noqa: E402

NOISE, SEED_BASE = 0.02, 31
SEEDS = (33, 31, 39, 31, 31, 60, 34)      # per image, found by scan()
IMAGES = [(48, 64, p) for p in POSES] + [(33, 47, p) for p in POSES] + [(120, 160, POSES[0])]
OFFSET = (0.05, -0.04, 0.06)
KS = (1, 5, 20, 100)
N_PERTURBED = 8
SEQ_STEPS = 200
THETA_CLIP = math.acos(1 - 1e-7)


class Namespace(types.SimpleNamespace):
    def train(self):
        pass


def bind(po, conf):
    """The reference's methods on a plain object; check_convergence also counts its calls and records (loss, gradient)."""
    cls = po.PerspectiveParamOpt
    ns = Namespace(conf=types.SimpleNamespace(**{**cls.default_conf, **conf}), steps=0, trace=[])
    for name in ("cost_function", "_update_estimate", "optimize", "_get_init_params"):
        setattr(ns, name, types.MethodType(getattr(cls, name), ns))

    def check_convergence(loss, losses_prev):
        ns.steps += 1
        grad = [p.grad.item() for p in (ns.roll_opt, ns.pitch_opt, ns.vfov_opt)]
        ns.trace.append([loss["up"].item(), loss["latitude"].item()] + grad + grad)       # (autograd gives the total's gradient: both terms carry it)
        return cls.check_convergence(ns, loss, losses_prev)

    ns.check_convergence = check_convergence
    return ns


def run(po, data, conf, dtype):
    """One reference call (B = 1): ((roll, pitch, vfov) float64, steps taken, initial estimate)."""
    data = {k: torch.from_numpy(v).to(dtype) for k, v in data.items()}
    ns = bind(po, conf)
    cam0, grav0 = ns._get_init_params(data)
    init = [grav0.roll.item(), grav0.pitch.item(), cam0.vfov.item()]
    ns.optimize(data, cam0, grav0)
    return np.array([ns.roll_opt.item(), ns.pitch_opt.item(), ns.vfov_opt.item()], np.float64), ns.steps, np.array(init, np.float64), ns


def cost_and_gradient(po, data, state, dtype):
    """[up, lat, d up / d(r, p, v), d lat / d(r, p, v)] of the reference's cost at `state`, and whether float64 rejects it."""
    data = {k: torch.from_numpy(v).to(dtype) for k, v in data.items()}
    h, w = data["latitude_field"].shape[-2:]
    ns = bind(po, {})
    ns.roll_opt, ns.pitch_opt, ns.vfov_opt = (torch.tensor([s], dtype=dtype, requires_grad=True) for s in state)
    cam = po.Camera.from_dict({"height": torch.tensor([float(h)], dtype=dtype), "width": torch.tensor([float(w)], dtype=dtype),
                               "vfov": ns.vfov_opt})
    cam, grav = ns._update_estimate(cam, None)
    up, lat = po.get_perspective_field(cam, grav)
    loss = ns.cost_function({"up_field": up, "latitude_field": lat}, data)
    params = (ns.roll_opt, ns.pitch_opt, ns.vfov_opt)
    g_up = torch.autograd.grad(loss["up"], params, retain_graph=True)
    g_lat = torch.autograd.grad(loss["latitude"], params)
    out = [loss["up"].item(), loss["latitude"].item()] + [g.item() for g in g_up] + [g.item() for g in g_lat]
    with torch.no_grad():
        cos = torch.nn.functional.cosine_similarity(up, data["up_field"], dim=1)
        ang = torch.acos(cos.clamp(-1, 1))
        rejected = bool(((lat - data["latitude_field"]).abs() < 1e-6).any() or ((ang - THETA_CLIP).abs() < 1e-6).any()
                        or ((ang - (math.pi - THETA_CLIP)).abs() < 1e-6).any())
    return np.array(out, np.float64), rejected


def scan(po, first=SEED_BASE, tries=40):
    """How SEEDS was found (python tests/golden/make_golden_param_opt.py --scan): per image the first noise seed from SEED_BASE
    on whose fields the REFERENCE, run in float64 with its default conf, stops before max_steps and recovers the pose to 0.1
    degrees.  The reference's schedule cuts the learning rate to 1e-8 within some forty steps of a noisy L1 cost, wherever the
    parameters then stand: on other seeds its own float64 result lies up to a degree off the pose or never meets its stop rule,
    and such fields say nothing about an implementation of it."""
    seeds = []
    for h, w, pose in IMAGES:
        for seed in range(first, first + tries):
            data = {k: v.numpy() for k, v in rg.render([pose], h, w, NOISE, seed=seed)[0].items()}
            r, steps, _, _ = run(po, data, {}, torch.float64)
            miss = np.degrees(np.abs(r - np.radians(pose))).max()
            print((h, w), pose, "seed", seed, "steps", steps, "miss deg", round(float(miss), 4), flush=True)
            if steps < 1000 and miss < 0.1:
                seeds.append(seed)
                break
        else:
            raise SystemExit(f"no seed for {(h, w, pose)}")
    print("SEEDS =", tuple(seeds))


def main():
    reference_solver()
    po = importlib.import_module("siclib.models.optimization.perspective_opt")
    if "--scan" in sys.argv:
        return scan(po)
    out = {"poses": np.array([p for _, _, p in IMAGES], np.float64), "sizes": np.array([(h, w) for h, w, _ in IMAGES], np.int32),
           "noise": NOISE, "seeds": np.array(SEEDS, np.int32), "ks": np.array(KS, np.int32), "offset": np.array(OFFSET)}
    n = len(IMAGES)
    init64, init32 = np.zeros((n, 3)), np.zeros((n, 3))
    states, cost64, cost32, nudges = np.zeros((n, 2, 3)), np.zeros((n, 2, 8)), np.zeros((n, 2, 8)), np.zeros((n, 2), np.int32)
    fixed64, fixed_spread = np.zeros((n, len(KS), 3)), np.zeros((n, len(KS), 3))
    default64, default_spread = np.zeros((n, 3)), np.zeros((n, 3))
    steps64, steps32 = np.zeros(n, np.int32), np.zeros((n, 1 + N_PERTURBED), np.int32)
    still_rejected = np.zeros((n, 2), bool)      # rejected after two retries: recorded, its gradients prove nothing
    sequence = []
    for i, (h, w, pose) in enumerate(IMAGES):
        data, _, _ = rg.render([pose], h, w, NOISE, seed=SEEDS[i])
        data = {k: v.numpy() for k, v in data.items()}
        out[f"up_field_{i}"], out[f"latitude_field_{i}"] = data["up_field"], data["latitude_field"]
        rng = np.random.default_rng(SEEDS[i])
        copies = [data] + [perturbed(data, rng) for _ in range(N_PERTURBED)]
        # (c) default conf
        default64[i], steps64[i], init64[i], _ = run(po, data, {}, torch.float64)
        for j, d in enumerate(copies):
            r, steps32[i, j], init, _ = run(po, d, {}, torch.float32)
            if j == 0:
                init32[i] = init
            default_spread[i] = np.maximum(default_spread[i], np.abs(r - default64[i]))
        # (b) fixed-length runs, stopping off
        for k, K in enumerate(KS):
            conf = {"abs_tol": -1.0, "rel_tol": 0.0, "max_steps": K}
            fixed64[i, k] = run(po, data, conf, torch.float64)[0]
            for d in copies:
                fixed_spread[i, k] = np.maximum(fixed_spread[i, k], np.abs(run(po, d, conf, torch.float32)[0] - fixed64[i, k]))
        if (h, w) == (48, 64):
            ns = run(po, data, {"abs_tol": -1.0, "rel_tol": 0.0, "max_steps": SEQ_STEPS}, torch.float64)[3]
            sequence.append(np.array(ns.trace, np.float64).astype(np.float32))
        # (a) cost and gradient
        truth = np.radians(np.array(pose, np.float64))
        for s, base in enumerate((init64[i], truth + np.array(OFFSET))):
            for retry in range(3):
                state = (base + 1e-3 * retry).astype(np.float32).astype(np.float64)      # the float32 numbers a caller hands over
                c64, rejected = cost_and_gradient(po, data, state, torch.float64)
                if not rejected:
                    break
            states[i, s], cost64[i, s], nudges[i, s], still_rejected[i, s] = state, c64, retry, rejected
            cost32[i, s] = cost_and_gradient(po, data, state.astype(np.float32), torch.float32)[0]
        print(i, (h, w), pose, "steps", steps64[i], steps32[i].tolist(), "default spread deg", np.degrees(default_spread[i]).round(5).tolist(),
              "fixed spread deg", np.degrees(fixed_spread[i]).max(1).tolist(), "nudges", nudges[i].tolist(), "rejected", still_rejected[i].tolist(), flush=True)
    out.update(init64=init64, init32=init32, rejected=still_rejected, states=states, cost64=cost64, cost32=cost32, nudges=nudges, fixed64=fixed64,
               fixed_spread=fixed_spread, default64=default64, default_spread=default_spread, default_steps64=steps64,
               default_steps32=steps32, sequence=np.stack(sequence))
    path = os.path.join(HERE, "param_opt_reference.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
