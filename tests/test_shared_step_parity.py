"""-m gpu: the shared-intrinsics LM step at large and ragged groups, per frame, against a float64 dense arrow-head step from
the same state (tests/shared_gate.py: the gate scaled by the group's own conditioning, kappa_g).

  - One call (launch_shared_step): groups either side of the 64-frame reduction tile and past the 256-frame apply
    stride, at least three groups per call so that later groups start beyond the first tile; whole batches of 1031 and
    2048 frames.  Final cost and covariance at HIP's own final state as test_step_parity.check_steps checks them.
  - The split protocol (gclm_shared_reduce, a sum over virtual ranks, gclm_shared_apply) with ragged group_of_frame:
    a group dealt 1 / 129, one dealt 70 / 70 (each rank reduces more than one tile), a group absent from a rank, a
    one-frame group, a rank without frames; all four models, so NI = 3 (radial) runs through the 32-float partials.
    Where one rank holds every frame the protocol is the one-call solve bit for bit.
  - Containment: a NaN pixel in the second tile of a group fails that group's step on every frame of it, and only it."""
import numpy as np
import pytest
import torch

from conftest import MEASURED
import shared_gate as sg
from test_step_parity import ALL_MODELS, DIV_STEPS, FIXED_K, _to_dev, check_steps, hip_run
from test_gpu_parity import run_virtual_ranks

pytestmark = pytest.mark.gpu

HW = (32, 48)
SEED = 21


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from geocalib_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _fields(model, sizes):
    from oracle import synth
    parts = [synth.make_shared_group(SEED, g, model, *HW, frames=n)[0] for g, n in enumerate(sizes)]
    data = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    return data, sg.groups_of(np.repeat(np.arange(len(sizes)), sizes))


def _gate_scale(oracle, model, data, groups):
    def f(start, lam):
        H, _ = sg.frame_systems(oracle, model, data, *start)
        scale, kappa = sg.group_scale(model, H, lam[0], groups)
        return scale, {"kappa_g": float(kappa.max()), "scale": float(scale.max())}
    return f


# ------------------------------------------------------------------ one call

ONE_CALL = [(m, gs, 3) for m in ALL_MODELS for gs in (1, 2, 63, 64, 65, 257)] + \
           [(m, None, n) for m in ("pinhole", "radial") for n in (1031, 2048)]


@pytest.mark.parametrize("model,group_size,n", ONE_CALL,
                         ids=[f"{m}-gs{gs}x{n}" if gs else f"{m}-batch{n}" for m, gs, n in ONE_CALL])
def test_shared_step_one_call(dev, oracle, model, group_size, n):
    sizes = (group_size,) * n if group_size else (n,)
    data, groups = _fields(model, sizes)
    conf = {"camera_model": model, "shared_intrinsics": True, "group_size": group_size}
    label = f"{model}/shared_gs{group_size}x{n}" if group_size else f"{model}/shared_batch{n}"
    check_steps(dev, oracle, label, conf, data, adaptive_ks=(), gate_scale=_gate_scale(oracle, model, data, groups))


# ------------------------------------------------------------------ split protocol

# group sizes, then per group the frames each rank holds (in frame order: rank 0 first)
LAYOUTS = {
    "two_ranks": ((130, 140, 1, 20), ((1, 129), (70, 70), (1, 0), (0, 20))),
    "three_ranks": ((130, 140, 1, 20), ((1, 64, 65), (70, 0, 70), (0, 0, 1), (0, 20, 0))),
    "empty_rank": ((130, 140, 1, 20), ((1, 129, 0), (70, 70, 0), (1, 0, 0), (0, 20, 0))),
    "one_rank": ((65, 65, 65), ((65, 0), (65, 0), (65, 0))),
}


def _deal(sizes, deal, dev):
    ranks = len(deal[0])
    sels = [[] for _ in range(ranks)]
    f0 = 0
    for size, counts in zip(sizes, deal):
        assert sum(counts) == size
        for r, c in enumerate(counts):
            sels[r] += range(f0, f0 + c)
            f0 += c
    gof_all = np.repeat(np.arange(len(sizes)), sizes)
    sels = [torch.tensor(s, dtype=torch.long, device=dev) for s in sels]
    gofs = [torch.from_numpy(gof_all[s.cpu().numpy()].astype(np.int32)).to(dev) for s in sels]
    return sels, gofs


def _split_run(dev, conf, data_dev, sels, gofs, G, steps):
    B = len(data_dev["up_field"])
    res = run_virtual_ranks(dev, {**conf, "num_steps": steps, "early_stop": False}, data_dev, sels, gofs, G, *HW)
    cam, grav = np.zeros((B, 8), np.float32), np.zeros((B, 3), np.float32)
    info = np.zeros((B, res[0][2].shape[1]), np.float32)
    for (c, g, i, _), sel in zip(res, sels):
        sel = sel.cpu().numpy()
        cam[sel], grav[sel], info[sel] = c, g, i
    return cam, grav, info


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("model", ALL_MODELS)
def test_shared_step_split_ragged(dev, oracle, model, layout):
    sizes, deal = LAYOUTS[layout]
    data, groups = _fields(model, sizes)
    data_dev = _to_dev(data, dev)
    sels, gofs = _deal(sizes, deal, dev)
    G, B = len(sizes), sum(sizes)
    conf = {"camera_model": model, "shared_intrinsics": True, "fix_lambda": True}
    ks = DIV_STEPS if model == "simple_divisional" else FIXED_K
    runs = {s: _split_run(dev, conf, data_dev, sels, gofs, G, s) for s in sorted({k - 1 for k in ks} | set(ks))}
    lam = np.full(B, 0.1, np.float32)
    for k in ks:
        (c0, g0, i0), (c1, g1, i1) = runs[k - 1], runs[k]
        terms = sg.gate_terms(oracle, model, data, (c0, g0), lam, groups)
        ratio = sg.gate((c0, g0), (c1, g1), model, terms)
        tag = f"shared_split/{model}/{layout}/fix/k{k}"
        MEASURED[tag] = {"worst_ratio": ratio.max(0).tolist(), "frames": B, "kappa_g": float(terms["kappa"].max())}
        assert np.isfinite(ratio).all() and (ratio <= 1).all(), (tag, ratio.max(0), np.argwhere(ratio > 1)[:8])
        assert not (i1[:, 14] > i0[:, 14]).any() and not terms["ref64"]["step_failures"].any(), tag
    if layout == "one_rank":
        # rank 0 holds everything and rank 1 adds zeros: the protocol IS the one-call solve (group_size 65), bit for bit
        for s, (c, g, _) in runs.items():
            one = hip_run(dev, {**conf, "group_size": sizes[0]}, data_dev, s, {})
            assert np.array_equal(c, one["cam"]) and np.array_equal(g, one["grav"]), s


# ------------------------------------------------------------------ containment

@pytest.mark.parametrize("model", ["pinhole", "radial"])
def test_shared_step_nan_frame_contained_to_its_group(dev, oracle, model):
    """group_size 100, two groups; frame 70 of group 0 (the second reduction tile) carries one NaN pixel.  Its damped
    gravity block is not positive definite, so group 0's step fails on every frame -- the oracle's shared rule: a failed
    group Cholesky zeroes the group's step -- each frame counting one step_failure per step and keeping its state (up to
    the rounding of a zero update).  Group 1 is the same call without the NaN, bit for bit (same batch, same sweep plan)."""
    data, groups = _fields(model, (100, 100))
    poisoned = {k: v.copy() for k, v in data.items()}
    poisoned["up_field"][70, :, 5, 9] = np.nan
    conf = {"camera_model": model, "shared_intrinsics": True, "group_size": 100, "fix_lambda": True}
    clean_dev, bad_dev = _to_dev(data, dev), _to_dev(poisoned, dev)
    start = hip_run(dev, conf, bad_dev, 0, {})
    ref = sg.reference_step(oracle, model, poisoned, (start["cam"], start["grav"]), np.full(200, 0.1, np.float32), groups)
    assert (ref["step_failures"][:100] == 1).all() and (ref["step_failures"][100:] == 0).all()
    worst = 0.0
    for steps in (1, 3):
        bad = hip_run(dev, conf, bad_dev, steps, {})
        clean = hip_run(dev, conf, clean_dev, steps, {})
        assert (bad["info"][:100, 14] == steps).all() and (bad["info"][100:, 14] == 0).all(), bad["info"][:, 14]
        for key in ("cam", "grav"):
            assert np.array_equal(bad[key][100:], clean[key][100:]), (steps, key)
            drift = np.abs(bad[key][:100] - start[key][:100]) / np.maximum(np.abs(start[key][:100]), 1e-3)
            worst = max(worst, float(drift.max()))
    MEASURED[f"shared_nan/{model}"] = {"group0_state_drift": worst}
    assert worst <= 2e-6, worst
