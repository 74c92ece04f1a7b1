"""CPU: the shared-intrinsics step gate of tests/shared_gate.py, and the oracle's envelope Cholesky that makes its float64
reference affordable at thousands of frames per group.

  - The honest float32 restatement of shared_step_kernel's Schur step (frame-order float32 sums over the group) meets the
    float64 gate at group sizes either side of the kernel's 64-frame reduction tile and 256-frame apply stride, up to
    2048 frames: the kernel's summation order needs no change at those sizes.
  - A restatement carrying one plausible kernel bug fails the gate on every frame the bug touches, at every size where
    the bug applies (test_step_oracle.test_step_gate_power is the model).
  - The envelope start of the oracle's Cholesky gives the dense loop's bits."""
import numpy as np
import pytest

from conftest import MEASURED
import shared_gate as sg

MODELS = ("pinhole", "simple_radial", "radial", "simple_divisional")
SIZES = (1, 2, 63, 64, 65, 256, 257, 1031, 2048)
RAGGED = (1, 2, 63, 64, 65, 130, 257)
HW = (32, 48)
LAM = 0.1
# the first step (from the trivial estimate) and the third; simple_divisional's gate holds its first step only
# (test_step_parity.DIV_STEPS)
STEPS = {"pinhole": (1, 3), "simple_radial": (1, 3), "radial": (1, 3), "simple_divisional": (1,)}


def _group_fields(model, sizes, seed=7):
    from oracle import synth
    parts = [synth.make_shared_group(seed, g, model, *HW, frames=n)[0] for g, n in enumerate(sizes)]
    data = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    gof = np.repeat(np.arange(len(sizes)), sizes)
    return data, sg.groups_of(gof)


def _start(oracle, model, data, groups, k):
    """theta_{k-1}: k - 1 fixed-lambda float32 oracle steps of every group from the trivial estimate."""
    cam, grav = np.zeros((len(data["up_field"]), 8), np.float32), np.zeros((len(data["up_field"]), 3), np.float32)
    for idx in groups:
        part = {key: v[idx] for key, v in data.items()}
        st = oracle.solve(part, {**sg.oracle_conf(model), "num_steps": k - 1, "early_stop": False}, precision="f32",
                          training=True, init=(None, None, None))
        cam[idx], grav[idx] = st["camera"], st["gravity"]
    return cam, grav


def _touched(mutant, model, groups, B):
    """Frames a mutant changes (None: the mutant does not apply to this layout).  A tile counted twice needs a second tile
    to show: one tile doubled scales the group's whole system and right-hand side, damping included, and leaves the step."""
    t = np.zeros(B, bool)
    for idx in groups:
        if mutant in ("drop_after_tile1", "last_tile_twice") and len(idx) > sg.TILE:
            t[idx] = True
        elif mutant == "apply_first_256":
            t[idx[sg.APPLY_STRIDE:]] = True
        elif mutant in ("damp_S", "no_EDg") or (mutant == "radial_k2_dropped" and model == "radial") or \
                (mutant == "lower_bound_off_by_one" and len(groups) > 1):
            t[idx] = True
    return t if t.any() else None


def _check(oracle, model, sizes, label):
    """The honest restatement within half the gate at every checked step; every mutant above the gate on every frame it
    touches, judged on the worst ratio over the checked steps (as test_step_oracle.test_step_gate_power: a frame counts
    as caught when one of the steps fails it)."""
    data, groups = _group_fields(model, sizes)
    B = sum(sizes)
    lam = np.full(B, LAM, np.float32)
    worst = {}
    for k in STEPS[model]:
        cam, grav = _start(oracle, model, data, groups, k)
        H, G = sg.frame_systems(oracle, model, data, cam, grav)
        H32, G32 = H.astype(np.float32), G.astype(np.float32)
        got = sg.restate_step(model, H32, G32, cam, grav, lam, groups)
        terms = sg.gate_terms(oracle, model, data, (cam, grav), lam, groups)
        ratio = sg.gate((cam, grav), got[:2], model, terms)
        MEASURED[f"shared_gate/restatement/{label}/k{k}"] = {"worst_ratio": ratio.max(0).tolist(),
                                                               "kappa_g": float(terms["kappa"].max())}
        assert not got[2].any() and not terms["ref64"]["step_failures"].any()
        assert ratio.max() < 0.5, (label, k, ratio.max(0), np.argwhere(ratio > 0.5)[:8])
        for mutant in sg.MUTANTS:
            bad = sg.restate_step(model, H32, G32, cam, grav, lam, groups, mutant=mutant)
            worst[mutant] = np.maximum(worst.get(mutant, 0), sg.gate((cam, grav), bad[:2], model, terms).max(1))
    for mutant, r in worst.items():
        touched = _touched(mutant, model, groups, B)
        if mutant == "S_transposed":
            # E_j . (Dinv E_i) and E_i . (Dinv E_j) are one number up to rounding (Dinv is symmetric bit for bit, E is
            # 2 x ni whatever its entries): the transposed kGS fill differs by rounding only, and the gate rightly passes it
            MEASURED[f"shared_gate/power/{label}/{mutant}"] = float(r.max())
            assert r.max() < 0.5, (label, mutant, r.max())
        elif touched is not None:
            MEASURED[f"shared_gate/power/{label}/{mutant}"] = float(r[touched].min())
            assert (r[touched] > 1).all(), (label, mutant, np.flatnonzero(touched & (r <= 1))[:8], r[touched].min())


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("model", MODELS)
def test_restatement_meets_gate_and_mutants_fail(oracle, model, N):
    """One group of N frames."""
    _check(oracle, model, (N,), f"{model}/N{N}")


@pytest.mark.parametrize("model", MODELS)
def test_restatement_ragged_groups(oracle, model):
    """Groups of unequal size handed through group_of_frame: the honest step passes, a lower_bound that is one frame late
    at every group boundary fails every frame (each group sums and updates its neighbour's first frame)."""
    _check(oracle, model, RAGGED, f"{model}/ragged")


def test_group_scale_is_one_for_one_frame(oracle):
    """tau * max(1, kappa_g / kappa_P) is exactly the per-image gate for a one-frame group: rho_g <= trace = P."""
    for model in MODELS:
        data, groups = _group_fields(model, (1, 1, 1))
        cam, grav = _start(oracle, model, data, groups, 1)
        H, _ = sg.frame_systems(oracle, model, data, cam, grav)
        assert np.array_equal(sg.group_scale(model, H, LAM, groups)[0], np.ones(3))


# ------------------------------------------------------------------ the envelope Cholesky is the dense one

def _bits(out):
    flat = {k: v for k, v in out.items() if k != "trace"}
    flat.update({f"trace/{k}": v for k, v in out.get("trace", {}).items()})
    return {k: np.ascontiguousarray(v).tobytes() for k, v in flat.items()}


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("case", ["shared", "independent", "shared_not_pd", "independent_not_pd"])
def test_envelope_cholesky_is_the_dense_loop(oracle, precision, case):
    """lm_oracle.c's chol_solve starts each inner sum at the first structural non-zero of the two rows; the terms it skips
    are exact zeros, so every output of the solve -- both entries (the reference rule and the from-a-state one), with
    the per-step trace -- has the dense loop's bits.  `_not_pd`: frame 5 carries a NaN pixel, so its (group's) damped
    system is not positive definite and the factorisation stops part-way."""
    from oracle import synth
    model = "radial"
    shared = case.startswith("shared")
    if shared:
        data = synth.make_shared_group(3, 0, model, *HW, frames=24)[0]
    else:
        data = synth.make_fields(3, range(12), model, *HW)[0]
    if case.endswith("not_pd"):
        data["up_field"][5, :, 7, 11] = np.nan
    conf = {"camera_model": model, "shared_intrinsics": shared, "num_steps": 4, "early_stop": False}
    outs = {}
    for dense in (False, True):
        if dense:
            with oracle.dense_cholesky():
                a = oracle.solve(data, conf, precision=precision, trace=True)
                b = oracle.solve(data, conf, precision=precision, trace=True, init=(None, None, None))
        else:
            a = oracle.solve(data, conf, precision=precision, trace=True)
            b = oracle.solve(data, conf, precision=precision, trace=True, init=(None, None, None))
        outs[dense] = (_bits(a), _bits(b))
    if case.endswith("not_pd"):
        assert (b["step_failures"][5] > 0) and (b["step_failures"].sum() == (4 * 24 if shared else 4)), b["step_failures"]
    for env, dense in zip(outs[False], outs[True]):
        assert env.keys() == dense.keys()
        for k in env:
            assert env[k] == dense[k], k
