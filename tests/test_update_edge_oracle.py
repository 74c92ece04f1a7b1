"""CPU: the edge table of the per-image LM update (tests/update_edges.py) is what it claims to be.

  - every state reaches the branch it names in the float64 oracle, with a margin: a state that stops reaching its branch
    fails here instead of quietly becoming a mid-domain case;
  - honest float32 (the float32 oracle) meets the unchanged step gate at every state with ratio <= 0.5 -- a condition on
    the choice of states, not a tolerance on the kernels;
  - the oracle's update is the reference's: the reference's own Gravity / BaseCamera methods at the table's states and
    deltas (golden_update_edges.npz), geocalib_amd's classes and the oracle agree at 1e-12;
  - the gate has power: a float64 update with one plausible kernel bug fails the step gate on the states named for it;
  - the seeded far states of the lambda-rule test take x10 steps, with cost changes no rounding can flip.

tests/test_update_edges.py (-m gpu) holds the HIP update to the same table."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, MEASURED
import update_edges as ue
from test_step_oracle import TAU_FLOOR, TAU_REL, div_k_allowance, step_gate, step_params

CONFIGS = [(m, f) for m in ue.MODELS for f in ue.FORMS]
SHARED = [(m, f, k) for m, f in CONFIGS for k in ue.shared_kinds(m)]
F32_ROOM = 0.5


def _gate_of(model, start, ref):
    """(B, components): the step gate tau_rel |delta^f64| + tau_floor of a step `ref` from `start`."""
    return TAU_REL * np.abs(step_params(model, ref["camera"], ref["gravity"]) - step_params(model, *start)) + TAU_FLOOR


def _check_branches(model, form, b, r64):
    """Every state of `b` took its branch in the float64 step `r64` (trace in float64), with BOUND_MARGIN gates to spare."""
    start = (b["cam0"], b["grav0"])
    gate = _gate_of(model, start, r64)
    delta = r64["trace"]["delta"][0]
    cam1, g1 = r64["trace"]["cam"][0], r64["trace"]["gravity"][0]          # fx fy k1 k2 / gravity after the step, float64
    fy_u, k1_u, k2_u = ue.unclamped(model, form, b["cam0"], delta)
    lo, hi = ue.f64_focal_bounds(ue.H)
    kb = ue.K_BOUND[model]
    g0 = b["grav0"].astype(np.float64)
    _, _, sigma = ue.householder(g0, "sigma_floor_dropped")
    assert not r64["step_failures"].any()
    for i, (name, branch) in enumerate(zip(b["names"], b["branches"])):
        why = (model, form, name, branch)
        if branch == "gy_pos":
            assert g0[i, 1] > 0.1 and g1[i, 1] > 0.1, why
        elif branch == "sgn0":
            assert g0[i, 0] == 0 and g0[i, 1] == 1, why
        elif branch == "gy_cross":
            assert g0[i, 1] < -0.01 and g1[i, 1] > 0.01, why
        elif branch == "sigma_floor":
            assert sigma[i] < 1e-7, why
        elif branch == "near_pole":
            assert 1e-3 < np.sqrt(1 - g0[i, 2] ** 2) < 0.02, why           # the 1e-4 of the roll denominator is 0.5 .. 10 % of it
        elif branch == "focal_min":
            assert np.log(lo) - np.log(fy_u[i]) >= ue.BOUND_MARGIN * gate[i, 0], why
            assert cam1[i, 1] == lo, why
        elif branch == "focal_max":
            assert np.log(fy_u[i]) - np.log(hi) >= ue.BOUND_MARGIN * gate[i, 0], why
            assert cam1[i, 1] == hi, why
        elif branch in ("k_hi", "k_lo"):
            s = 1.0 if branch == "k_hi" else -1.0
            assert s * k1_u[i] - kb >= ue.BOUND_MARGIN * gate[i, 4], why
            assert cam1[i, 2] == s * kb, why
        elif branch == "k2_hi":
            assert k2_u[i] - kb >= ue.BOUND_MARGIN * gate[i, 5], why
            assert cam1[i, 3] == kb, why
        else:
            assert branch == "mid", why
        if "ratio" in name:                                          # fx != fy: the bound is reached with the old ratio
            assert b["cam0"][i, 2] / b["cam0"][i, 3] == pytest.approx(1.25, rel=1e-6), why
            assert cam1[i, 0] / cam1[i, 1] == pytest.approx(1.25, rel=1e-6), why


def _f32_ratio(model, start, r32, r64):
    return step_gate(model, start, (r32["camera"], r32["gravity"]), (r64["camera"], r64["gravity"]),
                     extra=div_k_allowance(model, r32, r64))


@pytest.mark.parametrize("model,form", CONFIGS)
def test_every_state_reaches_its_branch_and_leaves_room_for_float32(oracle, model, form):
    b = ue.batch(model, form)
    assert len(set(b["names"])) == len(b["names"])
    r64, r32 = ue.oracle_step(oracle, model, form, b), ue.oracle_step(oracle, model, form, b, "f32")
    _check_branches(model, form, b, r64)
    assert np.array_equal(r32["step_failures"], r64["step_failures"])
    ratio = _f32_ratio(model, (b["cam0"], b["grav0"]), r32, r64)
    MEASURED[f"update_edges/{model}/{form}/oracle_f32/batch"] = dict(zip(b["names"], ratio.max(1).tolist()))
    assert np.isfinite(ratio).all() and (ratio <= F32_ROOM).all(), dict(zip(b["names"], ratio.max(1)))
    # the quirk: from g = (0, 1, 0) the reference reads roll = 0 (sign(0) = 0), so the (roll, pitch) step lands next to
    # (0, -1, 0) while the spherical step stays next to (0, 1, 0)
    gy = r64["trace"]["gravity"][0][b["names"].index("up_exact"), 1]
    assert gy < -0.9 if form == "rp_lin" else gy > 0.9, gy


SIGMAS = ("roll_uncertainty", "pitch_uncertainty", "gravity_uncertainty", "focal_uncertainty", "vfov_uncertainty")


@pytest.mark.parametrize("model,form", CONFIGS)
def test_second_step_and_uncertainty_leave_room_for_float32(oracle, model, form):
    """The other two things tests/test_update_edges.py asserts per state, for honest float32 first: the second step on the
    clamp and upside-down states (not simple_divisional: test_step_parity.DIV_STEPS) at <= 0.5 of the gate, and at the
    start states the covariance at <= 0.5 of the COV_EPS x condition number criterion and the sigmas at <= 0.5e-3.  The
    exact poles are not compared: the covariance is degenerate there (roll sigma > 1e10 in float64)."""
    from test_step_parity import COV_EPS
    b = ue.batch(model, form)
    if model != "simple_divisional":
        r1 = ue.oracle_step(oracle, model, form, b, "f32")
        b2 = {**b, "cam0": r1["camera"], "grav0": r1["gravity"]}
        a64, a32 = ue.oracle_step(oracle, model, form, b2), ue.oracle_step(oracle, model, form, b2, "f32")
        ratio = _f32_ratio(model, (b2["cam0"], b2["grav0"]), a32, a64).max(1)
        gated = np.array([n in ue.UPSIDE or br not in ("sigma_floor", "near_pole") for n, br in zip(b["names"], b["branches"])])
        assert (ratio[gated] <= F32_ROOM).all(), dict(zip(b["names"], ratio))
    u64 = ue.oracle_step(oracle, model, form, b, steps=0, training=False)
    u32 = ue.oracle_step(oracle, model, form, b, "f32", steps=0, training=False)
    keep = np.array([n not in ue.EXACT_POLES for n in b["names"]])
    assert (u64["roll_uncertainty"][~keep] > 1e4).all()
    esig = np.abs(np.stack([u32[k] for k in SIGMAS], 1)[keep] / np.stack([u64[k] for k in SIGMAS], 1)[keep] - 1)
    assert (esig <= 0.5e-3).all(), esig.max(0)
    Cr, C32 = u64["covariance"].astype(np.float64)[keep], u32["covariance"].astype(np.float64)[keep]
    Hr = np.linalg.inv(Cr)
    d = 1 / np.sqrt(np.abs(np.einsum("bii->bi", Hr)))
    kappa = np.linalg.cond(Hr * d[:, :, None] * d[:, None, :])
    sd = np.sqrt(np.abs(np.einsum("bii->bi", Cr)))
    ecov = (np.abs(C32 - Cr) / (sd[:, :, None] * sd[:, None, :])).max((1, 2)) / kappa
    assert (ecov <= 0.5 * COV_EPS).all(), (ecov.max(), kappa.max())


@pytest.mark.parametrize("model,form,kind", SHARED)
def test_every_shared_group_reaches_its_branch_and_leaves_room_for_float32(oracle, model, form, kind):
    b = ue.shared_group(model, form, kind)
    r64 = ue.oracle_step(oracle, model, form, b, shared=True)
    r32 = ue.oracle_step(oracle, model, form, b, "f32", shared=True)
    _check_branches(model, form, b, r64)
    g0, g1 = b["grav0"], r64["trace"]["gravity"][0]
    at = {n: i for i, n in enumerate(b["names"])}
    assert g0[at["upside_a"], 1] > 0.1 and g1[at["upside_a"], 1] > 0.1 and g1[at["cross"], 1] > 0 > g0[at["cross"], 1]
    assert np.array_equal(r32["step_failures"], r64["step_failures"])
    ratio = _f32_ratio(model, (b["cam0"], b["grav0"]), r32, r64)
    MEASURED[f"update_edges/{model}/{form}/oracle_f32/shared_{kind}"] = dict(zip(b["names"], ratio.max(1).tolist()))
    assert np.isfinite(ratio).all() and (ratio <= F32_ROOM).all(), dict(zip(b["names"], ratio.max(1)))


@pytest.mark.parametrize("model,form", CONFIGS)
def test_pole_on_the_pixel_grid_conditions(oracle, model, form):
    """What test_update_edges.py::test_pole_on_the_pixel_grid_pins_the_known_deviation rests on.  With the principal point
    on a pixel the reference's step from the exact pole is well conditioned in float32 (that pixel pins gravity: float32
    oracle <= 0.5 of the gate, both forms) and differs from the step without that pixel's up term by far more than 1000
    gates; the step without it leaves room for float32 in the spherical form (<= 0.5)."""
    b, masked = ue.pole_on_grid(model, form)
    bm = {**b, "data": masked}
    start = (b["cam0"], b["grav0"])
    r64, r32 = ue.oracle_step(oracle, model, form, b), ue.oracle_step(oracle, model, form, b, "f32")
    m64, m32 = ue.oracle_step(oracle, model, form, bm), ue.oracle_step(oracle, model, form, bm, "f32")
    assert (_f32_ratio(model, start, r32, r64) <= F32_ROOM).all()
    assert np.abs(r64["trace"]["delta"][0][:, :2]).max() < 1e-5 < 0.05 < np.abs(m64["trace"]["delta"][0][:, :2]).max(1).min()
    away = step_gate(model, start, (m64["camera"], m64["gravity"]), (r64["camera"], r64["gravity"])).max(1)
    assert (away > 10000).all(), away
    if form in ue.POLE_FORMS:
        assert (_f32_ratio(model, start, m32, m64) <= F32_ROOM).all()


# ------------------------------------------------------------------ the oracle's update is the reference's

def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    err = np.abs(a - b) / np.maximum(np.abs(b), 1.0)
    assert (err <= 1e-12).all(), (what, float(err.max()))


@pytest.mark.parametrize("model,form", CONFIGS)
def test_the_oracles_update_is_the_reference_s(oracle, model, form):
    from geocalib_amd import Gravity, camera_models
    golden = np.load(os.path.join(GOLDEN, "golden_update_edges.npz"))
    pre = f"{model}/{form}/"
    b = ue.batch(model, form)
    r64 = ue.oracle_step(oracle, model, form, b)
    delta = r64["trace"]["delta"][0]
    # the golden was recorded at this table: same states, same float64 step
    assert golden[pre + "names"].tolist() == b["names"]
    assert np.array_equal(golden[pre + "cam0"], b["cam0"]) and np.array_equal(golden[pre + "grav0"], b["grav0"])
    assert np.allclose(golden[pre + "delta"], delta, rtol=1e-8, atol=1e-12)
    delta = golden[pre + "delta"]
    sph, log = ue.FORMS[form]["use_spherical_manifold"], ue.FORMS[form]["use_log_focal"]
    nd = ue.NDIST[model]

    # (1) the package's classes against the reference's, on the stored inputs
    mine = ue.class_outputs(model, Gravity, camera_models[model], b["cam0"], b["grav0"], delta)
    ref = {k[len(pre) + 4:]: golden[k] for k in golden.files if k.startswith(pre + "out/")}
    assert set(mine) == set(ref)
    for k in ref:
        _close(mine[k], ref[k], (model, form, "package vs reference", k))
    i = b["names"].index("up_exact")
    assert ref["update_rp"][i, 1] < -0.9 and ref["update_sph"][i, 1] > 0.9          # the quirk, in the reference itself

    # (2) the package's classes on the oracle's own start (gravity as given) against the oracle's state after the step
    cam1, g1 = r64["trace"]["cam"][0], r64["trace"]["gravity"][0]
    own = ue.class_outputs(model, Gravity, camera_models[model], b["cam0"], b["grav0"], r64["trace"]["delta"][0], as_given=True)
    _close(own["update_sph" if sph else "update_rp"], g1, (model, form, "gravity"))
    _close(own["focal_log" if log else "focal_lin"][:, 2:4], cam1[:, :2], (model, form, "focal"))
    if nd:
        _close(own["dist"][:, 6:6 + nd], cam1[:, 2:2 + nd], (model, form, "dist"))

    # (3) ... and the numpy restatement the gate-power test mutates
    cam_r, grav_r = ue.apply_update(model, form, b["cam0"], b["grav0"], r64["trace"]["delta"][0])
    _close(grav_r, g1, (model, form, "restated gravity"))
    _close(cam_r[:, [2, 3, 6, 7]][:, :2 + nd], cam1[:, :2 + nd], (model, form, "restated camera"))
    _close(ue.grav_roll(np.asarray(golden[pre + "grav0"], np.float64) /
                        np.linalg.norm(golden[pre + "grav0"].astype(np.float64), axis=1, keepdims=True)), ref["roll"],
           (model, form, "restated roll"))


def test_float32_focal_bounds_are_the_reference_s():
    """update_edges.f32_focal_bounds, which the GPU test holds the clamped focal to, is what the reference's own
    update_focal clamps to in float32 (recorded in the golden), and within one float32 ulp of the float64 bounds."""
    golden = np.load(os.path.join(GOLDEN, "golden_update_edges.npz"))
    for h in (ue.H, 231, 480):
        mine = np.array(ue.f32_focal_bounds(h), np.float32)
        assert np.array_equal(mine, golden[f"bounds_f32/{h}"]), (h, mine, golden[f"bounds_f32/{h}"])
        assert (np.abs(mine.astype(np.float64) - ue.f64_focal_bounds(h)) <= 2 * np.spacing(mine)).all(), h


# ------------------------------------------------------------------ the gate has power

@pytest.mark.parametrize("model,form", CONFIGS)
def test_update_gate_power(oracle, model, form):
    """A float64 update with one bug (update_edges.UPDATE_MUTANTS), applied to the float64 oracle's own deltas, must fail
    the step gate (ratio > 1, or not finite) on every state named for the bug; the unmutated restatement passes everywhere."""
    b = ue.batch(model, form)
    r64 = ue.oracle_step(oracle, model, form, b)
    start, ref = (b["cam0"], b["grav0"]), (r64["camera"], r64["gravity"])
    delta = r64["trace"]["delta"][0]
    ratio = step_gate(model, start, ue.apply_update(model, form, b["cam0"], b["grav0"], delta), ref)
    assert (ratio <= F32_ROOM).all(), ratio.max(0)          # (the reference state is the oracle's float32 output: < 0.1)
    assert (ue.fx_error(b["cam0"], ue.apply_update(model, form, b["cam0"], b["grav0"], delta)[0]) <= 1e-15).all()
    ran = 0
    for mutant, (only_form, only_models, named) in ue.UPDATE_MUTANTS.items():
        if (only_form and only_form != form) or (only_models and model not in only_models):
            continue
        cam_m, grav_m = ue.apply_update(model, form, b["cam0"], b["grav0"], delta, mutant)
        ratio = step_gate(model, start, (cam_m, grav_m), ref).max(1)
        caught = ~(ratio <= 1)
        if mutant == "ratio_lost":          # the step gate reads fy only: fx is held to its ratio by fx_error
            ratio = ue.fx_error(b["cam0"], cam_m) / ue.FX_TOL
            caught = ~(ratio <= 1)
        for name in named:
            assert caught[b["names"].index(name)], (mutant, name, ratio[b["names"].index(name)])
        MEASURED[f"update_edges/{model}/{form}/gate_power/{mutant}"] = {n: float(ratio[b["names"].index(n)]) for n in named}
        ran += 1
    assert ran >= 3, ran


# ------------------------------------------------------------------ the lambda rule on the far states

@pytest.mark.parametrize("model", ue.LAMBDA_MODELS)
def test_lambda_rule_conditions_on_the_far_states(oracle, model):
    """What tests/test_update_edges.py::test_lambda_rule relies on, for exactly its seeds: on the decisions under test
    (update_edges.decisions_under_test: relative cost change >= 1e-3 in float64) the float32 and float64 oracles take the
    same decision; nearly all decisions are under test; at least two images take a x10 step under test within four steps
    (update_edges.far_states draws until two do); the upper clamp 1e2 is hit from 2e3 and the lower one holds from 1e-6."""
    tens = set()
    for lam0 in ue.LAMBDA_STARTS:
        _, c64, l64 = ue.lambda_run(oracle, model, lam0, "f64")
        _, c32, l32 = ue.lambda_run(oracle, model, lam0, "f32")
        under = ue.decisions_under_test(lam0, c64)
        rose = c64[1:] > c64[:-1]
        MEASURED[f"update_edges/{model}/lambda/oracle/{lam0:g}"] = {"under_test": int(under.sum()), "of": int(under.size),
                                                                     "x10_under_test": int((rose & under).sum())}
        assert np.allclose(l64[1:], ue.lambda_rule(l64[:-1], c64[:-1], c64[1:]), rtol=1e-12)
        assert np.allclose(l32[1:][under], l64[1:][under], rtol=1e-6), (lam0, l32[1:], l64[1:])
        if lam0 == 2e3:
            assert (l64[1] == 1e2).all()
            continue
        assert under.sum() >= 0.9 * under.size, (lam0, under.sum(0))
        if lam0 == 1e-6:
            assert (l64[1][~rose[0]] == 1e-6).all() and (~rose[0]).any()
        tens |= set(np.flatnonzero((rose & under).any(0)))
    assert len(tens) >= 2, tens


@pytest.mark.parametrize("mutant", ue.LAMBDA_MUTANTS)
@pytest.mark.parametrize("model", ["pinhole", "radial"])
def test_lambda_gate_power(oracle, model, mutant):
    """A lambda rule with one bug gives the next step another damping: the float64 step taken with it from the same state
    must fail the step gate against the float64 step with the rule's lambda, on every image."""
    far = ue.far_states(model)
    lam0 = 2e3 if mutant == "lambda_clamp_1e3" else 0.1
    out, cost, lam = ue.lambda_run(oracle, model, lam0, "f64", steps=1)
    start = (out["camera"], out["gravity"])
    bad = ue.lambda_rule(lam[0], cost[0], cost[1], mutant)
    assert np.allclose(lam[1], ue.lambda_rule(lam[0], cost[0], cost[1])) and (bad != lam[1]).all()
    c = {"camera_model": model, "num_steps": 1, "early_stop": False, "fix_lambda": True}
    step = lambda l: oracle.solve(far["data"], c, precision="f64", training=True, init=(*start, l.astype(np.float32)))  # noqa: E731
    ref, got = step(lam[1]), step(bad)
    ratio = step_gate(model, start, (got["camera"], got["gravity"]), (ref["camera"], ref["gravity"])).max(1)
    assert (ratio > 1).all(), ratio
