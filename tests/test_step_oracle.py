"""CPU: the oracle's one-step-from-a-state entry (lm_oracle_solve_from, `oracle.solve(..., init=...)`) and the per-step
gate that tests/test_step_parity.py holds every HIP LM step to.

One damped LM step is well conditioned where a whole solve is not: with D = diag(H), D^-1/2 (H + lambda D) D^-1/2 has its
eigenvalues in [lambda, P + lambda], so float32 rounding of H and G moves the step by at most (P + lambda) / lambda times
their relative error (51 at lambda = 0.1, P = 5).  A step taken from a kernel's own state can therefore be compared with a
float64 step from that same state, per image, with a tight gate and no exemptions.  These tests show that
  - the new entry is the old loop (identity, chaining), and
  - the gate leaves room for honest float32 arithmetic and fails every image of a subtly wrong sweep (gate power)."""
import numpy as np
import pytest

from conftest import MEASURED

NDIST = {"pinhole": 0, "simple_radial": 1, "radial": 2, "simple_divisional": 1}
# Started at 1e-4 / 1e-6 and measured on the MI355X: the log focal of a float32 update (exp(log f + delta), log f ~ 5 with
# an ulp of 4.8e-7) misses the float64 step by up to 1.13e-6, radial's latitude-only k2 by 1.69e-4 |delta|.  At 2e-4 / 2e-6
# every mutation of test_step_gate_power still fails every image.
TAU_REL, TAU_FLOOR = 2e-4, 2e-6


def step_params(model, cam, grav):
    """The components the step gate compares: log focal (fy; fx keeps its ratio), gravity (3), distortion (k1[, k2])."""
    cam = np.asarray(cam, np.float64)
    return np.concatenate([np.log(cam[:, 3:4]), np.asarray(grav, np.float64), cam[:, 6:6 + NDIST[model]]], 1)


def step_gate(model, start, got, ref, tau_rel=TAU_REL, tau_floor=TAU_FLOOR, extra=None):
    """Ratio (B, components) of |theta_k - theta_k^ref| to the gate tau_rel |delta^ref| + tau_floor (+ extra), where
    start = (cam, grav) of theta_{k-1}, got / ref = (cam, grav) of theta_k, ref being the float64 step from `start`.
    The step passes where every ratio is <= 1.  `extra` (B, components): an allowance added to the gate (the named
    simple_divisional k exception)."""
    p0, pg, pr = (step_params(model, *s) for s in (start, got, ref))
    gate = tau_rel * np.abs(pr - p0) + tau_floor
    if extra is not None:
        gate = gate + extra
    return np.abs(pg - pr) / gate


def div_k_allowance(model, ref32, ref64):
    """The one named exception: simple_divisional's k column cancels in float32 (camera.py:913), so its k component adds
    10x the float32-vs-float64 oracle spread of the same step, per image.  No other component, no other model.

    That does not cover all of it: once k1 != 0 the cancelling k column reaches every component of the coupled step --
    from step 2 on the float32 oracle's own step misses the float64 one by 500-9000x the gate on focal and gravity, HIP's
    by ~1000x.  tests/test_step_parity.py therefore gates simple_divisional's first step only (k1 = 0) and reports the
    rest as a limit instead of widening the gate."""
    p32, p64 = step_params(model, ref32["camera"], ref32["gravity"]), step_params(model, ref64["camera"], ref64["gravity"])
    extra = np.zeros_like(p64)
    if model == "simple_divisional":
        extra[:, 4] = 10 * np.abs(p32[:, 4] - p64[:, 4])
    return extra


def _fields(model, B, H, W, seed=3):
    from oracle import synth
    return synth.make_fields(seed, range(B), model, H, W)[0]


def _same(a, b):
    for k in a:
        if k in b and not isinstance(a[k], dict):
            assert np.array_equal(a[k], b[k]), k


# ------------------------------------------------------------------ the new entry is the old loop

@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("model,shared", [("pinhole", False), ("simple_radial", False), ("radial", False),
                                          ("simple_divisional", False), ("simple_radial", True)])
def test_solve_from_without_a_state_is_solve(oracle, model, shared, precision):
    data = _fields(model, 4, 36, 52)
    conf = {"camera_model": model, "num_steps": 6, "early_stop": False, "shared_intrinsics": shared}
    a = oracle.solve(data, conf, precision=precision, trace=True)
    b = oracle.solve(data, conf, precision=precision, trace=True, init=(None, None, None))
    assert (a["step_failures"] == 0).all()
    _same(a, b)
    _same(a["trace"], b["trace"])


@pytest.mark.parametrize("mode", ["independent", "shared_intrinsics", "fix_lambda", "adaptive_lambda"])
def test_single_steps_chain_to_the_solve(oracle, mode):
    """k one-step calls, each from the previous call's camera and gravity, are the k-step solve bit for bit (float32
    build: its state round-trips through the float32 outputs exactly).

    The lambda of step k (k = 0, 1, ... as the loop counts) is trace["lambda"][k]: the trace row of step k records the
    damping BEFORE that step's rule runs, i.e. the one its Cholesky used.  info[13] ("lambda") of a j-step solve is the
    value after the rule of its last step -- the lambda step j would use -- so the two agree: trace["lambda"][j] equals
    info[13] of the first j steps (checked below)."""
    model = "radial" if mode != "shared_intrinsics" else "simple_radial"
    data = _fields(model, 3, 40, 56, seed=5)
    K = 5
    conf = {"camera_model": model, "num_steps": K, "early_stop": False,
            "shared_intrinsics": mode == "shared_intrinsics", "fix_lambda": mode == "fix_lambda"}
    full = oracle.solve(data, conf, precision="f32", trace=True)
    lam_trace = full["trace"]["lambda"]
    if mode == "adaptive_lambda":
        assert len(np.unique(lam_trace)) > 1          # the rule actually moved lambda
    one = {**conf, "num_steps": 1}
    cam, grav = None, None
    for k in range(K):
        lam = lam_trace[k].astype(np.float32)
        out = oracle.solve(data, one, precision="f32", init=(cam, grav, lam if k else None))
        cam, grav = out["camera"], out["gravity"]
        assert np.array_equal(cam[:, [2, 3, 6, 7]], full["trace"]["cam"][k].astype(np.float32)), k
        assert np.array_equal(grav, full["trace"]["gravity"][k].astype(np.float32)), k
        if k + 1 < K:
            assert np.array_equal(out["lambda"], lam_trace[k + 1].astype(np.float32)), k
    _same({k: v for k, v in full.items() if k not in ("stop_at", "initial_cost", "initial_up_cost",
                                                      "initial_latitude_cost", "trace")}, out)
    # num_steps = 0 from the final state: the final costs and covariance of the solve, at that state
    at = oracle.solve(data, {**conf, "num_steps": 0}, precision="f32", init=(cam, grav, out["lambda"]))
    for key in ("final_cost", "final_up_cost", "final_latitude_cost", "covariance", "camera", "gravity"):
        assert np.array_equal(at[key], full[key]), key


def test_failed_cholesky_stays_with_its_image(oracle):
    """lm_oracle_solve zeroes the whole batch's step when one image's damped system is not positive definite (:129-133);
    the from-a-state entry contains it to that image, like the HIP update, and counts it in step_failures."""
    data = _fields("simple_radial", 3, 24, 32)
    for k in ("up_confidence", "latitude_confidence"):
        data[k][1] = 0                   # image 1: H = 0, damped H = 1e-6 I, G = 0 -> a zero step but no failure ...
    data["latitude_field"][1] = np.nan   # ... with NaN residuals every entry is NaN: not positive definite
    data["up_field"][1] = np.nan
    conf = {"camera_model": "simple_radial", "num_steps": 1, "early_stop": False, "fix_lambda": True}
    ref = oracle.solve(data, conf, precision="f64", training=True)
    got = oracle.solve(data, conf, precision="f64", training=True, init=(None, None, None))
    start = oracle.solve(data, {**conf, "num_steps": 0}, precision="f64", training=True)
    assert np.array_equal(ref["camera"], start["camera"])            # the reference rule: nobody moved
    assert got["step_failures"].tolist() == [0, 1, 0]
    assert np.array_equal(got["camera"][1], start["camera"][1])
    assert (got["camera"][[0, 2], 3] != start["camera"][[0, 2], 3]).all()


# ------------------------------------------------------------------ the gate has power

GATE_SHAPES = [((480, 640), 3), ((230, 324), 2)]


GATE_STEPS = (1, 2, 3, 10)        # the fixed-lambda steps tests/test_step_parity.py checks (k = 20: converged, no power)


def _state(oracle, model, data, k):
    """theta_{k-1}: the state after k - 1 fixed-lambda float32 steps, the start of step k."""
    conf = {"camera_model": model, "num_steps": k - 1, "early_stop": False, "fix_lambda": True}
    st = oracle.solve(data, conf, precision="f32", training=True)
    return conf, st["camera"], st["gravity"], np.full(len(st["camera"]), 0.1, np.float32)


def _mutations(oracle, model, data, cam, grav):
    H, W = data["latitude_field"].shape[-2:]
    out = {}

    def drop_row(y):
        m = {k: v.copy() for k, v in data.items()}
        m["up_confidence"][:, y] = 0
        m["latitude_confidence"][:, y] = 0
        return m
    out["row_0_dropped"] = drop_row(0)
    out["row_H/2_dropped"] = drop_row(H // 2)
    y = H // 3                                   # a mirrored row off by one: row H - y read from row H - y + 1
    m = {k: v.copy() for k, v in data.items()}
    for k in m:
        m[k][..., H - y, :] = m[k][..., H - y + 1, :]
    out["mirror_off_by_one"] = m
    m = {k: v.copy() for k, v in data.items()}   # the ragged tail: the last column of the width dropped
    m["up_confidence"][..., W - 1] = 0
    m["latitude_confidence"][..., W - 1] = 0
    out["last_column_dropped"] = m
    # one row's latitude sums with the wrong sign: the residual sin(lat) - sin(lat(theta)) of row H/4 negated (its
    # J^T W r terms flip, J^T W J and the cost stay)
    _, lat_pred = oracle.render(model, H, W, cam, grav)
    m = {k: v.copy() for k, v in data.items()}
    yy = H // 4
    s = 2 * np.sin(lat_pred[:, 0, yy].astype(np.float64)) - np.sin(m["latitude_field"][:, 0, yy].astype(np.float64))
    m["latitude_field"][:, 0, yy] = np.arcsin(np.clip(s, -1, 1)).astype(np.float32)
    out["latitude_row_sign"] = m
    return out


@pytest.mark.parametrize("shape,B", GATE_SHAPES)
@pytest.mark.parametrize("model", ["pinhole", "simple_radial", "radial"])
def test_step_gate_power(oracle, model, shape, B):
    """At each step k of GATE_STEPS the step gate passes the float32 oracle's step against the float64 step from the same
    state.  A float64 step taken on mutated fields (what a sweep that drops, mirrors or mis-signs one row or column would
    compute) must fail the gate on every image.  That is judged on the worst ratio over the checked steps, not per step:
    an image counts as caught when at least one of steps 1, 2, 3 and 10 fails it, which is how the GPU test checks them.
    (One wrong row can move a step by less than the gate where that row has little lever arm on the step, e.g. the centre
    row at the first step; another checked step then catches it.)

    simple_divisional is not here: its gate applies to the first step only (div_k_allowance), and one step from
    k1 = 0 does not fail every image under every mutation -- a limit of that model's float32 formulas, not a gate."""
    data = _fields(model, B, *shape)
    worst = {}
    for k in GATE_STEPS:
        conf, cam, grav, lam = _state(oracle, model, data, k)
        one = {**conf, "num_steps": 1}
        ref64 = oracle.solve(data, one, precision="f64", training=True, init=(cam, grav, lam))
        ref32 = oracle.solve(data, one, precision="f32", training=True, init=(cam, grav, lam))
        start, ref = (cam, grav), (ref64["camera"], ref64["gravity"])
        r = step_gate(model, start, (ref32["camera"], ref32["gravity"]), ref)
        assert r.max() < 0.5, (k, r.max(0))
        for name, m in _mutations(oracle, model, data, cam, grav).items():
            bad = oracle.solve(m, one, precision="f64", training=True, init=(cam, grav, lam))
            r = step_gate(model, start, (bad["camera"], bad["gravity"]), ref).max(1)
            worst[name] = np.maximum(worst.get(name, 0), r)
    for name, r in worst.items():
        MEASURED[f"gate_power/{model}/{shape[0]}x{shape[1]}/{name}"] = r.tolist()
        assert (r > 1).all(), (name, r)
