"""The early stop of the LM solve: case table and comparison functions, shared by tests/test_early_stop_oracle.py (CPU: the
table is what it claims to be) and tests/test_early_stop.py (-m gpu: the HIP solve is held to it).

The identity under test needs no tolerance.  A reference solve that breaks at iteration i returns theta_{i+1} with
stop_at = i + 1, and the final costs and the uncertainty at that state (lm_optimizer.py:576-644): what the same solver
returns for {num_steps: stop_at, early_stop: False}.  Nothing in a HIP call's plan depends on num_steps in a way that
changes bits, so for HIP the two must agree BIT FOR BIT -- camera, gravity, every cost, the sigmas, the covariance,
stop_at, lambda and step_failures -- on every launch path.

Every case stops at a step `stop` at which the state still moves by far more than any gate (tolerances 1e-5 .. 1e-2, not
the default 1e-8 at which theta_{s-1}, theta_s and theta_{s+1} are the same to every assertion), so that an off-by-one in
the stop logic -- the wrong state buffer, a tentative state that is kept, a per-image stop -- fails the comparisons below.
tests/test_early_stop_oracle.py proves per case, in the float32 and the float64 oracle:
  margin     r = |cost_k - cost_{k-1}| / (atol + rtol |cost_{k-1}|): >= LOUD for some image at every k < stop, <= QUIET for
             every image at k = stop.  HIP's costs sit within 3e-5 relative of its yardsticks' (DESIGN.md section 5), which
             moves r by at most ~0.06 at tol = 1e-4 and cost <= 0.1: neither side of the margin can be crossed by rounding.
  decisive   theta_{s-1} and theta_{s+1}, and the costs and the covariance at each, miss theta_s by >= DECISIVE gates.
  honest     the float32 oracle's result at `stop` is within F32_ROOM of the gate of the float64 one.
"""
import numpy as np

from conftest import measure_result
from test_gpu_parity import TOL
from test_step_parity import COV_EPS

LOUD, QUIET, DECISIVE, F32_ROOM = 1.33, 0.75, 5.0, 0.5
SHAPE = (48, 64)

# model, seed, images (indices of oracle/synth.py: make_fields) or `groups` shared-intrinsics groups of `frames` frames
# (make_shared_group), tol = atol = rtol, num_steps, and `stop`: the stop_at the case is there for.  `natural`: the step at
# which the comparison first goes quiet when num_steps does not get in the way (stop = min(natural, num_steps)); given
# only where it differs from `stop`.  shape: SHAPE unless given.  The q = |dcost| / (1 + |cost|) these rest on, float64
# oracle, 48x64, seed 31, one image: pinhole 7.1e-3, 3.1e-3, 6.5e-4, 2.4e-5, 4.3e-6; radial 6.9e-3, 2.2e-4, 1.6e-3,
# 9.7e-4, 7.5e-4, 4.3e-4, 1.9e-4, 9.2e-5, 1.2e-5 (not monotone: step 2 is quiet at 5e-4 although steps 3 .. 5 are not).
_PIN = {"model": "pinhole", "seed": 31, "images": [0]}
_RAD = {"model": "radial", "seed": 31, "images": [0]}
CASES = {
    "pinhole_s3": {**_PIN, "tol": 1.5e-3, "num_steps": 30, "stop": 3},                          # an odd stop
    "pinhole_s4": {**_PIN, "tol": 1.2e-4, "num_steps": 30, "stop": 4},                          # an even one
    # ... and num_steps around it: the stop fires at the last position first_quiet_step scans | the last comparison is
    # quiet and nothing is "stopped" | the comparison is never quiet
    "pinhole_s4_n5": {**_PIN, "tol": 1.2e-4, "num_steps": 5, "stop": 4},
    "pinhole_s4_n4": {**_PIN, "tol": 1.2e-4, "num_steps": 4, "stop": 4},
    "pinhole_s4_n3": {**_PIN, "tol": 1.2e-4, "num_steps": 3, "stop": 3, "natural": 4},
    "radial_quiet_then_loud": {**_RAD, "tol": 5e-4, "num_steps": 30, "stop": 2},                # louder steps follow the stop
    "radial_s9": {**_RAD, "tol": 3e-5, "num_steps": 30, "stop": 9},                             # a late stop
    "simple_radial_scalar": {"model": "simple_radial", "seed": 31, "images": [0], "shape": (47, 63), "tol": 1.5e-4,
                             "num_steps": 30, "stop": 4},                                         # W % 4 != 0: the scalar path
    # simple_divisional's float32 formulas cancel from its second step on (test_step_parity.DIV_STEPS): honest float32
    # holds it to the first step, and to draws on which that step is well conditioned.  96x128: six records per image
    "divisional_s1": {"model": "simple_divisional", "seed": 32, "images": [0], "shape": (96, 128), "tol": 1e-2,
                      "num_steps": 30, "stop": 1},
    # five independent images: some are quiet steps before the batch is (seed 77, pinhole: first quiet at 3, 3, 3, 4, 2)
    "pinhole_b5": {"model": "pinhole", "seed": 77, "images": [0, 1, 2, 3, 4], "tol": 3e-4, "num_steps": 30, "stop": 4},
    "simple_radial_b5": {"model": "simple_radial", "seed": 77, "images": [0, 1, 2, 3, 4], "tol": 2e-4, "num_steps": 30, "stop": 4},
    "radial_b5": {"model": "radial", "seed": 77, "images": [0, 1, 2, 3, 4], "tol": 7e-5, "num_steps": 30, "stop": 9},
    "divisional_b5": {"model": "simple_divisional", "seed": 32, "images": [5, 9, 11, 14, 15], "tol": 1e-2, "num_steps": 30, "stop": 1},
    # shared intrinsics: one group (group_size None: the oracle applies as it stands), and two groups of three, whose stop
    # is the first step at which every frame of BOTH groups is quiet in the oracle's fixed-length solves of each
    "shared_one_group": {"model": "simple_radial", "seed": 31, "groups": 1, "frames": 6, "tol": 5e-5, "num_steps": 30, "stop": 5},
    "shared_two_groups": {"model": "pinhole", "seed": 77, "groups": 2, "frames": 3, "tol": 5e-4, "num_steps": 30, "stop": 4},
    # one conf, two inputs whose stops lie six steps apart: the counters of one solve must not reach the next
    "radial_x": {**_RAD, "tol": 3e-4, "num_steps": 30, "stop": 2},
    "radial_y": {"model": "radial", "seed": 77, "images": [3], "tol": 3e-4, "num_steps": 30, "stop": 8},
}
TRIPLE = ("pinhole_s4_n5", "pinhole_s4_n4", "pinhole_s4_n3")
BATCHES = ("pinhole_b5", "simple_radial_b5", "radial_b5")          # some image is quiet before the batch is
NO_ORACLE = ("shared_two_groups",)          # the oracle's stop is over one call's images: (a) and (b) only

INFO_COLS = {"stop_at": 0, "initial_up_cost": 1, "initial_latitude_cost": 2, "initial_cost": 3, "final_up_cost": 4,
             "final_latitude_cost": 5, "final_cost": 6, "roll_uncertainty": 7, "pitch_uncertainty": 8,
             "gravity_uncertainty": 9, "focal_uncertainty": 10, "vfov_uncertainty": 11, "lambda": 13, "step_failures": 14}
COST_KEYS = ("initial_up_cost", "initial_latitude_cost", "initial_cost", "final_up_cost", "final_latitude_cost", "final_cost")
SIGMA_KEYS = ("roll_uncertainty", "pitch_uncertainty", "gravity_uncertainty", "focal_uncertainty", "vfov_uncertainty")
BIT_KEYS = ("camera", "gravity", "stop_at") + COST_KEYS + SIGMA_KEYS + ("covariance", "lambda", "step_failures")


def case(name: str) -> dict:
    c = {"shape": SHAPE, "groups": 0, **CASES[name], "name": name}
    c["B"] = c["groups"] * c["frames"] if c["groups"] else len(c["images"])
    c.setdefault("natural", c["stop"])
    assert c["stop"] == min(c["natural"], c["num_steps"]) and c["B"] <= 8 and 1e-5 <= c["tol"] <= 1e-2, name
    return c


def fields(c: dict) -> dict:
    """The case's inputs as numpy arrays (oracle/synth.py; a shared-intrinsics case: `groups` groups of `frames` frames)."""
    from oracle import synth
    H, W = c["shape"]
    if not c["groups"]:
        return synth.make_fields(c["seed"], c["images"], c["model"], H, W)[0]
    parts = [synth.make_shared_group(c["seed"], g, c["model"], H, W, frames=c["frames"])[0] for g in range(c["groups"])]
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def conf(c: dict, **over) -> dict:
    """The LMOptimizer conf of the case's early-stopped solve; conf(c, num_steps=s, early_stop=False) is its fixed twin."""
    out = {"camera_model": c["model"], "atol": c["tol"], "rtol": c["tol"], "num_steps": c["num_steps"], "early_stop": True}
    if c["groups"]:
        out |= {"shared_intrinsics": True, "group_size": c["frames"] if c["groups"] > 1 else None}
    return {**out, **over}


def from_rows(cam: np.ndarray, grav: np.ndarray, info: np.ndarray) -> dict:
    """A result dict, keyed like the oracle's, from the raw rows of a HIP call (include/gclm.h: GCLM_INFO_*)."""
    P = int(info[0, 12])
    out = {"camera": cam, "gravity": grav, "covariance": info[:, 16:16 + P * P].reshape(-1, P, P).copy()}
    out.update({k: info[:, col].copy() for k, col in INFO_COLS.items()})
    return out


# ------------------------------------------------------------------ the oracle's view of a case

def _parts(c: dict):
    return [np.arange(g * c["frames"], (g + 1) * c["frames"]) for g in range(c["groups"])] if c["groups"] else [np.arange(c["B"])]


def oracle_solve(oracle, c: dict, data: dict, cf: dict, precision: str, **kw) -> dict:
    """The oracle on the case, one call per shared-intrinsics group (a group is one arrow-head system, and the oracle's
    stop is over the images of one call: a conf with early_stop on is for cases of one part only)."""
    parts = _parts(c)
    assert len(parts) == 1 or not cf["early_stop"]
    cf = {k: v for k, v in cf.items() if k != "group_size"}
    outs = [oracle.solve({k: v[idx] for k, v in data.items()}, cf, precision=precision, **kw) for idx in parts]
    return {k: np.concatenate([o[k] for o in outs]) for k in outs[0] if k != "trace"}


def oracle_fixed(oracle, c: dict, data: dict, steps: int, precision: str = "f64") -> dict:
    return oracle_solve(oracle, c, data, conf(c, num_steps=steps, early_stop=False), precision)


def cost_sequence(oracle, c: dict, data: dict, n: int, precision: str) -> np.ndarray:
    """(n + 1, B): the mean cost at theta_0 .. theta_n of the fixed-length solve, in double from the oracle's trace."""
    cf = {k: v for k, v in conf(c, num_steps=n + 1, early_stop=False).items() if k != "group_size"}
    seqs = []
    for idx in _parts(c):
        t = oracle.solve({k: v[idx] for k, v in data.items()}, cf, precision=precision, training=True, trace=True)["trace"]
        seqs.append(t["cost_up"][:n + 1] + t["cost_lat"][:n + 1])
    return np.concatenate(seqs, axis=1)


def stop_ratios(costs: np.ndarray, tol: float) -> np.ndarray:
    """(n, B): row k - 1 holds r = |cost_k - cost_{k-1}| / (atol + rtol |cost_{k-1}|) of comparison k = 1 .. n."""
    return np.abs(costs[1:] - costs[:-1]) / (tol + tol * np.abs(costs[:-1]))


def stop_step(r: np.ndarray, num_steps: int) -> int:
    """infos["stop_at"]: the first comparison at which EVERY image is quiet, else num_steps."""
    quiet = np.flatnonzero((r[:num_steps] <= 1).all(1))
    return int(quiet[0]) + 1 if quiet.size else num_steps


# ------------------------------------------------------------------ the comparison functions

def bit_differences(a: dict, b: dict) -> list:
    """(b): the keys on which two results differ in any bit -- camera, gravity, stop_at, every cost column, the sigmas, the
    covariance, lambda and step_failures.  Empty: the same answer."""
    return [k for k in BIT_KEYS if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True)]


def gate_ratios(out: dict, ref: dict) -> dict:
    """(c): the distances of a result from the float64 oracle's, each over its gate -- parameters and costs over the
    project's end-of-solve gates (conftest.compare_result with test_gpu_parity.TOL), the covariance over COV_EPS x the
    condition number of the scaled Hessian (test_step_parity.check_steps).  <= 1 everywhere: the gate is met."""
    m = measure_result(out, ref)
    ratios = {k: m[k] / TOL[k] for k in ("focal", "dist", "gravity", "cost", "unc")}
    Cr, Ch = ref["covariance"].astype(np.float64), np.asarray(out["covariance"], np.float64)
    Hr = np.linalg.inv(Cr)
    d = 1 / np.sqrt(np.abs(np.einsum("bii->bi", Hr)))
    kappa = np.linalg.cond(Hr * d[:, :, None] * d[:, None, :])
    sd = np.sqrt(np.abs(np.einsum("bii->bi", Cr)))
    ecov = (np.abs(Ch - Cr) / (sd[:, :, None] * sd[:, None, :])).max((1, 2)) / kappa
    ratios["cov"] = float(ecov.max() / COV_EPS)
    return ratios


PARAM_GATES, COST_GATES, COV_GATES = ("focal", "dist", "gravity"), ("cost",), ("cov",)


def worst(ratios: dict, keys=None) -> float:
    return max(v for k, v in ratios.items() if keys is None or k in keys)


def assert_case_result(tag: str, c: dict, out: dict, fixed: dict, ref64: dict = None) -> dict:
    """What tests/test_early_stop.py asserts of an early-stopped solve `out`: (a) stop_at is the table's on every image,
    (b) `out` equals `fixed`, the same solver's {num_steps: stop, early_stop: False}, bit for bit, (c) `out` meets the
    gates against the float64 oracle's fixed-length solve `ref64` (None: a case the oracle does not apply to).  Returns the
    ratios of (c)."""
    assert (np.asarray(out["stop_at"]) == c["stop"]).all(), (tag, "stop_at", out["stop_at"], c["stop"])
    diff = bit_differences(out, fixed)
    assert not diff, (tag, "differs from its fixed-length twin in", diff, {k: (out[k], fixed[k]) for k in diff if k != "covariance"})
    if ref64 is None:
        return {}
    ratios = gate_ratios(out, ref64)
    print(tag, {k: float(f"{v:.3g}") for k, v in ratios.items()})
    assert np.isfinite(list(ratios.values())).all() and worst(ratios) <= 1, (tag, ratios)
    assert np.array_equal(out["step_failures"], ref64["step_failures"]), (tag, out["step_failures"], ref64["step_failures"])
    return ratios
