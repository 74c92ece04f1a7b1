"""CPU: the early-stop case table (tests/early_stop_cases.py) is what it claims to be, before anything runs on a card.

Per case, in the float32 and the float64 oracle (the measured values are printed):
  margin     every comparison before the stop is loud for some image (r >= LOUD), the one at the stop is quiet for every
             image (r <= QUIET), both oracles stop there -- derived, not tuned: see early_stop_cases;
  decisive   theta_{s-1} and theta_{s+1}, the costs and the covariance at each, miss theta_s by >= DECISIVE gates of the
             comparison the GPU module calls: an off-by-one cannot hide;
  honest     the float32 oracle at the stop is within F32_ROOM of the gate of the float64 one (this is what keeps
             simple_divisional to its first step and to well-conditioned draws: the others differ by up to 360 gates);
  identity   the oracle's early-stopped solve equals its own fixed-length solve of `stop` steps bit for bit, lambda and
             step_failures included: the property tests/test_early_stop.py holds HIP to.
And the comparison has power: results with one plausible defect of the stop logic, built from the oracle's own states --
theta_{s+1} (the tentative state kept), theta_{s-1} (the wrong state buffer), stop_at off by one, every image frozen at
its own first quiet step, the final costs or the covariance of the neighbouring state, lambda one update behind -- all
fail early_stop_cases.assert_case_result."""
import functools

import numpy as np
import pytest

import early_stop_cases as ec

NAMES = list(ec.CASES)
WITH_ORACLE = [n for n in NAMES if n not in ec.NO_ORACLE]
N_SEQ = 13          # comparisons looked at: past the latest stop of the table


@pytest.fixture(scope="module", autouse=True)
def _built(oracle):
    return oracle


@functools.lru_cache(maxsize=None)
def _data(name):
    return ec.fields(ec.case(name))


@functools.lru_cache(maxsize=None)
def _fixed(name, steps, precision="f64"):
    from oracle import lm_oracle
    return ec.oracle_fixed(lm_oracle, ec.case(name), _data(name), steps, precision)


@functools.lru_cache(maxsize=None)
def _ratios(name, precision):
    from oracle import lm_oracle
    c = ec.case(name)
    return ec.stop_ratios(ec.cost_sequence(lm_oracle, c, _data(name), N_SEQ, precision), c["tol"])


def test_the_table_covers_what_it_is_there_for():
    cases = [ec.case(n) for n in NAMES]
    stops = {c["stop"] for c in cases}
    assert {1, 2} <= stops and any(s % 2 and s > 1 for s in stops) and any(s % 2 == 0 and s > 2 for s in stops) and max(stops) >= 7
    assert {c["model"] for c in cases} == {"pinhole", "simple_radial", "radial", "simple_divisional"}
    assert any(c["shape"] == (47, 63) for c in cases) and any(c["shape"] == (96, 128) for c in cases)
    assert all(c["shape"] in ((48, 64), (47, 63), (96, 128)) for c in cases)
    n5, n4, n3 = (ec.case(n) for n in ec.TRIPLE)
    s = n5["natural"]
    assert (n5["num_steps"], n4["num_steps"], n3["num_steps"]) == (s + 1, s, s - 1) and n4["natural"] == n3["natural"] == s
    x, y = ec.case("radial_x"), ec.case("radial_y")
    assert ec.conf(x) == ec.conf(y) and y["stop"] >= x["stop"] + 4
    assert ec.case("shared_one_group")["groups"] == 1 and ec.conf(ec.case("shared_one_group"))["group_size"] is None
    two = ec.case("shared_two_groups")
    assert (two["groups"], two["frames"]) == (2, 3) and ec.conf(two)["group_size"] == 3


@pytest.mark.parametrize("name", NAMES)
def test_margin(name):
    c = ec.case(name)
    n, s = c["natural"], c["stop"]
    for precision in ("f64", "f32"):
        r = _ratios(name, precision)
        loud = r[:n - 1].max(1)                      # the loudest image of every comparison before the natural stop
        print(f"{name} {precision}: loudest r before the stop {np.round(loud, 2).tolist()}, r at the stop {np.round(r[n - 1], 3).tolist()}")
        assert (loud >= ec.LOUD).all(), (name, precision, loud)
        assert (r[n - 1] <= ec.QUIET).all(), (name, precision, r[n - 1])
        assert ec.stop_step(r, c["num_steps"]) == s
        if name not in ec.NO_ORACLE:          # what the oracle itself compared (its stop is over the images of one call)
            assert (_fixed(name, s, precision)["stop_at"] == s).all()
            assert (_fixed(name, n + 1, precision)["stop_at"] == n).all()
    if name == "radial_quiet_then_loud":
        after = _ratios(name, "f64")[s:s + 3, 0]
        assert (after >= ec.LOUD).all(), after          # louder steps follow the quiet one
    if name in ec.BATCHES:
        r = _ratios(name, "f64")[:s - 1]
        quiet, moving = r <= 1, r >= ec.LOUD
        assert (quiet.any(1) & moving.any(1)).any(), name          # one image quiet while another still moves
        assert (quiet.sum(0) >= 2).any(), (name, quiet.sum(0))     # an image quiet for two or more steps before the stop


def test_two_group_stop_is_over_both_groups():
    """The stop of two groups in one call: the first step at which every frame of BOTH is quiet in the oracle's
    fixed-length cost sequences of the two parts -- which need not be the later of the parts' own stops."""
    c = ec.case("shared_two_groups")
    r = _ratios("shared_two_groups", "f64")
    parts = [r[:, :c["frames"]], r[:, c["frames"]:]]
    own = [ec.stop_step(p, c["num_steps"]) for p in parts]
    both = ec.stop_step(r, c["num_steps"])
    print("two groups: own stops", own, "batch stop", both)
    assert both == c["stop"] >= max(own)


@pytest.mark.parametrize("name", NAMES)
def test_decisive(name):
    s = ec.case(name)["stop"]
    at = _fixed(name, s)
    for k in (s - 1, s + 1):
        g = ec.gate_ratios(_fixed(name, k), at)
        got = {"parameters": ec.worst(g, ec.PARAM_GATES), "costs": ec.worst(g, ec.COST_GATES), "covariance": ec.worst(g, ec.COV_GATES)}
        print(f"{name}: theta_{k} against theta_{s}, in gates: {({q: round(v, 1) for q, v in got.items()})}")
        assert min(got.values()) >= ec.DECISIVE, (name, k, got)


@pytest.mark.parametrize("name", NAMES)
def test_honest_float32(name):
    s = ec.case(name)["stop"]
    g = ec.gate_ratios(_fixed(name, s, "f32"), _fixed(name, s, "f64"))
    print(f"{name}: float32 oracle against float64 at the stop, in gates: {({k: float(f'{v:.2g}') for k, v in g.items()})}")
    assert ec.worst(g) <= ec.F32_ROOM, (name, g)


@pytest.mark.parametrize("name", WITH_ORACLE)
def test_oracle_identity(name):
    from oracle import lm_oracle
    c = ec.case(name)
    for precision in ("f64", "f32"):
        stopped = ec.oracle_solve(lm_oracle, c, _data(name), ec.conf(c), precision)
        fixed = _fixed(name, c["stop"], precision)
        assert not ec.bit_differences(stopped, fixed), (name, precision, ec.bit_differences(stopped, fixed))
        ec.assert_case_result(f"{name}/{precision}", c, stopped, fixed, _fixed(name, c["stop"], "f64") if precision == "f64" else None)


# ------------------------------------------------------------------ mutants

def _with(result, donor, keys):
    return {**result, **{k: donor[k] for k in keys}}


def _mutants(name):
    """(label, result, the check of assert_case_result it must fail on its own) for the case."""
    c = ec.case(name)
    s = c["stop"]
    at, before, after = _fixed(name, s), _fixed(name, s - 1), _fixed(name, s + 1)
    if name in ec.NO_ORACLE:          # each part reports its own stop
        at = {**at, "stop_at": np.full(c["B"], s, np.float32)}
    state, costs = ("camera", "gravity"), ("final_up_cost", "final_latitude_cost", "final_cost")
    cov = ("covariance",) + ec.SIGMA_KEYS
    out = [("theta_next", _with(at, after, state), "gate"), ("theta_prev", _with(at, before, state), "gate"),
           ("stop_at_plus_1", {**at, "stop_at": at["stop_at"] + 1}, "stop_at"),
           ("stop_at_minus_1", {**at, "stop_at": at["stop_at"] - 1}, "stop_at"),
           ("costs_next", _with(at, after, costs), "gate"), ("costs_prev", _with(at, before, costs), "gate"),
           ("covariance_next", _with(at, after, cov), "gate"), ("covariance_prev", _with(at, before, cov), "gate")]
    if not np.array_equal(before["lambda"], at["lambda"]):          # (equal at the 1e-6 clamp, and under shared intrinsics)
        out.append(("lambda_one_behind", _with(at, before, ("lambda",)), "bits"))
    if name in ec.BATCHES:
        r = _ratios(name, "f64")
        own = [int(np.flatnonzero(r[:, b] <= 1)[0]) + 1 for b in range(c["B"])]
        assert min(own) < s
        frozen = {k: np.stack([_fixed(name, own[b])[k][b] for b in range(c["B"])]) for k in at}
        out.append(("per_image_stop", {**frozen, "stop_at": at["stop_at"]}, "gate"))
    return c, at, out


@pytest.mark.parametrize("name", NAMES)
def test_mutants_fail(name):
    c, at, mutants = _mutants(name)
    ref64 = None if name in ec.NO_ORACLE else at
    ec.assert_case_result(name, c, at, at, ref64)                                   # the unmutated result passes
    for label, result, how in mutants:
        with pytest.raises(AssertionError):
            ec.assert_case_result(f"{name}/{label}", c, result, at, ref64)
        assert ec.bit_differences(result, at), (name, label)                        # (b) sees every one of them
        if how == "gate":                                                           # ... and (c) on its own
            g = ec.gate_ratios(result, at)
            print(f"{name}/{label}: worst gate ratio {ec.worst(g):.1f}")
            assert ec.worst(g) > 1, (name, label, g)
        elif how == "stop_at":                                                      # ... and (a)
            assert (result["stop_at"] != c["stop"]).all()
    labels = [m[0] for m in mutants]
    if name in ("pinhole_s3", "pinhole_s4", "pinhole_b5", "radial_quiet_then_loud", "divisional_s1"):
        assert "lambda_one_behind" in labels, name
