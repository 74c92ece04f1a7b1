"""-m gpu: an early-stopped HIP solve against the fixed-length solve of the same steps, at stops where the state still moves.

early_stop = True with 30 steps is the library's default, and six places must agree on it: stop_fired_before
(gclm_internal.h), first_quiet_step (gclm_device.h), update_kernel / shared_step_kernel / prep_final_kernel /
finalize_kernel (gclm_update.hip), the skip at the head of sweep_kernel and the prologue and final launch of
fused_step_kernel (gclm_pass.hip), the host loops and the pacer (gclm_api.hip).  For every case of
tests/early_stop_cases.py (proved on the CPU by tests/test_early_stop_oracle.py) and every launch path, asserted through
early_stop_cases.assert_case_result:
  (a) stop_at is the table's on every image;
  (b) the result EQUALS, bit for bit, the HIP solve with {num_steps: stop, early_stop: False} on the same handle knobs:
      camera, gravity, every cost, the sigmas, the covariance, stop_at, lambda and step_failures (raw info rows);
  (c) the result meets the project's end-of-solve gates (test_gpu_parity.TOL) and the COV_EPS x condition number
      criterion (test_step_parity) against the float64 oracle's {num_steps: stop, early_stop: False}.
Every path asserts that it was the one taken.  The worst ratio of (c) per path goes to MEASURED under early_stop/."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import MEASURED
import early_stop_cases as ec
from test_step_parity import _to_dev, hip_run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from geocalib_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


_REF = {}


def _ref64(oracle, c):
    """The float64 oracle's fixed-length solve of the case, computed once."""
    if c["name"] in ec.NO_ORACLE:
        return None
    key = (c["model"], c["seed"], str(c.get("images")), c["groups"], c["shape"], c["tol"], c["stop"])
    if key not in _REF:
        _REF[key] = ec.oracle_fixed(oracle, c, ec.fields(c), c["stop"], "f64")
    return _REF[key]


def _set_knobs(opt, dev, knobs):
    from geocalib_amd import _lib
    lib = _lib.load()
    opt.row_pairs = knobs.get("row_pairs")
    opt.paced_launches = knobs.get("paced", 0)
    h = opt._handle(dev)
    for name, fn in (("slat", lib.gclm_set_slat_plane), ("fused", lib.gclm_set_fused_steps)):
        if name in knobs:
            _lib.check(fn(h.ptr, int(knobs[name])), h.ptr, name)
    return h


def _timed(opt, h, dev, solve):
    """solve() on the handle with its sweep launches counted: (result of early_stop_cases.from_rows, what the handle says
    about the path it took)."""
    from geocalib_amd import _lib
    lib = _lib.load()
    _lib.check(lib.gclm_set_timing(h.ptr, 1), h.ptr, "gclm_set_timing")
    solve()
    torch.cuda.synchronize()
    assert opt._handle(dev) is h
    n, ms = C.c_int(0), C.c_float(0)
    _lib.check(lib.gclm_last_pass_timing(h.ptr, C.byref(n), C.byref(ms)), h.ptr, "gclm_last_pass_timing")
    cam, grav, info = (t.cpu().numpy() for t in opt._last_raw)
    return ec.from_rows(cam, grav, info), {"launches": n.value, "slat_bytes": lib.gclm_slat_plane_bytes(h.ptr)}


def _stopped(dev, cf, data_dev, knobs):
    """The early-stopped solve of conf `cf` with the handle knobs forced (test_step_parity.hip_run, which runs the fixed
    twin, with the stop left on).  Paced launches: one solve first, as the pacer's own test does."""
    from geocalib_amd import LMOptimizer
    opt = LMOptimizer(dict(cf)).eval()
    h = _set_knobs(opt, dev, knobs)
    if knobs.get("paced"):
        opt(dict(data_dev))
        torch.cuda.synchronize()
    return _timed(opt, h, dev, lambda: opt(dict(data_dev)))


def _fixed(dev, c, data_dev, knobs):
    hk = {k: v for k, v in knobs.items() if k != "paced"}          # (ignored without the stop)
    r = hip_run(dev, ec.conf(c), data_dev, c["stop"], hk)
    return ec.from_rows(r["cam"], r["grav"], r["info"]), r


def _record(name, path, ratios):
    if ratios:
        MEASURED[f"early_stop/{name}/{path}"] = {"worst_ratio": ec.worst(ratios), **{k: float(v) for k, v in ratios.items()}}


# path -> (handle knobs, one launch per step?, scratch plane expected?).  The scratch plane is forced on wherever a solve
# can keep one (it changes no bit): the one-launch-per-step path declines it (gclm_api.hip: make_plan), so the plane's
# size says which path ran, as in test_step_parity / test_update_edges.
PATHS = {
    "one_launch": ({"slat": 1}, True, False),                              # B = 1: the library's own choice
    "one_launch_paced1": ({"slat": 1, "paced": 1}, True, False),
    "one_launch_paced3": ({"slat": 1, "paced": 3}, True, False),
    "two_launch": ({"fused": 0, "slat": 1, "row_pairs": False}, False, True),
    "scalar": ({"slat": 1}, False, False),                                 # W % 4 != 0: no float4 sweep, no plane, never one launch
    "two_launch_no_plane": ({"fused": 0, "slat": 0, "row_pairs": False}, False, False),
    "row_pairs": ({"fused": 0, "slat": 1, "row_pairs": True}, False, True),
    "shared": ({"slat": 1}, False, True),
}
SINGLE = ("pinhole_s3", "pinhole_s4") + ec.TRIPLE + ("radial_quiet_then_loud", "radial_s9", "divisional_s1")
RUNS = ([(n, p) for n in SINGLE for p in ("one_launch", "two_launch")] +
        [(n, p) for n in ("pinhole_s3", "radial_quiet_then_loud") for p in ("one_launch_paced1", "one_launch_paced3")] +
        [("simple_radial_scalar", "scalar"), ("pinhole_b5", "two_launch"), ("simple_radial_b5", "two_launch"),
         ("simple_radial_b5", "two_launch_no_plane"), ("radial_b5", "row_pairs"), ("divisional_b5", "row_pairs"),
         ("shared_one_group", "shared"), ("shared_two_groups", "shared")])


@pytest.mark.parametrize("name,path", RUNS)
def test_early_stop_equals_the_fixed_length_solve(dev, oracle, name, path):
    c = ec.case(name)
    knobs, one_launch, plane = PATHS[path]
    data = ec.fields(c)
    data_dev = _to_dev(data, dev)
    out, took = _stopped(dev, ec.conf(c), data_dev, knobs)
    fixed, ftook = _fixed(dev, c, data_dev, knobs)
    # the path: every loop sweep is issued (and skipped on the device after the stop) unless the launches are paced
    assert (took["slat_bytes"] > 0) == plane and (ftook["slat_bytes"] > 0) == plane, (took, ftook["slat_bytes"])
    assert ftook["launches"] == c["stop"] + 1, ftook["launches"]
    if knobs.get("paced") and c["stop"] + knobs["paced"] + 3 < c["num_steps"] + 1:
        assert c["stop"] + 1 <= took["launches"] <= c["stop"] + knobs["paced"] + 3, took      # the pacer's own bound
    else:
        assert took["launches"] == c["num_steps"] + 1, took
    if one_launch:
        assert c["B"] == 1 and c["shape"][1] % 4 == 0
    if path == "scalar":
        assert c["shape"][1] % 4 != 0
    if c["shape"] == (96, 128):
        assert ftook["chunks"] > 1, ftook["chunks"]          # more than one record per image
    if path == "row_pairs":          # the row-pair walk ran: its sums differ from the one-row walk's in the last bits
        one_row = hip_run(dev, ec.conf(c), data_dev, c["stop"], {**knobs, "row_pairs": False})
        assert not np.array_equal(one_row["info"][:, 6], fixed["final_cost"])
    ratios = ec.assert_case_result(f"early_stop/{name}/{path}", c, out, fixed, _ref64(oracle, c))
    _record(name, path, ratios)


def test_early_stop_through_the_stop_communicator(dev, oracle):
    """calibrate_sharded with a one-rank RcclComm and GCLM_FORCE_COLLECTIVES=1 (the set-up of test_gpu_parity.py::
    test_sharded_early_stop_through_the_stop_communicator): the counters travel through the all-reduce of every step, the
    stop is still the batch's, and the result is the fixed-length solve's bit for bit."""
    from geocalib_amd import LMOptimizer
    from geocalib_amd.parallel import RcclComm, calibrate_sharded
    c = ec.case("pinhole_b5")
    data_dev = _to_dev(ec.fields(c), dev)
    comm = RcclComm(RcclComm.unique_id(), 1, 0, 0)
    opt = LMOptimizer(ec.conf(c)).eval()
    h = _set_knobs(opt, dev, {})
    os.environ["GCLM_FORCE_COLLECTIVES"] = "1"
    try:
        out, took = _timed(opt, h, dev, lambda: calibrate_sharded(opt, data_dev, c["B"], comm=comm))
    finally:
        os.environ.pop("GCLM_FORCE_COLLECTIVES", None)
    assert took["launches"] == c["num_steps"] + 1, took
    fixed, _ = _fixed(dev, c, data_dev, {})
    ec.assert_case_result("early_stop/pinhole_b5/sharded", c, out, fixed)


@pytest.mark.parametrize("path", ["one_launch", "one_launch_paced3", "two_launch"])
def test_counters_do_not_reach_the_next_solve(dev, oracle, path):
    """One optimiser, one handle: X (stops at 2), Y (stops six steps later), X again.  Both X results are the same bits
    and Y is what a fresh handle gives -- a counter, a `stopped` flag or a progress word left over from the previous
    solve would move one of them.  Each is also held to (a), (b) and (c)."""
    from geocalib_amd import LMOptimizer
    x, y = ec.case("radial_x"), ec.case("radial_y")
    knobs = PATHS[path][0]
    dx, dy = _to_dev(ec.fields(x), dev), _to_dev(ec.fields(y), dev)
    opt = LMOptimizer(ec.conf(x)).eval()
    h = _set_knobs(opt, dev, knobs)
    got = [_timed(opt, h, dev, lambda d=d: opt(dict(d)))[0] for d in (dx, dy, dx)]
    fresh_y, _ = _stopped(dev, ec.conf(y), dy, knobs)
    assert not ec.bit_differences(got[0], got[2]), ec.bit_differences(got[0], got[2])
    assert not ec.bit_differences(got[1], fresh_y), ec.bit_differences(got[1], fresh_y)
    for c, d, out in ((x, dx, got[0]), (y, dy, got[1]), (x, dx, got[2])):
        fixed, _ = _fixed(dev, c, d, knobs)
        _record(c["name"], f"{path}/same_handle", ec.assert_case_result(f"early_stop/{c['name']}/{path}/same_handle", c, out, fixed, _ref64(oracle, c)))
