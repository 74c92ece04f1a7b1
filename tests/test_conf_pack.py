"""-m gpu: the packed confidence plane of the pinhole solve (include/gclm.h: gclm_set_conf_pack; gclm_pass.hip: row_math, CPACK).

With the plane forced on (mode 1) the first sweep of a solve packs the two confidence planes into one word per pixel and
every later sweep reads that plane.  The format is restated in numpy by tests/test_conf_pack_format.py; here the HIP solve
is held to it BIT FOR BIT (camera, gravity, every cost, the sigmas, the covariance, lambda, step_failures:
early_stop_cases.bit_differences):
  1  confidences that are float32(q) * float32(1 / 65535) already: mode 1 == mode 0;
  2  U(0, 1) confidences c: mode 1 on c == mode 0 on decode(encode(c)) -- this pins the encoder's rounding;
  3  a confidence outside [0, 1] or a NaN flags its image (gclm_conf_pack_fallbacks counts them), a clean image beside them
     still satisfies 2, and the flagged images meet the float64 step gate of tests/test_step_parity.py;
  4  solves the plane is not instantiated for take no plane under mode 1 and return mode 0's bits;
  5  the built-in rule (mode -1) takes no plane at these sizes;  6  a refused plane means an unpacked solve, not an error;
  7  a handle that solved A then B returns B of a fresh handle;  8  two side streams equal one;  9  an early-stopped solve
     equals its fixed-length twin (tests/early_stop_cases.py).
Shapes, B = 3: 48x64 (the issue's one-chunk shape; at this batch size the planner cuts it into 2 chunks, so 16x64 -- truly one
chunk -- rides along), 50x68 (two chunks per image, the last one ragged: 20 of 30 rows), 6x640 (a wave's tile spans two rows);
independent and shared intrinsics (one group of 3), log focal on and off.  Every case asserts the path it names."""
import ctypes as C

import numpy as np
import pytest
import torch

import early_stop_cases as ec
from test_conf_pack_format import roundtrip
from test_step_oracle import TAU_FLOOR, TAU_REL, step_gate
from test_step_parity import _oracle_step, _to_dev

pytestmark = pytest.mark.gpu

B = 3
SHAPES = {"48x64": (48, 64), "16x64_one_chunk": (16, 64), "50x68_ragged": (50, 68), "6x640_tile_spans_rows": (6, 640)}
STEPS = 5
MODES = {None: -1, False: 0, True: 1}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from geocalib_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


_FIELDS = {}


def fields(shape, shared, model="pinhole", n=B, seed=7):
    """numpy fields of the case, generated once and never modified (callers copy what they change)."""
    key = (shape, shared, model, n, seed)
    if key not in _FIELDS:
        from oracle import synth
        if shared:
            _FIELDS[key] = synth.make_shared_group(seed, 0, model, *shape, frames=n)[0]
        else:
            _FIELDS[key] = synth.make_fields(seed, range(n), model, *shape)[0]
    return {k: v for k, v in _FIELDS[key].items()}


def with_conf(data, fn):
    out = dict(data)
    for k in ("up_confidence", "latitude_confidence"):
        if k in out:
            out[k] = fn(out[k])
    return out


def rounded_in_range(c):
    ok = (c >= 0) & (c <= 1)
    return np.where(ok, roundtrip(np.where(ok, c, 0).astype(np.float32)), c).astype(np.float32)


def conf_of(shared, logf=True, model="pinhole", **over):
    c = {"camera_model": model, "num_steps": STEPS, "early_stop": False, "use_log_focal": logf}
    if shared:
        c |= {"shared_intrinsics": True, "group_size": None}
    return {**c, **over}


def solve(dev, conf, data_dev, mode, fused=0, limit=None, opt=None, overlap=1):
    """One HIP solve with gclm_set_conf_pack(mode) (and the one-launch-per-step path off unless asked for); returns the
    result keyed like the oracle's and what the handle says about the plane."""
    from geocalib_amd import LMOptimizer, _lib
    lib = _lib.load()
    if opt is None:
        opt = LMOptimizer(dict(conf)).eval()
    opt.conf_pack = mode
    opt.overlap_streams = overlap
    h = opt._handle(dev)
    assert h.conf_pack == MODES[mode]
    _lib.check(lib.gclm_set_fused_steps(h.ptr, fused), h.ptr, "gclm_set_fused_steps")
    if limit is not None:
        _lib.check(lib.gclm_set_slat_plane_limit(h.ptr, limit), h.ptr, "gclm_set_slat_plane_limit")
    opt(dict(data_dev))
    torch.cuda.synchronize()
    assert opt._handle(dev) is h
    n = C.c_int(-1)
    _lib.check(lib.gclm_conf_pack_fallbacks(h.ptr, C.byref(n)), h.ptr, "gclm_conf_pack_fallbacks")
    cam, grav, info = (t.cpu().numpy() for t in opt._last_raw)
    took = {"bytes": lib.gclm_conf_pack_bytes(h.ptr), "fallbacks": n.value, "workspace": lib.gclm_workspace_bytes(h.ptr),
            "slat_bytes": lib.gclm_slat_plane_bytes(h.ptr), "opt": opt, "handle": h}
    return ec.from_rows(cam, grav, info), took


def same(a, b):
    return ec.bit_differences(a, b)


def plane_bytes(data):
    return int(data["latitude_field"].size) * 4


CASES = [(s, sh, lf) for s in SHAPES for sh in (False, True) for lf in (True, False)]
IDS = [f"{s}-{'shared' if sh else 'independent'}-{'logf' if lf else 'linf'}" for s, sh, lf in CASES]


def test_the_shapes_are_cut_as_the_docstring_says(dev):
    from geocalib_amd import LMOptimizer, _lib
    lib = _lib.load()
    h = LMOptimizer(conf_of(False)).eval()._handle(dev)
    cut = {}
    for name, (H, W) in SHAPES.items():
        rows, chunks = C.c_int(0), C.c_int(0)
        _lib.check(lib.gclm_plan_cut(h.ptr, B, H, W, 1, C.byref(rows), C.byref(chunks)), h.ptr, "gclm_plan_cut")
        cut[name] = (rows.value, chunks.value)
    print(cut)
    assert cut["16x64_one_chunk"][1] == 1
    rows, chunks = cut["50x68_ragged"]
    assert chunks >= 2 and 50 % rows != 0
    assert cut["6x640_tile_spans_rows"][1] >= 2


@pytest.mark.parametrize("shape,shared,logf", CASES, ids=IDS)
def test_representable_confidences_give_the_unpacked_bits(dev, shape, shared, logf):
    data = with_conf(fields(SHAPES[shape], shared), roundtrip)
    data_dev = _to_dev(data, dev)
    cf = conf_of(shared, logf)
    packed, took = solve(dev, cf, data_dev, True)
    assert took["bytes"] == plane_bytes(data) and took["fallbacks"] == 0, took
    plain, took0 = solve(dev, cf, data_dev, False)
    assert took0["bytes"] == 0 and took["workspace"] == took0["workspace"] + took["bytes"], (took, took0)
    assert not same(packed, plain), same(packed, plain)


@pytest.mark.parametrize("shape,shared,logf", CASES, ids=IDS)
def test_arbitrary_confidences_give_the_bits_of_their_round_trip(dev, shape, shared, logf):
    rng = np.random.default_rng(11)
    data = with_conf(fields(SHAPES[shape], shared), lambda c: rng.random(c.shape, dtype=np.float32))
    cf = conf_of(shared, logf)
    packed, took = solve(dev, cf, _to_dev(data, dev), True)
    assert took["bytes"] == plane_bytes(data) and took["fallbacks"] == 0, took
    plain, _ = solve(dev, cf, _to_dev(with_conf(data, roundtrip), dev), False)
    assert not same(packed, plain), same(packed, plain)
    exact, _ = solve(dev, cf, _to_dev(data, dev), False)
    assert same(packed, exact)                  # (the rounding is visible in the bits: the comparison above can fail)


def _flagged_batch():
    """Four images of 50x68 (two chunks of 30 rows): 1.5 in chunk 0 of image 0, -0.1 in chunk 1 of image 1, a NaN in chunk 1
    of image 2; image 3 is clean."""
    data = fields(SHAPES["50x68_ragged"], False, n=4, seed=21)
    up, lat = data["up_confidence"].copy(), data["latitude_confidence"].copy()
    up[0, 3, 5] = 1.5
    lat[1, 44, 61] = -0.1
    up[2, 31, 0] = np.nan
    return {**data, "up_confidence": up, "latitude_confidence": lat}


def test_out_of_range_confidences_flag_their_image_only(dev):
    data = _flagged_batch()
    cf = conf_of(False)
    packed, took = solve(dev, cf, _to_dev(data, dev), True)
    assert took["bytes"] == plane_bytes(data) and took["fallbacks"] == 3, took
    plain, _ = solve(dev, cf, _to_dev(with_conf(data, rounded_in_range), dev), False)
    for k in ec.BIT_KEYS:                       # the clean image: the bits of its round trip, as if it were alone
        assert np.array_equal(np.asarray(packed[k])[3], np.asarray(plain[k])[3], equal_nan=True), k
    # the next solve on the handle starts from clean flags
    clean = with_conf(fields(SHAPES["50x68_ragged"], False, n=4, seed=21), roundtrip)
    _, took2 = solve(dev, cf, _to_dev(clean, dev), True, opt=took["opt"])
    assert took2["fallbacks"] == 0 and took2["bytes"] == took["bytes"], took2


@pytest.mark.parametrize("k", [1, 2, 3, 10])
def test_flagged_images_meet_the_float64_step_gate(dev, oracle, k):
    data = _flagged_batch()
    data_dev = _to_dev(data, dev)
    cf = {"camera_model": "pinhole", "fix_lambda": True}
    runs = {}
    for s in (k - 1, k):
        runs[s], took = solve(dev, conf_of(False, num_steps=s, fix_lambda=True), data_dev, True)
        assert took["fallbacks"] == (3 if s >= 1 else 0), (s, took)      # (no LM step: one sweep, nothing to pack)
    r0, r1 = runs[k - 1], runs[k]
    start = (r0["camera"], r0["gravity"])
    ref64 = _oracle_step(oracle, cf, data, start, r0["lambda"].copy(), "f64")
    ratio = step_gate("pinhole", start, (r1["camera"], r1["gravity"]), (ref64["camera"], ref64["gravity"]), TAU_REL, TAU_FLOOR)
    print(f"conf_pack flagged images, step {k}: worst ratio per image {ratio.max(1)}")
    assert np.isfinite(ratio).all() and (ratio <= 1).all(), (k, ratio.max(0), np.argwhere(ratio > 1)[:8])
    hip_failed = r1["step_failures"] > r0["step_failures"]
    assert np.array_equal(hip_failed, ref64["step_failures"] > 0), (hip_failed, ref64["step_failures"])


NOT_INSTANTIATED = ("four_planes", "latitude_only", "simple_radial", "one_launch_per_step", "misaligned", "scalar_width",
                    "sin_latitude_plane")


@pytest.mark.parametrize("what", NOT_INSTANTIATED)
def test_mode_1_leaves_the_other_paths_alone(dev, what):
    from geocalib_amd import _lib
    lib = _lib.load()
    shape = (48, 66) if what == "scalar_width" else (48, 64)
    model = "simple_radial" if what == "simple_radial" else "pinhole"
    data = fields(shape, False, model=model)
    if what == "four_planes":
        data.pop("up_confidence")
    elif what == "latitude_only":
        data = {k: data[k] for k in ("latitude_field", "latitude_confidence")}
    data_dev = _to_dev(data, dev, unaligned=what == "misaligned")
    cf = conf_of(False, model=model)
    fused = 1 if what == "one_launch_per_step" else 0
    outs = {}
    for mode in (True, False):
        opt = None
        if what == "sin_latitude_plane":             # pinhole's own scratch plane of sin(latitude), forced: never both planes
            from geocalib_amd import LMOptimizer
            opt = LMOptimizer(dict(cf)).eval()
            _lib.check(lib.gclm_set_slat_plane(opt._handle(dev).ptr, 1), None, "gclm_set_slat_plane")
        outs[mode], took = solve(dev, cf, data_dev, mode, fused=fused, opt=opt)
        assert took["bytes"] == 0 and took["fallbacks"] == 0, (what, mode, took)
        assert (took["slat_bytes"] > 0) == (what in ("sin_latitude_plane", "simple_radial")), took    # (simple_radial's own)
    assert not same(outs[True], outs[False]), (what, same(outs[True], outs[False]))


def test_the_plan_query_states_the_built_in_rule(dev):
    """gclm_plan_conf_pack: what a solve of that shape would do (no device work).  The built-in rule packs the flagship batch
    and leaves 832 images of 640x480 alone; mode 1 packs wherever the kernels exist; mode 0 never."""
    from geocalib_amd import LMOptimizer, _lib
    lib = _lib.load()
    opt = LMOptimizer(conf_of(False, num_steps=20)).eval()
    h = opt._handle(dev)
    def q(*a):
        out = C.c_int(-7)
        rc = lib.gclm_plan_conf_pack(h.ptr, *a, C.byref(out))
        return out.value if rc == 0 else rc

    assert q(1024, 480, 640, 1, 1, 21) == 1 and q(832, 480, 640, 1, 1, 21) == 0 and q(3, 48, 64, 1, 1, 21) == 0
    assert q(1024, 480, 640, 1, 1, 5) == 0 and q(1024, 480, 640, 0, 1, 21) == 0 and q(1024, 480, 640, 1, 0, 21) == 0
    opt.conf_pack = True
    assert opt._handle(dev) is h and q(3, 48, 64, 1, 1, 2) == 0          # three small images: one launch per LM step, no plane
    _lib.check(lib.gclm_set_fused_steps(h.ptr, 0), h.ptr, "gclm_set_fused_steps")
    assert opt._handle(dev) is h and q(3, 48, 64, 1, 1, 2) == 1 and q(3, 48, 64, 1, 1, 1) == 0 and q(3, 48, 66, 1, 1, 21) == 0
    opt.conf_pack = False
    assert opt._handle(dev) is h and q(1024, 480, 640, 1, 1, 21) == 0
    assert lib.gclm_plan_conf_pack(None, 1, 1, 1, 1, 1, 1, C.byref(C.c_int(0))) == -1 and q(0, 48, 64, 1, 1, 21) == -3
    assert lib.gclm_plan_conf_pack(h.ptr, 1, 1, 1, 1, 1, 1, None) == -1


@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_built_in_rule_does_not_pack_small_solves(dev, shape):
    rng = np.random.default_rng(3)
    data_dev = _to_dev(with_conf(fields(SHAPES[shape], False), lambda c: rng.random(c.shape, dtype=np.float32)), dev)
    cf = conf_of(False, num_steps=20)
    auto, took = solve(dev, cf, data_dev, None)
    assert took["bytes"] == 0 and took["fallbacks"] == 0, took
    plain, _ = solve(dev, cf, data_dev, False)
    assert not same(auto, plain), same(auto, plain)


def test_a_refused_plane_means_an_unpacked_solve(dev):
    rng = np.random.default_rng(4)
    data = with_conf(fields(SHAPES["48x64"], False), lambda c: rng.random(c.shape, dtype=np.float32))
    data_dev = _to_dev(data, dev)
    cf = conf_of(False)
    plain, took0 = solve(dev, cf, data_dev, False)
    capped, took = solve(dev, cf, data_dev, True, limit=plane_bytes(data) - 1)
    assert took["bytes"] == 0 and took["workspace"] == took0["workspace"] and took["fallbacks"] == 0, took
    assert not same(capped, plain), same(capped, plain)
    again, took = solve(dev, cf, data_dev, True, opt=took["opt"])              # remembered: not retried per call, still no error
    assert took["bytes"] == 0 and not same(again, plain)
    # a limit the plane fits under: the next solve has it
    packed, took = solve(dev, cf, data_dev, True, limit=plane_bytes(data), opt=took["opt"])
    assert took["bytes"] == plane_bytes(data), took
    ref, _ = solve(dev, cf, _to_dev(with_conf(data, roundtrip), dev), False)
    assert not same(packed, ref), same(packed, ref)


def test_a_reused_handle_returns_what_a_fresh_one_does(dev):
    cf = conf_of(False)
    a = _flagged_batch()                                                       # 4 images of 50x68, three of them flagged
    rng = np.random.default_rng(9)
    b = with_conf(fields(SHAPES["48x64"], False, seed=5), lambda c: rng.random(c.shape, dtype=np.float32))
    b_dev = _to_dev(b, dev)
    fresh, took = solve(dev, cf, b_dev, True)
    assert took["bytes"] == plane_bytes(b) and took["fallbacks"] == 0
    _, took_a = solve(dev, cf, _to_dev(a, dev), True)
    assert took_a["fallbacks"] == 3
    reused, took_b = solve(dev, cf, b_dev, True, opt=took_a["opt"])
    assert took_b["handle"] is took_a["handle"] and took_b["bytes"] == plane_bytes(a) and took_b["fallbacks"] == 0, took_b
    assert not same(reused, fresh), same(reused, fresh)


def test_two_side_streams_equal_one(dev):
    from geocalib_amd import LMOptimizer
    rng = np.random.default_rng(13)
    data = with_conf(fields(SHAPES["50x68_ragged"], False, n=4), lambda c: rng.random(c.shape, dtype=np.float32))
    data_dev = _to_dev(data, dev)
    cf = conf_of(False)
    one, took = solve(dev, cf, data_dev, True, overlap=1)
    assert took["bytes"] == plane_bytes(data)
    from geocalib_amd import _lib
    lib = _lib.load()
    opt = LMOptimizer(dict(cf)).eval()
    opt._OVERLAP_MIN_IMAGES = 1                                                # (parts of two images each)
    opt.conf_pack = True
    opt.overlap_streams = 2
    assert opt._overlap_parts(4, *SHAPES["50x68_ragged"]) == 2
    opt(dict(data_dev))                                                        # creates the side streams' handles ...
    torch.cuda.synchronize()
    assert len(opt._handles) >= 2
    for h in opt._handles.values():                                            # ... which then leave the one-launch-per-step path
        _lib.check(lib.gclm_set_fused_steps(h.ptr, 0), h.ptr, "gclm_set_fused_steps")
    opt(dict(data_dev))
    torch.cuda.synchronize()
    cam, grav, info = (t.cpu().numpy() for t in opt._last_raw)
    two = ec.from_rows(cam, grav, info)
    packed = sorted(lib.gclm_conf_pack_bytes(h.ptr) for h in opt._handles.values())
    assert packed[-2:] == [plane_bytes(data) // 2] * 2, packed                 # both parts packed their two images
    assert not same(two, one), same(two, one)


@pytest.mark.parametrize("name", ["pinhole_s4", "pinhole_b5"])
def test_early_stop_equals_its_fixed_length_twin(dev, oracle, name):
    c = ec.case(name)
    data = ec.fields(c)
    data_dev = _to_dev(data, dev)
    out, took = solve(dev, ec.conf(c), data_dev, True)
    fixed, ftook = solve(dev, ec.conf(c, num_steps=c["stop"], early_stop=False), data_dev, True)
    assert took["bytes"] == plane_bytes(data) == ftook["bytes"] and took["fallbacks"] == 0, (took, ftook)
    ref64 = ec.oracle_fixed(oracle, c, data, c["stop"], "f64")
    ec.assert_case_result(f"conf_pack/{name}", c, out, fixed, ref64)
