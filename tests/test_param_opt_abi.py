"""CPU: gclm_param_opt without a device -- the entry points are declared, exported and bound, the default config is the
reference's default_conf, the workspace size is monotone, every invalid argument is refused before any HIP call, the float64
statement of tests/param_opt_gate.py equals the reference's float64 autograd (tests/golden/param_opt_reference.npz) and its
state machine equals torch.optim.Adam + ReduceLROnPlateau run live, the Python module refuses what it does not implement and
hands the C entries the arguments of include/gclm.h.  For the edge gates of tests/test_param_opt.py: the per-pixel statement
equals the yardstick, the yardstick equals the reference at the recorded edges (tests/golden/param_opt_edges.npz), every case is
decisive and enters the branch it is named for, and the derived bound refuses each mutant of the pass."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import geocalib_amd
from geocalib_amd import _call, _lib, perspective_opt
from abi_harness import HEADER, LLVM, assert_declared_exported_and_bound
import param_opt_gate as pg
from test_host_calls import STREAM, p, rec  # noqa: F401  (the recorder fixture, not edited)

COST_ARGS = ["const float*", "const float*", "const float*", "int", "int", "int", "void*", "size_t", "float*", "void*"]
STEP_ARGS = ["void*", "const float*", "int", "const gclm_param_opt_config*", "void*"]
LOOP_ARGS = ["const float*", "const float*", "const float*", "int", "int", "int", "const gclm_param_opt_config*", "void*", "size_t",
             "float*", "float*", "void*"]


def test_entry_points_are_declared_exported_and_bound():
    assert_declared_exported_and_bound("gclm_param_opt_cost", COST_ARGS)
    assert_declared_exported_and_bound("gclm_param_opt_step", STEP_ARGS)
    assert_declared_exported_and_bound("gclm_param_opt", LOOP_ARGS)
    assert_declared_exported_and_bound("gclm_default_param_opt_config", ["gclm_param_opt_config*"])
    assert assert_declared_exported_and_bound("gclm_param_opt_workspace", ["int"] * 3, ret="size_t") == [C.c_int] * 3
    header = open(HEADER).read()
    changelog = header[header.index("ABI version:"):header.index("#define GCLM_VERSION")]
    for name in ("gclm_param_opt,", "gclm_param_opt_cost", "gclm_param_opt_step", "gclm_param_opt_workspace", "gclm_default_param_opt_config"):
        assert name in changelog, name
    assert geocalib_amd.PerspectiveParamOpt is perspective_opt.PerspectiveParamOpt


def test_config_struct_matches_the_header():
    header = open(HEADER).read()
    body = header[header.index("typedef struct gclm_param_opt_config {"):header.index("} gclm_param_opt_config;")]
    import re
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in re.findall(r"(?:int32_t|double)\s+([^;]+);", body) for n in re.split(r"\s*,\s*", decl.strip())]
    assert names == [n for n, _ in _lib.GclmParamOptConfig._fields_]
    for macro, value in (("STATE_WORDS", _lib.PARAM_OPT_STATE_WORDS), ("INFO_WORDS", _lib.PARAM_OPT_INFO_WORDS),
                         ("MAX_PATIENCE", _lib.PARAM_OPT_MAX_PATIENCE)):
        assert int(re.search(rf"#define GCLM_PARAM_OPT_{macro}\s+(\d+)", header).group(1)) == value


def test_default_config_is_the_reference_default_conf():
    """perspective_opt.py:24-36 of the reference, and torch's ReduceLROnPlateau defaults for what its options leave out."""
    cfg = _lib.GclmParamOptConfig.default()
    assert cfg.struct_size == C.sizeof(_lib.GclmParamOptConfig) == 8 * 4 + 8 * 8
    assert (cfg.max_steps, cfg.patience, cfg.use_scheduler, cfg.sched_patience, cfg.sched_cooldown, cfg.reserved) == (1000, 3, 1, 3, 0, 0)
    assert (cfg.lr, cfg.abs_tol, cfg.rel_tol, cfg.lamb) == (0.01, 1e-7, 1e-9, 0.5)
    assert (cfg.sched_factor, cfg.sched_threshold, cfg.sched_min_lr, cfg.sched_eps) == (0.1, 1e-4, 0.0, 1e-8)
    assert cfg.poll_every == 16
    d = perspective_opt.PerspectiveParamOpt.default_conf
    assert {k: d[k] for k in ("max_steps", "lr", "patience", "abs_tol", "rel_tol", "lamb", "verbose")} == \
        {"max_steps": 1000, "lr": 0.01, "patience": 3, "abs_tol": 1e-7, "rel_tol": 1e-9, "lamb": 0.5, "verbose": False}
    assert d["lr_scheduler"] == {"name": "ReduceLROnPlateau", "options": {"mode": "min", "patience": 3}}
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(torch.optim.Adam([torch.zeros(1, requires_grad=True)]), mode="min", patience=3)
    assert (sched.factor, sched.threshold, sched.threshold_mode, sched.cooldown, sched.eps, sched.min_lrs) == (0.1, 1e-4, "rel", 0, 1e-8, [0])
    c = perspective_opt.PerspectiveParamOpt({})._config()
    assert bytes(c) == bytes(cfg)
    assert _lib.load().gclm_default_param_opt_config(None) == -3


def test_workspace_size_is_monotone_and_zero_for_refused_sizes():
    ws = _lib.load().gclm_param_opt_workspace
    assert 0 < ws(2, 48, 64) < 1 << 16
    for grow in ((3, 48, 64), (2, 49, 64), (2, 48, 65)):
        assert ws(*grow) > ws(2, 48, 64), grow
    for B, H, W in ((1, 2, 2), (7, 479, 641), (1024, 480, 640)):
        assert ws(B, H, W) <= ws(B + 1, H, W) and ws(B, H, W) <= ws(B, H + 1, W) <= ws(B, H + 1, W + 1)
    assert ws(1024, 480, 640) < 64 << 20
    for bad in ((0, 48, 64), (65536, 48, 64), (2, 1, 64), (2, 48, 1), (2, 65536, 32768), (2, 2 ** 31 - 1, 2), (-1, 48, 64)):
        assert ws(*bad) == 0, bad


# fake, never dereferenced device addresses: every call below must be refused before the first HIP call
UP, LAT, RPV, INIT, WS, OUT, INFO, STATE, COST = 0x4000000, 0x8000000, 0x100000, 0x200000, 0x20000000, 0x30000000, 0x40000000, \
    0x50000000, 0x60000000
PX = 2 * 48 * 64 * 4           # bytes of one plane of the batch


def _cfg(**change):
    cfg = _lib.GclmParamOptConfig.default()
    for k, v in change.items():
        setattr(cfg, k, v)
    return cfg


BAD_CONFIG = [("wrong struct_size", dict(struct_size=8)), ("max_steps 0", dict(max_steps=0)), ("max_steps -1", dict(max_steps=-1)),
              ("max_steps over the cap", dict(max_steps=1000001)), ("patience 0", dict(patience=0)), ("patience 9", dict(patience=9)),
              ("negative lr", dict(lr=-0.01)), ("NaN lr", dict(lr=math.nan)), ("infinite lr", dict(lr=math.inf)),
              ("lamb -0.1", dict(lamb=-0.1)), ("lamb 1.1", dict(lamb=1.1)), ("NaN lamb", dict(lamb=math.nan)),
              ("NaN abs_tol", dict(abs_tol=math.nan)), ("NaN rel_tol", dict(rel_tol=math.nan)), ("sched_patience -1", dict(sched_patience=-1)),
              ("sched_cooldown -1", dict(sched_cooldown=-1)), ("poll_every -1", dict(poll_every=-1)), ("sched_factor 1", dict(sched_factor=1.0)),
              ("sched_factor -0.1", dict(sched_factor=-0.1)), ("NaN sched_threshold", dict(sched_threshold=math.nan)),
              ("negative sched_min_lr", dict(sched_min_lr=-1.0)), ("infinite sched_eps", dict(sched_eps=math.inf))]

LOOP_OK = dict(up=UP, lat=LAT, init=INIT, B=2, H=48, W=64, cfg={}, ws=WS, ws_bytes=1 << 24, rpv=RPV, info=INFO)
LOOP_BAD = [("NULL up", dict(up=None)), ("NULL latitude", dict(lat=None)), ("NULL config", dict(cfg=None)), ("NULL workspace", dict(ws=None)),
            ("NULL rpv", dict(rpv=None)), ("NULL info", dict(info=None)), ("B = 0", dict(B=0)), ("B > 65535", dict(B=65536)),
            ("H = 1", dict(H=1)), ("W = 1", dict(W=1)), ("H * W > 2^31 - 1", dict(H=65536, W=32768, ws_bytes=1 << 62)),
            ("up misaligned", dict(up=UP + 2)), ("latitude misaligned", dict(lat=LAT + 1)), ("init misaligned", dict(init=INIT + 2)),
            ("rpv misaligned", dict(rpv=RPV + 2)), ("info misaligned", dict(info=INFO + 1)), ("workspace misaligned", dict(ws=WS + 8)),
            ("rpv overlaps info", dict(rpv=INFO + 4)), ("rpv overlaps up", dict(rpv=UP + 2 * PX - 4)), ("info overlaps latitude", dict(info=LAT)),
            ("workspace overlaps up", dict(ws=UP - 16)), ("workspace overlaps info", dict(ws=INFO - 16)),
            ("rpv overlaps init", dict(rpv=INIT + 20)), ("workspace too small", dict(ws_bytes=1000))] + \
    [(what, dict(cfg=change)) for what, change in BAD_CONFIG]


def _loop(a):
    cfg = None if a["cfg"] is None else C.byref(_cfg(**a["cfg"]))
    return _lib.load().gclm_param_opt(a["up"], a["lat"], a["init"], a["B"], a["H"], a["W"], cfg, a["ws"], a["ws_bytes"], a["rpv"],
                                      a["info"], None)


@pytest.mark.parametrize("what,change", LOOP_BAD, ids=[b[0] for b in LOOP_BAD])
def test_loop_refuses_invalid_arguments_before_any_hip_call(what, change):
    assert _loop({**LOOP_OK, **change}) == -3, what


COST_OK = dict(up=UP, lat=LAT, rpv=RPV, B=2, H=48, W=64, ws=WS, ws_bytes=1 << 24, out=OUT)
COST_BAD = [("NULL up", dict(up=None)), ("NULL latitude", dict(lat=None)), ("NULL rpv", dict(rpv=None)), ("NULL workspace", dict(ws=None)),
            ("NULL out", dict(out=None)), ("B = 0", dict(B=0)), ("B > 65535", dict(B=65536)), ("H = 1", dict(H=1)), ("W = 1", dict(W=1)),
            ("H * W > 2^31 - 1", dict(H=65536, W=32768, ws_bytes=1 << 62)), ("up misaligned", dict(up=UP + 2)),
            ("latitude misaligned", dict(lat=LAT + 3)), ("rpv misaligned", dict(rpv=RPV + 1)), ("out misaligned", dict(out=OUT + 2)),
            ("workspace misaligned", dict(ws=WS + 4)), ("out overlaps rpv", dict(out=RPV + 8)), ("out overlaps up", dict(out=UP)),
            ("out overlaps latitude", dict(out=LAT + PX - 4)), ("workspace overlaps latitude", dict(ws=LAT + PX - 16)),
            ("workspace overlaps out", dict(ws=OUT - 16)), ("workspace too small", dict(ws_bytes=1000))]


@pytest.mark.parametrize("what,change", COST_BAD, ids=[b[0] for b in COST_BAD])
def test_cost_refuses_invalid_arguments_before_any_hip_call(what, change):
    a = {**COST_OK, **change}
    assert _lib.load().gclm_param_opt_cost(a["up"], a["lat"], a["rpv"], a["B"], a["H"], a["W"], a["ws"], a["ws_bytes"], a["out"], None) == -3


STEP_OK = dict(state=STATE, cost=COST, B=3, cfg={})
STEP_BAD = [("NULL state", dict(state=None)), ("NULL cost", dict(cost=None)), ("NULL config", dict(cfg=None)), ("B = 0", dict(B=0)),
            ("B > 65535", dict(B=65536)), ("state misaligned", dict(state=STATE + 4)), ("cost misaligned", dict(cost=COST + 2)),
            ("state overlaps cost", dict(cost=STATE + 3 * 128 - 4))] + [(what, dict(cfg=change)) for what, change in BAD_CONFIG]


@pytest.mark.parametrize("what,change", STEP_BAD, ids=[b[0] for b in STEP_BAD])
def test_step_refuses_invalid_arguments_before_any_hip_call(what, change):
    a = {**STEP_OK, **change}
    cfg = None if a["cfg"] is None else C.byref(_cfg(**a["cfg"]))
    assert _lib.load().gclm_param_opt_step(a["state"], a["cost"], a["B"], cfg, None) == -3


# ------------------------------------------------------------------ the float64 statement against the reference
N_IMAGES = 7


@pytest.mark.parametrize("i", range(N_IMAGES))
def test_closed_form_equals_the_reference_float64_autograd(i):
    """Golden (a): each of the eight numbers within 1e-10 of the reference's cost under float64 autograd, relative to the largest
    entry of its term (the cost, or the three gradient entries).  A state the maker still rejected after two retries has a pixel
    within 1e-6 of a sign switch; float64 against float64 agrees there too."""
    g = pg.golden()
    up, lat = pg.fields(i)
    for s in range(2):
        got, want = pg.cost_and_gradient(up, lat, g["states"][i, s]), g["cost64"][i, s]
        for sl in (slice(0, 1), slice(1, 2), slice(2, 5), slice(5, 8)):
            err = np.abs(got[sl] - want[sl]).max() / np.abs(want[sl]).max()
            print(i, s, sl, err)
            assert err <= 1e-10, (i, s, sl, got[sl], want[sl])


@pytest.mark.parametrize("i", range(N_IMAGES))
def test_initial_estimate_equals_the_reference(i):
    g = pg.golden()
    got = pg.initial_estimate(*pg.fields(i))
    assert np.abs(got - g["init64"][i]).max() <= 1e-12, (got, g["init64"][i])
    assert np.array_equal(g["states"][i, 0], (g["init64"][i] + 1e-3 * g["nudges"][i, 0]).astype(np.float32).astype(np.float64))


def test_golden_file_holds_the_recorded_cases():
    g = pg.golden()
    assert os.path.getsize(pg.GOLDEN) < 1_000_000
    assert g["sizes"].tolist() == [[48, 64]] * 3 + [[33, 47]] * 3 + [[120, 160]] and g["ks"].tolist() == [1, 5, 20, 100]
    assert g["poses"][:3].tolist() == [[10, 20, 60], [-35, 40, 90], [5, 3, 40]] and float(g["noise"]) == 0.02
    assert g["sequence"].shape == (3, 200, 8) and g["sequence"].dtype == np.float32
    assert (g["nudges"] <= 2).all() and g["fixed_spread"].shape == (7, 4, 3) and (g["default_spread"] > 0).all()


# ------------------------------------------------------------------ the state machine against torch, live
MACHINES = {"stopping off": dict(abs_tol=-1.0, rel_tol=0.0), "default": {}, "loose rel_tol": dict(rel_tol=2e-5),
            "abs_tol": dict(abs_tol=0.0164), "no scheduler": dict(use_scheduler=0, abs_tol=-1.0, rel_tol=0.0),
            "cooldown and floor": dict(abs_tol=-1.0, rel_tol=0.0, sched_cooldown=2, sched_min_lr=1e-5, sched_patience=1, sched_factor=0.5),
            "patience 5, lamb 0.3": dict(patience=5, lamb=0.3, rel_tol=1e-5), "eps": dict(abs_tol=-1.0, rel_tol=0.0, sched_eps=1e-4)}


@pytest.mark.parametrize("name", MACHINES)
def test_state_machine_equals_torch_adam_and_plateau(name):
    """The recorded 200-step sequences of golden: parameters to 1e-12, the lr after every step and the stopping step identical."""
    g = pg.golden()
    stops, reduced = [], 0
    for i in range(3):
        rpv = g["init64"][i]
        params, lrs, stop, sm = pg.replay(g["sequence"][i], rpv, **MACHINES[name])
        t_params, t_lrs, t_stop = pg.torch_replay(g["sequence"][i], rpv, **MACHINES[name])
        assert stop == t_stop and params.shape == t_params.shape
        assert np.array_equal(lrs, t_lrs), (name, i)
        assert np.abs(params - t_params).max() <= 1e-12, (name, i, np.abs(params - t_params).max())
        stops.append(stop)
        reduced += len(sm.reductions)
    print(name, "stops", stops, "reductions", reduced)
    if name in ("loose rel_tol", "abs_tol", "patience 5, lamb 0.3"):
        assert any(0 < s < 200 for s in stops), stops          # the stop is exercised
    if name in ("stopping off", "cooldown and floor"):
        assert stops == [0, 0, 0] and reduced >= 3             # ... and so is the scheduler
    if name == "no scheduler":
        assert reduced == 0


# ------------------------------------------------------------------ the Python module
def test_module_refuses_what_it_does_not_implement():
    P = perspective_opt.PerspectiveParamOpt
    with pytest.raises(ValueError, match="unknown"):
        P({"steps": 3})
    with pytest.raises(NotImplementedError, match="StepLR"):
        P({"lr_scheduler": {"name": "StepLR", "options": {"step_size": 3}}})
    with pytest.raises(NotImplementedError, match="max"):
        P({"lr_scheduler": {"name": "ReduceLROnPlateau", "options": {"mode": "max"}}})
    with pytest.raises(NotImplementedError, match="abs"):
        P({"lr_scheduler": {"name": "ReduceLROnPlateau", "options": {"threshold_mode": "abs"}}})
    with pytest.raises(NotImplementedError, match="verbose"):
        P({"lr_scheduler": {"name": "ReduceLROnPlateau", "options": {"verbose": True}}})
    for bad in ({"patience": 0}, {"patience": 9}, {"max_steps": 0}, {"lr": -1.0}, {"lamb": 2.0},
                {"lr_scheduler": {"name": "ReduceLROnPlateau", "options": {"factor": 1.0}}}):
        with pytest.raises(ValueError):
            P(bad)
    none = P({"lr_scheduler": {"name": None}})._config()
    assert none.use_scheduler == 0
    c = P({"lr_scheduler": {"name": "ReduceLROnPlateau", "options": {"patience": 5, "cooldown": 2, "min_lr": 1e-5}}, "poll_every": 0})._config()
    assert (c.use_scheduler, c.sched_patience, c.sched_cooldown, c.sched_min_lr, c.poll_every) == (1, 5, 2, 1e-5, 0)


def test_module_has_no_cpu_path():
    data = {"up_field": torch.zeros(1, 2, 8, 8), "latitude_field": torch.zeros(1, 1, 8, 8)}
    with pytest.raises(RuntimeError, match="HIP device"):
        perspective_opt.PerspectiveParamOpt({})(data)
    with pytest.raises(RuntimeError, match="HIP device"):
        perspective_opt.cost_function(torch.zeros(1, 3), data)


def test_module_hands_over_the_arguments_of_the_header(rec):  # noqa: F811
    rec.gclm_param_opt_workspace = lambda B, H, W: 4096
    rec.gclm_default_param_opt_config = lambda cfg: 0
    B, H, W = 3, 6, 8
    data = {"up_field": torch.randn(B, 2, H, W), "latitude_field": torch.rand(B, 1, H, W)}
    rpv0 = torch.rand(B, 3)
    out = perspective_opt.cost_function(rpv0, data)
    (name, a), = rec.calls
    ws = a[6]
    assert name == "gclm_param_opt_cost" and a[:6] == (p(data["up_field"]), p(data["latitude_field"]), p(rpv0), B, H, W)
    assert a[7] == 4096 and a[9] == STREAM and a[8] == out["up"].data_ptr() and ws % 16 == 0
    assert out["up_grad"].shape == out["latitude_grad"].shape == (B, 3) and out["latitude"].shape == (B,)
    del rec.calls[:]
    res = perspective_opt.PerspectiveParamOpt({"max_steps": 7})(data, init=rpv0)
    (name, a), = rec.calls
    assert name == "gclm_param_opt" and a[:6] == (p(data["up_field"]), p(data["latitude_field"]), p(rpv0), B, H, W)
    assert a[8] == 4096 and a[9] == p(res["rpv"]) and a[11] == STREAM and not rec.entered
    assert sorted(res) == sorted(["camera_opt", "gravity_opt", "steps", "converged", "final_cost", "final_up_cost",
                                  "final_latitude_cost", "lr", "initial", "rpv"])
    assert res["camera_opt"].shape == (B,) and res["gravity_opt"].shape == (B,) and res["steps"].dtype == torch.int32
    del rec.calls[:]
    perspective_opt.PerspectiveParamOpt({})(data)
    assert rec.calls[0][1][2] is None                          # no initial state: NULL, the kernel takes the reference's
    with pytest.raises(ValueError):
        perspective_opt.cost_function(torch.rand(B + 1, 3), data)
    with pytest.raises(ValueError):
        perspective_opt.PerspectiveParamOpt({})({"up_field": data["up_field"], "latitude_field": data["latitude_field"][:2]})


# ------------------------------------------------------------------ code objects
@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="LLVM tools missing")
def test_pass_kernels_carry_no_scratch(tmp_path):
    from test_kernel_audit import kernel_metadata
    k = {n: v for n, v in kernel_metadata(tmp_path).items() if "param_opt_pass_kernel" in n}
    for px in (1, 2, 4):
        assert any(f"param_opt_pass_kernelILi{px}E" in n for n in k), (px, sorted(k))
    print(k)
    # at most 128 VGPRs: a SIMD's 512 registers per lane then hold four waves or more, which an arithmetic-bound pass needs to
    # cover its transcendental chains; LDS is the one record per wave
    assert all(v["scratch"] == 0 and v["vgpr"] <= 128 and v["lds"] <= 512 for v in k.values()), k


# ------------------------------------------------------------------ the per-pixel statement, its bound and the edge cases
EDGE_NAMES = pg.EDGE_NAMES
CLIP_CASES = ("lower_clip", "upper_clip")
ALL_CASES = [f"ragged/{n}" for n in pg.RAGGED] + [f"edge/{n}" for n in EDGE_NAMES] + [f"batch3/{b}" for b in range(3)] + ["batch70"]


def images_of(case):
    """[(up, latitude, state)] of a case of ALL_CASES: one image, or the seventy of batch70."""
    kind, _, name = case.partition("/")
    if kind == "ragged":
        return [pg.ragged_case(name)]
    if kind == "edge":
        return [pg.edge_case(name)]
    up, lat, states = pg.batch3() if kind == "batch3" else pg.batch70()
    return [(up[b], lat[b], states[b]) for b in ([int(name)] if kind == "batch3" else range(pg.B70))]


def test_edges_file_holds_the_recorded_cases():
    g = pg.edges()
    assert os.path.getsize(pg.EDGES) < 100_000
    assert g["names"].tolist() == EDGE_NAMES
    for name in EDGE_NAMES:
        up, lat, state = pg.edge_case(name)
        H, W = {"zenith_q0": (6, 12), "zenith": (8, 12), "nadir": (8, 12), "roll80_vfov120": (8, 12), "vfov20": (8, 12), "pitch-60": (33, 47)}.get(name, (6, 8))
        assert up.shape == (2, H, W) and lat.shape == (1, H, W) and up.dtype == lat.dtype == np.float32
        assert state.dtype == np.float64 and np.array_equal(state, pg.f32(state))
        assert g[f"ref64_{name}"].shape == (8,) and g[f"finite_{name}"].all() and int(g[f"nudges_{name}"]) <= 2
    f = 4 / math.tan(math.radians(30))
    assert np.array_equal(pg.edge_case("zenith")[2], pg.f32([0, math.atan(f / 2), math.radians(60)]))
    assert np.array_equal(pg.edge_case("nadir")[2], pg.f32([0, -math.atan(f / 2), math.radians(60)]))
    assert abs(math.degrees(pg.edge_case("roll80_vfov120")[2][2]) - 120) < 1e-5 and abs(math.degrees(pg.edge_case("vfov20")[2][2]) - 20) < 1e-5
    assert abs(math.degrees(pg.edge_case("pitch-60")[2][1]) + 60 - math.degrees(pg.OFFSET[1])) < 1e-5


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_closed_form_equals_the_reference_float64_autograd_at_the_edges(name):
    """tests/golden/param_opt_edges.npz: each of the eight numbers within 1e-10 of the reference's cost under float64 autograd,
    relative to the largest entry of its term, with the reference's float64 clamp bound (the double 1 - 1e-6); a term the
    reference has at exactly 0 (the up gradients of the clip cases) is exactly 0.  A number the reference returned non-finite
    would be held to nothing here (the file has none)."""
    up, lat, state = pg.edge_case(name)
    got, want, finite = pg.cost_and_gradient(up, lat, state, clamp_hi=pg.LAT_HI64), pg.edges()[f"ref64_{name}"], pg.edges()[f"finite_{name}"]
    for sl in (slice(0, 1), slice(1, 2), slice(2, 5), slice(5, 8)):
        ok = finite[sl]
        scale = np.abs(want[sl][ok]).max() if ok.any() else 0.0
        err = np.abs(got[sl] - want[sl])[ok].max() if ok.any() else 0.0
        print(name, sl, err, scale)
        assert err <= 1e-10 * scale, (name, sl, got[sl], want[sl])
    if "zenith" in name or name == "nadir":   # the clamp bound matters: one pixel's latitude error changes by asin's slope there
        assert abs(pg.cost_and_gradient(up, lat, state)[1] - want[1]) > 1e-10 * want[1]


@pytest.mark.parametrize("case", ALL_CASES)
def test_per_pixel_statement_in_float64_is_the_yardstick(case):
    """The means of per_pixel's float64 planes equal cost_and_gradient to 1e-12 (of 1, or of the number where it is larger)."""
    for up, lat, state in images_of(case):
        got, want = pg.per_pixel(up, lat, state)[0].mean((1, 2)), pg.cost_and_gradient(up, lat, state)
        assert (np.abs(got - want) <= 1e-12 * np.maximum(1, np.abs(want))).all(), (case, got, want)
        hi = pg.per_pixel(up, lat, state, clamp_hi=pg.LAT_HI64)[0].mean((1, 2))
        assert (np.abs(hi - pg.cost_and_gradient(up, lat, state, clamp_hi=pg.LAT_HI64)) <= 1e-12 * np.maximum(1, np.abs(want))).all()


@pytest.mark.parametrize("case", ALL_CASES)
def test_every_case_is_decisive(case):
    """No pixel of any case lies where float32 and float64 may take different sides of a switch (param_opt_gate.indecisive),
    and the float32 restatement takes every branch as float64 does."""
    for up, lat, state in images_of(case):
        bad = pg.indecisive(up, lat, state)
        assert not any(v.any() for v in bad.values()), (case, {k: np.argwhere(v).tolist() for k, v in bad.items()})
        a64, a32 = pg.per_pixel(up, lat, state)[1], pg.per_pixel(up, lat, state, np.float32)[1]
        for k in ("lo", "hi", "clamped", "long"):
            assert np.array_equal(a64[k], a32[k]), (case, k)
        assert np.array_equal(np.sign(a64["e"]), np.sign(a32["e"]))


def test_edge_cases_enter_the_branches_they_are_named_for():
    for name, row, H in (("zenith", 2, 8), ("nadir", 6, 8), ("zenith_q0", 1, 6)):
        up, lat, state = pg.edge_case(name)
        for dtype in (np.float64, np.float32):
            a = pg.per_pixel(up, lat, state, dtype)[1]
            assert np.argwhere(a["clamped"]).tolist() == [[row, 6]]
            assert np.abs(a["s"][row, 6]) - pg.LAT_HI > 9e-7                       # the clamp's margin
            assert sorted(np.argwhere(~a["long"]).tolist()) == sorted([[row, 6], [H - 1 - row, 3], [4, 9]])
        assert abs(np.hypot(*up[:, 4, 9].astype(np.float64)) - pg.DELIBERATE_SHORT) < 1e-12 and not up[:, row, 6].any() and not up[:, H - 1 - row, 3].any()
    # the clamp of |q|: a float32 state leaves |q| near 1e-8 at the pole's pixel, except where the pose record is exact
    up, lat, state = pg.edge_case("zenith_q0")
    assert pg.per_pixel(up, lat, state, np.float32)[1]["n2"][1, 6] == 0 and np.argwhere(pg.per_pixel(up, lat, state, np.float32)[1]["n2"] < 1e-24).tolist() == [[1, 6]]
    up, lat, state = pg.edge_case("lower_clip")
    t, a = pg.per_pixel(up, lat, state)
    assert a["lo"].all() and (t[0] == pg.THETA_CLIP).all() and not t[2:5].any()
    assert np.array_equal(pg.gate(up, lat, state)[1][2:5], np.zeros(3))             # bound 0: the device must return exactly 0
    up, lat, state = pg.edge_case("upper_clip")
    t, a = pg.per_pixel(up, lat, state)
    assert a["hi"].sum() == 18 and a["hi"][:, :3].all() and a["lo"][:, 3:].all() and not t[2:5].any()
    assert np.array_equal(pg.gate(up, lat, state)[1][2:5], np.zeros(3))
    up, lat, state = pg.edge_case("exact_zero")
    for dtype in (np.float64, np.float32):
        assert np.argwhere(pg.per_pixel(up, lat, state, dtype)[1]["e"] == 0).tolist() == [[3, 4]]
    # the noisy cases reach the lower clip by chance only; the test of the clip-off mutant counts on these
    assert sum(int(pg.per_pixel(*c)[1]["lo"].sum()) for n in pg.RAGGED for c in [pg.ragged_case(n)]) >= 3


@pytest.mark.parametrize("case", ALL_CASES)
def test_bound_is_a_float32_bound_and_the_restatement_meets_it(case):
    """The bound of each number is MARGIN * D_k + MARGIN * 2^-23 * A_k > 0 except where the term is identically 0; it stays
    below 4e-5 of the mean magnitude of the term's planes (A_k, for a gradient the largest of its three): a float32
    evaluation's, not a looser one (the latitude cost is the loosest: an error near 0.01 rad formed from latitudes near 1 rad,
    whose float32 rounding is 6e-8, times MARGIN).  The float32 restatement itself stays within a quarter of it (it must: a mean of differences
    is no larger than the mean of their magnitudes) -- what the device's ratio is to be read against."""
    worst_rel, worst_own = 0.0, 0.0
    for up, lat, state in images_of(case):
        t64 = pg.per_pixel(up, lat, state)[0]
        want, bound, f32 = pg.gate(up, lat, state)
        A = np.abs(t64).mean((1, 2))
        scale = np.array([A[0], A[1]] + [A[2:5].max()] * 3 + [A[5:8].max()] * 3)
        assert ((bound > 0) | (A == 0)).all() and (bound[scale > 0] <= 4e-5 * scale[scale > 0]).all(), (case, bound[scale > 0] / scale[scale > 0])
        own = pg.ratios(f32, want, bound)
        worst_rel, worst_own = max(worst_rel, (bound[scale > 0] / scale[scale > 0]).max()), max(worst_own, own.max())
    print(f"{case}: bound up to {worst_rel:.2e} of the term, float32 restatement up to {worst_own:.3f} of the bound")
    assert worst_own <= 0.25


# mutant -> the cases it must be caught at.  "all" is every case but, for an error in the up gradient alone, the two clip
# cases: every pixel of theirs is inside the clip, their up gradient is 0 whatever its formula (and is gated to exactly 0).
def _under_the_clip(case):
    return all(pg.per_pixel(*c)[1]["lo"].any() or pg.per_pixel(*c)[1]["hi"].any() for c in images_of(case))


MUTANT_CASES = {"principal point": ALL_CASES, "dg/dr swapped": ALL_CASES,
                "dcp w dropped": [c for c in ALL_CASES if c.split("/")[-1] not in CLIP_CASES],
                "clip off": [f"edge/{n}" for n in CLIP_CASES] + [c for c in ALL_CASES if c.startswith(("ragged", "batch3", "edge/zenith", "edge/nadir")) and _under_the_clip(c)],
                "clamp off": ["edge/zenith", "edge/nadir", "edge/zenith_q0"], "short target by |crs|": ["edge/zenith", "edge/nadir", "edge/zenith_q0"],
                "sign(0) = 1": ["edge/exact_zero"]}
MUTANT_IDS = [(m, c) for m, cs in MUTANT_CASES.items() for c in cs]
POWER = 4.0                                   # a mutant must exceed the bound by this factor


@pytest.mark.parametrize("mutant,case", MUTANT_IDS, ids=[f"{m}-{c}" for m, c in MUTANT_IDS])
def test_bound_refuses_the_mutants_of_the_pass(mutant, case):
    """Each deliberate error in the float64 statement puts at least one of the eight numbers POWER x outside its bound, at every
    image of the case.  (clip off: at the noisy cases only where a pixel lies under the clip.)"""
    caught = []
    for up, lat, state in images_of(case):
        want, bound, _ = pg.gate(up, lat, state)
        got = pg.per_pixel(up, lat, state, mutant=mutant)[0].mean((1, 2))
        caught.append(pg.ratios(got, want, bound).max())
    print(f"{mutant} at {case}: {min(caught):.3g} .. {max(caught):.3g} of the bound")
    assert min(caught) >= POWER


@pytest.mark.parametrize("name", ["6x260", "50x516"])
def test_bound_refuses_a_dropped_tile_column(name):
    up, lat, state = pg.ragged_case(name)
    W, px = pg.RAGGED[name][1], pg.RAGGED[name][3]
    x0 = pg.last_tile_column(W, px)
    assert 0 < x0 < W
    t = pg.per_pixel(up, lat, state)[0].copy()
    t[:, :, x0:] = 0
    want, bound, _ = pg.gate(up, lat, state)
    r = pg.ratios(t.mean((1, 2)), want, bound)
    print(name, "columns from", x0, "left out:", r)
    assert r.max() >= POWER


def test_bound_refuses_image_b_at_the_state_of_image_0():
    up, lat, states = pg.batch70()
    assert len({tuple(s) for s in states}) == pg.B70
    for b in range(1, pg.B70):
        want, bound, _ = pg.gate(up[b], lat[b], states[b])
        r = pg.ratios(pg.per_pixel(up[b], lat[b], states[0])[0].mean((1, 2)), want, bound)
        assert r.max() >= POWER, (b, r)


@pytest.mark.parametrize("pose", pg.INIT_EDGES)
def test_initial_interval_holds_the_estimate_and_the_edges_take_their_branches(pose):
    """(e): the fields of INIT_EDGES reach the mirrored-roll branch (|roll| > 90 degrees, and roll = 90 where g_y = 0) and both
    ends of the vfov clamp; the interval for the device holds the float64 estimate and is a few float32 ulps wide except in
    roll near +-90 degrees."""
    up, lat = pg.init_fields(pose)
    est = pg.initial_estimate(up, lat)
    lo, hi = pg.initial_interval(up, lat)
    assert (lo <= est).all() and (est <= hi).all()
    width = (hi - lo) / np.spacing(np.abs(est).astype(np.float32)).astype(np.float64)
    print(pose, np.degrees(est), width)
    assert (width[1:] <= 9).all()
    if abs(pose[0]) > 90:
        assert abs(abs(math.degrees(est[0])) - abs(pose[0])) < 0.1 and np.sign(est[0]) == np.sign(pose[0]) and width[0] <= (13 if abs(pose[0]) > 100 else 400)
    if pose[0] == 90:
        assert up[1, 24, 32] == 0 and 89 < math.degrees(lo[0]) < 90 < math.degrees(hi[0]) < 91     # the two branches meet here
    if pose[2] == 10:
        assert est[2] == pytest.approx(float(np.float32(math.radians(20))), abs=1e-12)
    if pose[2] == 150:
        assert est[2] == pytest.approx(float(np.float32(math.radians(120))), abs=1e-12)


# ------------------------------------------------------------------ the caller's workspace
def _device_call(name, dev):
    up, lat, state = pg.ragged_case(name)
    data = {"up_field": torch.from_numpy(up.copy())[None].to(dev), "latitude_field": torch.from_numpy(lat.copy())[None].to(dev)}
    init = torch.from_numpy(np.asarray(state, np.float32))[None].to(dev)
    opt = perspective_opt.PerspectiveParamOpt({"max_steps": 12})

    def run():
        out = opt(data, init=init)
        return [out[k] for k in ("rpv", "steps", "converged", "final_cost", "final_up_cost", "final_latitude_cost", "lr")]
    return run


@pytest.mark.gpu
def test_results_do_not_depend_on_what_the_workspace_held(monkeypatch):
    """gclm_param_opt on the ragged 6 x 260 case (two tile columns, two tile rows) with the wrapper's torch.empty workspace
    holding 0x00 bytes, 0xFF bytes, and the state and records of a call at 50 x 516: the same bits after twelve steps."""
    from workspace_fill import same_bits_whatever_the_memory_held
    dev = torch.device("cuda:0")
    same_bits_whatever_the_memory_held(monkeypatch, dev, _device_call("6x260", dev), _device_call("50x516", dev))
