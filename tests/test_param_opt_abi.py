"""CPU: gclm_param_opt without a device -- the entry points are declared, exported and bound, the default config is the
reference's default_conf, the workspace size is monotone, every invalid argument is refused before any HIP call, the float64
statement of tests/param_opt_gate.py equals the reference's float64 autograd (tests/golden/param_opt_reference.npz) and its
state machine equals torch.optim.Adam + ReduceLROnPlateau run live, the Python module refuses what it does not implement and
hands the C entries the arguments of include/gclm.h."""
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
