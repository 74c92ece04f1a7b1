"""CPU: gclm_field_errors without a device -- the entry points are declared, exported and bound, every invalid argument is
refused before any HIP call, the workspace size is monotone, the float64 yardstick of tests/field_error_gate.py equals
metrics.perspective_field_metrics on CPU float64 inputs, the seven scalar metrics match closed forms and the reference's
recorded angles, the gate passes an honest float32 restatement of the kernel and fails its mutants, the Python wrapper hands
the C entry the arguments of include/gclm.h, and the kernels carry no scratch."""
import ctypes as C
import math
import os

import pytest
import torch

from geocalib_amd import Gravity, _call, _lib, camera_models, fields, metrics
from abi_harness import HEADER, LLVM, assert_declared_exported_and_bound
import field_error_gate as fg
import perspective_gate as pg
from test_host_calls import MAX, STREAM, p, rec  # noqa: F401  (the recorder fixture, not edited)

ARGS = ["int", "const float*", "const float*", "int", "int", "int", "const float*", "const float*", "const float*", "const float*",
        "int", "const float*", "void*", "size_t", "float*", "float*", "float*", "void*"]


def test_entry_points_are_declared_exported_and_bound():
    args = assert_declared_exported_and_bound("gclm_field_errors", ARGS)
    for a, t in zip(args, ARGS):
        assert t in ("int", "size_t") or a in (C.c_void_p, C.POINTER(C.c_float)), (a, t)
    assert assert_declared_exported_and_bound("gclm_field_errors_workspace", ["int"] * 4, ret="size_t") == [C.c_int] * 4
    header = open(HEADER).read()
    changelog = header[header.index("ABI version:"):header.index("#define GCLM_VERSION")]
    assert "gclm_field_errors_workspace" in changelog and "gclm_field_errors " in changelog


# fake, never dereferenced device addresses: every call below must be refused before the first HIP call
CAM, GRAV, UP, LAT, UPC, LATC = 0x100000, 0x200000, 0x4000000, 0x8000000, 0xC000000, 0x10000000
WS, STATS, UERR, LERR = 0x20000000, 0x30000000, 0x40000000, 0x50000000
PX_BYTES = 2 * 48 * 64 * 4
OK = dict(model=1, cam=CAM, grav=GRAV, B=2, H=48, W=64, up=UP, lat=LAT, upc=UPC, latc=LATC, n=4, thr=(1.0, 3.0, 5.0, 10.0),
          ws=WS, ws_bytes=1 << 24, stats=STATS, uerr=UERR, lerr=LERR)
BAD = [("NULL camera", dict(cam=None)), ("NULL gravity", dict(grav=None)), ("NULL stats", dict(stats=None)),
       ("NULL workspace", dict(ws=None)), ("both fields NULL", dict(up=None, lat=None, upc=None, latc=None, uerr=None, lerr=None)),
       ("up confidence without up", dict(up=None, uerr=None)), ("up map without up", dict(up=None, upc=None)),
       ("latitude confidence without latitude", dict(lat=None, lerr=None)), ("latitude map without latitude", dict(lat=None, latc=None)),
       ("B = 0", dict(B=0)), ("B > 65535", dict(B=65536)), ("H = 0", dict(H=0)), ("W = 0", dict(W=0)),
       ("H * W > 2^31 - 1", dict(H=65536, W=32768, ws_bytes=1 << 62)), ("tile grid over 2^32 threads", dict(H=2 ** 31 - 1, W=1, ws_bytes=1 << 62)),
       ("model -1", dict(model=-1)), ("model 4", dict(model=4)), ("n_thresholds -1", dict(n=-1)), ("n_thresholds 9", dict(n=9, thr=(1.0,) * 9)),
       ("NULL thresholds", dict(thr=None)), ("NaN threshold", dict(thr=(1.0, math.nan, 5.0, 10.0))),
       ("infinite threshold", dict(thr=(1.0, 3.0, 5.0, math.inf))), ("workspace too small", dict(ws_bytes=1000)),
       ("camera misaligned", dict(cam=CAM + 2)), ("up misaligned", dict(up=UP + 1)), ("latitude confidence misaligned", dict(latc=LATC + 2)),
       ("stats misaligned", dict(stats=STATS + 2)), ("workspace misaligned", dict(ws=WS + 1)), ("latitude map misaligned", dict(lerr=LERR + 3)),
       ("stats overlap the camera", dict(stats=CAM + 32)), ("stats overlap the gravity", dict(stats=GRAV - 8)),
       ("up map overlaps up", dict(uerr=UP + 2 * PX_BYTES - 4)), ("latitude map overlaps latitude", dict(lerr=LAT)),
       ("up map overlaps the latitude confidence", dict(uerr=LATC - 4)), ("workspace overlaps the up confidence", dict(ws=UPC + PX_BYTES - 4)),
       ("workspace overlaps stats", dict(ws=STATS - 4)), ("the maps overlap", dict(lerr=UERR + PX_BYTES - 4)),
       ("up map overlaps stats", dict(uerr=STATS - PX_BYTES + 4))]


def _call_abi(a):
    thr = None if a["thr"] is None else (C.c_float * len(a["thr"]))(*a["thr"])
    return _lib.load().gclm_field_errors(a["model"], a["cam"], a["grav"], a["B"], a["H"], a["W"], a["up"], a["lat"], a["upc"],
                                         a["latc"], a["n"], thr, a["ws"], a["ws_bytes"], a["stats"], a["uerr"], a["lerr"], None)


@pytest.mark.parametrize("what,change", BAD, ids=[b[0] for b in BAD])
def test_invalid_arguments_are_refused_before_any_hip_call(what, change):
    assert _call_abi({**OK, **change}) == -3, what


def test_workspace_size_is_monotone_and_zero_for_invalid_sizes():
    ws = _lib.load().gclm_field_errors_workspace
    assert 0 < ws(2, 48, 64, 4) <= OK["ws_bytes"]
    for grow in ((3, 48, 64, 4), (2, 49, 64, 4), (2, 48, 65, 4), (2, 48, 64, 5)):
        assert ws(*grow) > ws(2, 48, 64, 4), grow
    for B, H, W in ((1, 1, 1), (7, 479, 641), (1024, 480, 640)):
        assert ws(B, H, W, 0) <= ws(B + 1, H, W, 0) and ws(B, H, W, 0) <= ws(B, H + 1, W, 0) <= ws(B, H + 1, W + 1, 0)
    assert ws(1024, 480, 640, 4) < 256 << 20
    for bad in ((0, 48, 64, 4), (65536, 48, 64, 4), (2, 0, 64, 4), (2, 48, 0, 4), (2, 65536, 32768, 4), (2, 48, 64, -1),
                (2, 48, 64, 9), (2, 2 ** 31 - 1, 1, 0)):
        assert ws(*bad) == 0, bad


# ------------------------------------------------------------------ the yardstick
SMALL = [c for c in fg.CASES if not c[5]]
_cache = {}


def _case(case):
    """(cams, gravs, data, yardstick) of a case with every plane, computed once and left unchanged."""
    if case not in _cache:
        cams, gravs, data = fg.make_case(case)
        _cache[case] = (cams, gravs, data, fg.yardstick(case, cams, gravs, data))
    return _cache[case]


@pytest.mark.parametrize("case", [c for c in SMALL if c[1:4] == fg.SHAPES[0]], ids=fg.case_id)
def test_yardstick_equals_the_torch_path_in_float64(case):
    """The latitude errors agree to 1e-9 degrees.  The up errors to 5e-6: float64 acos of a cosine next to 1 (the small-angle
    image) has a quantum of acos(1 - 2^-53) = 8.5e-7 degrees, and simple_divisional's s' of the torch path cancels in float64
    too where |k1 r2| is tiny (tests/test_perspective_abi.py)."""
    cams, gravs, data, y = _case(case)
    cam, grav = camera_models[case[0]](cams.double()), Gravity(gravs.double())
    grav._data = gravs.double()                   # as stored: the yardstick does not renormalise either
    out = metrics.perspective_field_metrics({k: v.double() for k, v in data.items()}, cam, grav, return_errors=True)
    keys = ["up_angle_error", "up_angle_error_weighted"] + [f"up_angle_recall@{t}" for t in fg.THRESHOLDS]
    keys += [k.replace("up_", "latitude_") for k in keys]
    assert sorted(out) == sorted(keys + ["up_error", "latitude_error"])
    # (the target of the torch path is clamped at the float64 bound, the yardstick's at the float32 one: no pixel is near it)
    tol = 5e-6
    near = (y["e_up"] - torch.tensor(fg.THRESHOLDS)[:, None, None, None]).abs().min() < tol
    assert (out["up_error"] - y["e_up"]).abs().max() <= tol and (out["latitude_error"] - y["e_lat"]).abs().max() <= 1e-9
    for i, k in enumerate(keys):
        if "recall" in k and near:
            continue
        assert torch.allclose(out[k].double(), y["stats"][:, i], rtol=1e-6, atol=tol), k
    only_lat = metrics.perspective_field_metrics({"latitude_field": data["latitude_field"].double()}, cam, grav, (2, 4))
    assert sorted(only_lat) == ["latitude_angle_error", "latitude_angle_recall@2", "latitude_angle_recall@4"]
    with pytest.raises(ValueError):
        metrics.perspective_field_metrics({}, cam, grav)


@pytest.mark.parametrize("model", pg.MODELS)
def test_every_default_threshold_cuts_through_the_errors(model):
    """The recall test is not vacuous: at least one case per model has an image whose yardstick recalls of both fields lie
    strictly between 0.05 and 0.95 at every default threshold."""
    found = False
    for case in (c for c in SMALL if c[0] == model):
        s = _case(case)[3]["stats"]
        rec_cols = s[:, [2, 3, 4, 5, 8, 9, 10, 11]]
        found |= bool(((rec_cols > 0.05) & (rec_cols < 0.95)).all(1).any())
    assert found


# ------------------------------------------------------------------ the scalar metrics
def test_scalar_metrics_match_closed_forms():
    d = math.radians
    g0, g1 = Gravity.from_rp(torch.tensor([d(10.0), d(-5.0)]), torch.tensor([d(20.0), d(3.0)])), \
        Gravity.from_rp(torch.tensor([d(7.0), d(-9.0)]), torch.tensor([d(25.5), d(-1.0)]))
    assert torch.allclose(metrics.roll_error(g0, g1), torch.tensor([3.0, 4.0]), atol=2e-3)
    assert torch.allclose(metrics.pitch_error(g0, g1), torch.tensor([5.5, 4.0]), atol=2e-3)
    zero = Gravity.from_rp(torch.zeros(2), torch.tensor([d(0.0), d(30.0)]))
    tilt = Gravity.from_rp(torch.zeros(2), torch.tensor([d(40.0), d(-15.0)]))
    assert torch.allclose(metrics.gravity_error(zero, tilt), torch.tensor([40.0, 45.0]), atol=1e-3)
    assert metrics.gravity_error(zero, zero).abs().max() < 0.05          # (float32 acos: the quantum is 0.02 .. 0.03 degrees)
    cams = {}
    for model, k1 in (("pinhole", None), ("simple_radial", [0.1, -0.2])):
        for name, vfov in (("a", [60.0, 90.0]), ("b", [50.0, 97.5])):
            dd = {"height": torch.full((2,), 480.0), "width": torch.full((2,), 640.0), "vfov": torch.tensor([d(v) for v in vfov])}
            if k1:
                dd["k1"] = torch.tensor(k1) * (1 if name == "a" else 3)
            cams[model, name] = camera_models[model].from_dict(dd)
    assert torch.allclose(metrics.vfov_error(cams["pinhole", "a"], cams["pinhole", "b"]), torch.tensor([10.0, 7.5]), atol=1e-3)
    assert metrics.dist_error(cams["pinhole", "a"], cams["pinhole", "b"]).tolist() == [0.0, 0.0]
    assert torch.allclose(metrics.dist_error(cams["simple_radial", "a"], cams["simple_radial", "b"]), torch.tensor([0.2, 0.4]))
    up = torch.tensor([[1.0, 0.0], [0.0, 2.0], [-1.0, 0.0], [3.0, 3.0]]).T.reshape(1, 2, 2, 2)
    e = metrics.up_error(up, torch.tensor([1.0, 0.0]).reshape(1, 2, 1, 1).expand(1, 2, 2, 2).contiguous())
    assert e.shape == (1, 2, 2) and torch.allclose(e.reshape(-1), torch.tensor([0.0, 90.0, 180.0, 45.0]), atol=0.03)
    lat = torch.tensor([0.1, -0.2, 0.0, 1.0]).reshape(1, 1, 2, 2)
    e = metrics.latitude_error(lat, torch.zeros(1, 1, 2, 2))
    assert e.shape == (1, 2, 2) and torch.allclose(e.reshape(-1), torch.tensor([0.1, 0.2, 0.0, 1.0]) * 180 / math.pi)


@pytest.mark.parametrize("model", pg.MODELS)
def test_scalar_metrics_match_the_reference_angles(model):
    """tests/golden/golden_host_api.npz: the reference's own roll and vfov of its cameras and gravities, image i against
    image i + 1."""
    from test_host_api import host_api_golden
    g = host_api_golden()
    cams, gravs = g[f"api/{model}/camera"], g[f"api/{model}/gravity"]
    cam, grav = camera_models[model](cams), Gravity(gravs)
    other_c, other_g = camera_models[model](cams.roll(1, 0)), Gravity(gravs.roll(1, 0))
    roll, vfov = g[f"api/{model}/out64/roll"].double().reshape(-1), g[f"api/{model}/out64/vfov"].double().reshape(-1)
    assert torch.allclose(metrics.roll_error(grav, other_g).double(), (roll - roll.roll(1)).abs() * fg.DEG, atol=1e-3)
    assert torch.allclose(metrics.vfov_error(cam, other_c).double(), (vfov - vfov.roll(1)).abs() * fg.DEG, atol=1e-3)
    assert metrics.gravity_error(grav, grav).abs().max() < 0.05 and metrics.pitch_error(grav, grav).abs().max() == 0
    want = (cams[:, 6] - cams.roll(1, 0)[:, 6]).abs() if model != "pinhole" else torch.zeros(cams.shape[0])
    assert torch.equal(metrics.dist_error(cam, other_c), want)


# ------------------------------------------------------------------ the GPU test's gate, checked here
@pytest.mark.parametrize("case", fg.CASES + fg.EXTREMES, ids=fg.case_id)
def test_gate_passes_an_honest_float32_restatement(case):
    cams, gravs, data = fg.make_case(case)
    for which in ("all", "noconf", "up", "lat"):
        d = fg.subset(data, which)
        v = fg.verdict(fg.yardstick(case, cams, gravs, d), fg.restate(case, cams, gravs, d))
        print(f"{fg.case_id(case)} {which}: honest float32 {v}")
        assert v["up_px"] <= 0.25 and v["lat_px"] <= 0.25 and v["means"] <= 0.5 and v["recalls"] == 0 and v["nan"] == 0, (which, v)


_C = {(c[0], c[2], c[3]): c for c in SMALL}
# (mutant, case, what it must push past its gate)
MUTANTS = [("acos32", _C["pinhole", 37, 53], "up_px"), ("acos32", _C["radial", 30, 200], "means"),
           ("nomask", _C["simple_radial", 37, 53], "up_px"), ("nomask", _C["pinhole", 9, 132], "means"),
           ("unmasked_mean", _C["pinhole", 37, 53], "means"), ("unmasked_mean", _C["simple_divisional", 30, 200], "means"),
           ("radians", _C["radial", 37, 53], "lat_px"), ("radians", _C["simple_divisional", 9, 132], "recalls"),
           ("swapconf", _C["pinhole", 30, 200], "means"), ("swapconf", _C["simple_radial", 9, 132], "means"),
           ("renorm", _C["pinhole", 37, 53], "lat_px"), ("renorm", _C["simple_radial", 30, 200], "lat_px"),
           ("halfpx", _C["pinhole", 37, 53], "up_px"), ("halfpx", _C["simple_divisional", 37, 53], "lat_px")]


@pytest.mark.parametrize("mutant,case,what", MUTANTS, ids=[f"{m}-{fg.case_id(c)}-{w}" for m, c, w in MUTANTS])
def test_gate_fails_each_mutant(mutant, case, what):
    cams, gravs, data, y = _case(case)
    if mutant == "renorm":           # a stored gravity that is not a unit vector
        gravs = gravs * 1.001
        y = fg.yardstick(case, cams, gravs, data)
    v = fg.verdict(y, fg.restate(case, cams, gravs, data, mutant=mutant))
    print(f"{mutant} on {fg.case_id(case)}: {v}")
    assert not fg.passes(v) and (v[what] > 1 if what != "recalls" else v[what] > 0), (mutant, v)
    if mutant == "acos32":           # ... and it is the small-angle image that catches it
        last = {k: (t[-1:] if t is not None else None) for k, t in fg.restate(case, cams, gravs, data, mutant=mutant).items()}
        ylast = {k: (t[-1:] if torch.is_tensor(t) else t) for k, t in y.items()}
        assert fg.verdict(ylast, last)["up_px"] > 1


# ------------------------------------------------------------------ the call path (the recorder of test_host_calls.py)
def _inputs(B, H=2, W=2):
    g = torch.Generator().manual_seed(0)
    cam = torch.tensor([[float(W), float(H), 1.5, 1.5, W / 2, H / 2, 0.05, 0.0]]).repeat(B, 1)
    grav = torch.tensor([[0.0, 1.0, 0.0]]).repeat(B, 1)
    return cam, grav, torch.randn(B, 2, H, W, generator=g), torch.rand(B, 1, H, W, generator=g), torch.rand(B, H, W, generator=g), \
        torch.rand(B, H, W, generator=g)


def test_field_errors_hands_over_the_arguments_of_the_header(rec):  # noqa: F811
    cam, grav, up, lat, upc, latc = _inputs(2)
    stats, ue, le = fields.field_errors("radial", cam, grav, up, lat, upc, latc, (1, 3, 5, 10), return_errors=True)
    assert stats.shape == (2, 12) and ue.shape == le.shape == (2, 2, 2)
    (n0, a0), (n1, a1) = rec.calls
    assert (n0, a0) == ("gclm_field_errors_workspace", (2, 2, 2, 4)) and n1 == "gclm_field_errors"
    ws = a1[12]
    assert a1 == (2, p(cam), p(grav), 2, 2, 2, p(up), p(lat), p(upc), p(latc), 4, [1.0, 3.0, 5.0, 10.0], ws, 0, p(stats), p(ue), p(le),
                  STREAM)
    assert isinstance(ws, int) and ws not in (p(stats), p(ue), p(le)) and not rec.entered


def test_field_errors_passes_null_for_absent_planes(rec):  # noqa: F811
    cam, grav, up, lat, upc, latc = _inputs(2)
    stats, ue, le = fields.field_errors("pinhole", cam, grav, None, lat, None, None, ())
    assert ue is None and le is None and stats.shape == (2, 4)
    a = rec.calls[1][1]
    assert a[:12] == (0, p(cam), p(grav), 2, 2, 2, None, p(lat), None, None, 0, []) and a[14:] == (p(stats), None, None, STREAM)
    del rec.calls[:]
    stats, ue, le = fields.field_errors("pinhole", cam, grav, up, None, upc, None, (2.5,), return_errors=True)
    a = rec.calls[1][1]
    assert a[6:12] == (p(up), None, p(upc), None, 1, [2.5]) and a[14:] == (p(stats), p(ue), None, STREAM) and le is None
    with pytest.raises(ValueError):
        fields.field_errors("pinhole", cam, grav)
    with pytest.raises(ValueError):
        fields.field_errors("pinhole", cam, grav, None, lat, upc)


def test_field_errors_slices_and_advances_every_pointer(rec):  # noqa: F811
    B = MAX + 3
    cam, grav, up, lat, upc, latc = _inputs(B, 1, 1)
    stats, ue, le = fields.field_errors("pinhole", cam, grav, up, lat, upc, latc, (1, 3), return_errors=True)
    (_, w), (_, first), (_, second) = rec.calls
    assert w == (MAX, 1, 1, 2)                   # one workspace, sized for the largest call
    ws = first[12]
    assert first == (0, p(cam), p(grav), MAX, 1, 1, p(up), p(lat), p(upc), p(latc), 2, [1.0, 3.0], ws, 0, p(stats), p(ue), p(le), STREAM)
    assert second == (0, p(cam) + MAX * 32, p(grav) + MAX * 12, 3, 1, 1, p(up) + MAX * 8, p(lat) + MAX * 4, p(upc) + MAX * 4,
                      p(latc) + MAX * 4, 2, [1.0, 3.0], ws, 0, p(stats) + MAX * 8 * 4, p(ue) + MAX * 4, p(le) + MAX * 4, STREAM)


def test_metrics_take_the_torch_path_off_the_device():
    """CPU tensors never reach the library (no device check fires): the torch composition answers."""
    case = SMALL[0]
    cams, gravs, data, y = _case(case)
    out = metrics.perspective_field_metrics(data, camera_models[case[0]](cams), Gravity(gravs), return_errors=True)
    assert out["up_error"].dtype == torch.float32 and out["up_angle_error"].shape == (case[1],)
    assert torch.allclose(out["latitude_angle_error"].double(), y["stats"][:, 6], rtol=1e-4, atol=1e-5)
    assert torch.allclose(out["up_angle_error"].double(), y["stats"][:, 0], rtol=1e-3, atol=0.03)     # float32 acos: quantised
    assert _call.MAX_CALL == MAX


# ------------------------------------------------------------------ code objects
@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="LLVM tools missing")
def test_field_error_kernels_carry_no_scratch(tmp_path):
    from test_kernel_audit import kernel_metadata
    k = {n: v for n, v in kernel_metadata(tmp_path).items() if "field_error" in n}
    for m in range(4):
        for px in (1, 2, 4):
            assert any(f"field_error_kernelILi{m}ELi{px}E" in n for n in k), (m, px, sorted(k))
    assert any("field_error_finish_kernel" in n for n in k)
    print({n: v for n, v in k.items()})
    assert all(v["scratch"] == 0 for v in k.values()), k
    assert all(v["vgpr"] <= 64 and v["lds"] <= 2048 for v in k.values()), k


# ------------------------------------------------------------------ the caller's workspace
def _device_call(case, dev):
    cams, gravs, data = fg.make_case(case)
    args = [t.to(dev) for t in (cams, gravs, *(data[k] for k in ("up_field", "latitude_field", "up_confidence", "latitude_confidence")))]
    return lambda: fields.field_errors(case[0], *args, thresholds=fg.THRESHOLDS, return_errors=True)


@pytest.mark.gpu
def test_results_do_not_depend_on_what_the_workspace_held(monkeypatch):
    """gclm_field_errors at 30 x 200 (tile columns and rows both ragged) with the wrapper's torch.empty workspace holding 0x00
    bytes, 0xFF bytes, and the records of a call at 3 x 37 x 53: the same bits."""
    from workspace_fill import same_bits_whatever_the_memory_held
    dev = torch.device("cuda:0")
    same_bits_whatever_the_memory_held(monkeypatch, dev, _device_call(("simple_radial", 2, 30, 200, "random", False), dev),
                                       _device_call(("simple_radial", 3, 37, 53, "random", False), dev))
