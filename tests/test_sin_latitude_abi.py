"""CPU: the sin(latitude) handoff from the head epilogue to the solve (gclm_pack_fields_ex -> gclm_solve_ex /
gclm_calibrate_ex / gclm_shared_begin_ex) is declared, exported and bound, and every Python route hands each C call the
rows of data["sin_latitude"] that match its rows of data["latitude_field"].  The C entry points and the device check are
replaced by recorders: no kernel runs here (tests/test_sin_latitude_handoff.py runs them on the GPU)."""
import ctypes as C
import inspect
import re
import types

import pytest
import torch

from geocalib_amd import _call, _lib, lm_optimizer, parallel
from geocalib_amd.lm_optimizer import LMOptimizer
from abi_harness import declared

PARENTS = {"gclm_pack_fields_ex": "gclm_pack_fields", "gclm_solve_ex": "gclm_solve", "gclm_calibrate_ex": "gclm_calibrate",
           "gclm_shared_begin_ex": "gclm_shared_begin"}


def test_ex_entry_points_are_declared_exported_and_bound_with_one_more_pointer():
    lib = C.CDLL(_lib.LIB_PATH)
    for ex, parent in PARENTS.items():
        assert hasattr(lib, ex), f"{ex} not exported"
        assert ex in _lib.EXPORTED_SYMBOLS
        pe, pp = declared(ex, names=True), declared(parent, names=True)
        # the plane goes just before the stream: the parent's parameters, then the plane, then `void* stream`
        assert len(pe) == len(pp) + 1, (ex, pe)
        assert pe[:-2] == pp[:-1] and pe[-1] == pp[-1] == "void* stream", (ex, pe)
        assert re.fullmatch(r"(const )?float\* d_sin_lat", pe[-2]), pe[-2]
        res_e, args_e = _lib._SIGNATURES[ex]
        res_p, args_p = _lib._SIGNATURES[parent]
        assert res_e is res_p and list(args_e) == list(args_p[:-1]) + [_lib._P, args_p[-1]], ex
    assert _lib.load().gclm_version() == 610 == _lib.ABI_VERSION


def test_pack_fields_has_the_sin_latitude_switch():
    from geocalib_amd.fields import pack_fields
    p = inspect.signature(pack_fields).parameters["sin_latitude"]
    assert p.default is False and p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD


# ------------------------------------------------------------------ recorders in place of the device and the library

class _Rec:
    """Stands in for the loaded library: records the pointer arguments of every gclm_* call."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("gclm_"):
            raise AttributeError(name)

        def fn(*args):
            if name == "gclm_plan_cut":            # every part is cut like the whole batch
                args[5]._obj.value = 20
                return 0
            self.calls.append((name, args))
            return 0
        return fn


class _NoDevice:
    def __init__(self, *a):
        pass

    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


class _Stream:
    cuda_stream = 0

    def __init__(self, *a, **k):
        pass

    def record_event(self):
        return None

    def wait_event(self, e):
        return None


@pytest.fixture
def rec(monkeypatch):
    r = _Rec()
    monkeypatch.setattr(_lib, "load", lambda: r)
    # the one device check lets CPU tensors through (the conversion around it stays the real one)
    monkeypatch.setattr(_call, "require_device", lambda t, name: None)
    monkeypatch.setattr(_call, "raw_stream", lambda device: 0)
    monkeypatch.setattr(LMOptimizer, "_handle", lambda self, device, stream=None: types.SimpleNamespace(ptr=C.c_void_p(1)))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: _Stream())
    monkeypatch.setattr(torch.cuda, "Stream", _Stream)
    monkeypatch.setattr(torch.cuda, "device", _NoDevice)
    return r


def _fields(B, H, W, confidences=True):
    g = torch.Generator().manual_seed(B)
    d = {"up_field": torch.randn(B, 2, H, W, generator=g), "latitude_field": torch.rand(B, 1, H, W, generator=g) - 0.5}
    if confidences:
        d["up_confidence"] = torch.rand(B, H, W, generator=g)
        d["latitude_confidence"] = torch.rand(B, H, W, generator=g)
    d["sin_latitude"] = torch.sin(d["latitude_field"])
    return d


def _offsets(calls, name, lat_arg, slat_arg, data):
    """(lat, sin_lat) byte offsets into the caller's tensors, per call of `name`."""
    lat0, slat0 = data["latitude_field"].data_ptr(), data["sin_latitude"].data_ptr()
    return [(a[lat_arg] - lat0, a[slat_arg] - slat0) for n, a in calls if n == name]


def test_chunked_calibration_hands_every_slice_its_rows_of_sin_latitude(rec):
    B = LMOptimizer._MAX_CALL + 3
    data = _fields(B, 1, 4, confidences=False)
    opt = LMOptimizer({"camera_model": "simple_radial", "num_steps": 2})
    opt.setup_optimization_and_priors(data)
    opt.calibrate_fields(data)
    offs = _offsets(rec.calls, "gclm_calibrate_ex", 2, 16, data)
    row = 4 * 4
    assert offs == [(0, 0), (LMOptimizer._MAX_CALL * row, LMOptimizer._MAX_CALL * row)], offs
    assert [a[5] for n, a in rec.calls if n == "gclm_calibrate_ex"] == [LMOptimizer._MAX_CALL, 3]
    assert not any(n == "gclm_calibrate" for n, _ in rec.calls)


def test_overlapped_calibration_hands_every_part_its_rows_of_sin_latitude(rec):
    B, H, W = 768, 2, 4
    data = _fields(B, H, W)
    opt = LMOptimizer({"camera_model": "radial", "num_steps": 2, "early_stop": False})
    opt.overlap_streams = 3
    opt.setup_optimization_and_priors(data)
    opt.calibrate_fields(data)
    offs = _offsets(rec.calls, "gclm_calibrate_ex", 2, 16, data)
    assert len(offs) == 3 and all(lat == slat for lat, slat in offs), offs
    assert [o[0] for o in offs] == [lo * H * W * 4 for lo in (0, 256, 512)]
    assert [a[5] for n, a in rec.calls if n == "gclm_calibrate_ex"] == [256, 256, 256]
    assert any(n == "gclm_merge_stop_at" for n, _ in rec.calls)


def test_single_call_and_optimize_pass_the_plane_and_null_without_it(rec):
    data = _fields(4, 2, 4)
    opt = LMOptimizer({"camera_model": "pinhole", "num_steps": 2})
    opt.setup_optimization_and_priors(data)
    opt.calibrate_fields(data)
    without = {k: v for k, v in data.items() if k != "sin_latitude"}
    opt.calibrate_fields(without)
    cam0, grav0 = lm_optimizer.get_trivial_estimation(data, opt.camera_model)
    opt.optimize(data, cam0, grav0)
    opt.optimize(without, cam0, grav0)
    cal = [a for n, a in rec.calls if n == "gclm_calibrate_ex"]
    sol = [a for n, a in rec.calls if n == "gclm_solve_ex"]
    assert [a[16] for a in cal] == [data["sin_latitude"].data_ptr(), None]
    assert [a[11] for a in sol] == [data["sin_latitude"].data_ptr(), None]
    assert all(a[2] == data["latitude_field"].data_ptr() for a in cal + sol)      # the radians stay required


def test_sin_latitude_is_checked_like_the_fields(monkeypatch):
    lat = torch.zeros(2, 1, 4, 4)
    with pytest.raises(RuntimeError, match="`sin_latitude` must live on a HIP device"):
        LMOptimizer._sin_lat({"sin_latitude": torch.zeros(2, 1, 4, 4)}, lat)
    monkeypatch.setattr(_call, "require_device", lambda t, name: None)
    with pytest.raises(ValueError, match="shape of `latitude_field`"):
        LMOptimizer._sin_lat({"sin_latitude": torch.zeros(2, 1, 4, 5)}, lat)
    assert LMOptimizer._sin_lat({}, lat) is None


def test_calibrate_sharded_passes_the_key_to_the_optimizer(monkeypatch):
    seen = {}

    def fake(self, data):
        seen["data"] = data
        return "cam", "grav", {}
    monkeypatch.setattr(LMOptimizer, "calibrate_fields", fake)
    data = _fields(4, 2, 4)
    out = parallel.calibrate_sharded(LMOptimizer({"camera_model": "simple_radial", "num_steps": 2, "early_stop": False}),
                                     data, 4)
    assert out["camera"] == "cam"
    assert seen["data"]["sin_latitude"] is data["sin_latitude"]


def test_shared_intrinsics_split_hands_the_plane_to_the_session(rec):
    data = _fields(4, 2, 4)
    opt = LMOptimizer({"camera_model": "simple_radial", "num_steps": 2, "early_stop": False, "shared_intrinsics": True})
    split = parallel.SharedIntrinsicsSplit(opt, num_groups=1)
    split(data, torch.zeros(4, dtype=torch.int32))
    begins = [a for n, a in rec.calls if n == "gclm_shared_begin_ex"]
    assert len(begins) == 1 and begins[0][12] == data["sin_latitude"].data_ptr()
    assert begins[0][2] == data["latitude_field"].data_ptr()
    split({k: v for k, v in data.items() if k != "sin_latitude"}, torch.zeros(4, dtype=torch.int32))
    assert [a[12] for n, a in rec.calls if n == "gclm_shared_begin_ex"][1] is None
