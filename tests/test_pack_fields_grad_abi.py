"""CPU: gclm_pack_fields_typed and gclm_pack_fields_backward without a device -- declared, exported, bound and documented;
every invalid argument refused before any HIP call, and the legal neighbours reaching the launch; what the compiler made of
the two kernels (no scratch, no LDS, in any instantiation); and the calls fields.pack_fields makes of them, with the library
replaced by the recorder of tests/test_host_calls.py."""
import ctypes as C
import os

import pytest
import torch

from conftest import ROOT
from geocalib_amd import _lib, fields
from abi_harness import assert_declared_exported_and_bound
from test_host_calls import STREAM, p, rec      # noqa: F401  (rec is a fixture)
from test_kernel_audit import kernel_metadata

TYPED_ARGS = ["int"] + ["const void*"] * 4 + ["int"] * 3 + ["float*"] * 5 + ["void*"]
BACKWARD_ARGS = ["int"] + ["const void*"] * 4 + ["int"] * 3 + ["const float*"] * 4 + ["void*"] * 5


def test_entry_points_are_declared_exported_bound_and_documented():
    args = assert_declared_exported_and_bound("gclm_pack_fields_typed", TYPED_ARGS)
    assert len(args) == 14 and [a for a in args if a is C.c_int] == [C.c_int] * 4
    args = assert_declared_exported_and_bound("gclm_pack_fields_backward", BACKWARD_ARGS)
    assert len(args) == 17 and [a for a in args if a is C.c_int] == [C.c_int] * 4
    header = open(os.path.join(ROOT, "include", "gclm.h")).read()
    changelog = header[header.index("ABI version:"):header.index("#define GCLM_VERSION")]
    assert "gclm_pack_fields_typed and gclm_pack_fields_backward added, also within 610" in changelog
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "| `gclm_pack_fields_typed` |" in doc and "| `gclm_pack_fields_backward` |" in doc


# fake, never dereferenced device addresses: every refused call below must be refused before the first HIP call
UPR, ULC, LATR, LLC = 0x1000000, 0x1100000, 0x1200000, 0x1300000
UP, UPC, LAT, LATC, SLAT = 0x5000000, 0x5100000, 0x5200000, 0x5300000, 0x5400000
GUP, GUPC, GLAT, GLATC = 0x6000000, 0x6100000, 0x6200000, 0x6300000
DUP, DUPC, DLAT, DLATC = 0x7000000, 0x7100000, 0x7200000, 0x7300000
PX = 2 * 6 * 8 * 4                       # bytes of a (B, h, w) float plane
HX = PX // 2                             # ... of 16-bit elements

# ------------------------------------------------------------------ gclm_pack_fields_typed
T_OK = dict(dt=2, upr=UPR, ulc=ULC, latr=LATR, llc=LLC, B=2, H=6, W=8, up=UP, upc=UPC, lat=LAT, latc=LATC, slat=SLAT)
T_BAD = [("dtype 3", dict(dt=3)), ("dtype -1", dict(dt=-1)), ("NULL up raw", dict(upr=None)), ("NULL latitude raw", dict(latr=None)),
         ("NULL up output", dict(up=None)), ("NULL latitude output", dict(lat=None)), ("float32: NULL up raw", dict(dt=0, upr=None)),
         ("H = 0", dict(H=0)), ("W = 0", dict(W=0)), ("W < 0", dict(W=-8)), ("B < 0", dict(B=-1)), ("float32: B < 0", dict(dt=0, B=-1)),
         ("up log-confidence without its output", dict(upc=None)), ("latitude log-confidence without its output", dict(latc=None)),
         ("half raws converted in place", dict(up=UPR)), ("half latitude converted in place", dict(dt=1, lat=LATR)),
         ("half log-confidence converted in place", dict(upc=ULC)),
         ("up output starts at the up raws' last element", dict(up=UPR + 2 * HX - 4)),
         ("latitude output ends one float inside the latitude raws", dict(lat=LATR - PX + 4)),
         ("up confidence on the latitude log-confidence", dict(upc=LLC)),
         ("latitude confidence on the up output's second plane", dict(latc=UP + PX)),
         ("sin(latitude) on the latitude output", dict(slat=LAT)), ("sin(latitude) on the up raws", dict(slat=UPR)),
         ("float32: sin(latitude) on the latitude raws", dict(dt=0, slat=LATR)),
         ("half raws off a 2-byte boundary", dict(upr=UPR + 1)), ("half log-confidence off a 2-byte boundary", dict(dt=1, llc=LLC + 3)),
         ("output off a 4-byte boundary", dict(lat=LAT + 2))]
T_NEIGHBOURS = [dict(), dict(dt=1), dict(dt=0), dict(H=1, W=1), dict(H=5, W=7), dict(ulc=None, upc=None), dict(llc=None, latc=None),
                dict(ulc=None, llc=None, upc=None, latc=None, slat=None), dict(ulc=None), dict(slat=None),
                dict(dt=0, up=UPR, lat=LATR, upc=ULC, latc=LLC),      # float32 stays legal in place
                dict(up=UPR + 2 * HX), dict(lat=LATR - PX), dict(upr=UPR + 2, latr=LATR + 6), dict(up=UP + 4, slat=SLAT + 12)]


def _typed(a):
    return _lib.load().gclm_pack_fields_typed(a["dt"], a["upr"], a["ulc"], a["latr"], a["llc"], a["B"], a["H"], a["W"], a["up"],
                                              a["upc"], a["lat"], a["latc"], a["slat"], None)


@pytest.mark.parametrize("what,change", T_BAD, ids=[b[0] for b in T_BAD])
def test_typed_forward_refuses_invalid_arguments_before_any_hip_call(what, change):
    assert set(change) <= set(T_OK) and 1 <= len(change) <= 2
    assert _typed({**T_OK, **change}) == -3, what


# ------------------------------------------------------------------ gclm_pack_fields_backward
B_OK = dict(dt=0, upr=UPR, ulc=ULC, latr=LATR, llc=LLC, B=2, H=6, W=8, gup=GUP, gupc=GUPC, glat=GLAT, glatc=GLATC, dup=DUP,
            dupc=DUPC, dlat=DLAT, dlatc=DLATC)
B_BAD = [("dtype 3", dict(dt=3)), ("dtype -1", dict(dt=-1)), ("H = 0", dict(H=0)), ("W = 0", dict(W=0)), ("H < 0", dict(H=-6)),
         ("B < 0", dict(B=-1)), ("no gradient asked for", dict(dup=None, dupc=None, dlat=None, dlatc=None)),
         ("up gradient without the up raws", dict(upr=None)), ("up gradient without its incoming gradient", dict(gup=None)),
         ("latitude gradient without the latitude raws", dict(latr=None)), ("latitude gradient without its incoming gradient", dict(glat=None)),
         ("up confidence gradient without its log-confidence", dict(ulc=None)),
         ("up confidence gradient without its incoming gradient", dict(gupc=None)),
         ("latitude confidence gradient without its log-confidence", dict(llc=None)),
         ("latitude confidence gradient without its incoming gradient", dict(glatc=None)),
         ("up gradient written over the up raws", dict(dup=UPR)), ("up gradient on its incoming gradient", dict(dup=GUP)),
         ("up gradient starts at the incoming gradient's last float", dict(dup=GUP + 2 * PX - 4)),
         ("latitude gradient ends one float inside the latitude raws", dict(dlat=LATR - PX + 4)),
         ("latitude gradient on the up gradient's second plane", dict(dlat=DUP + PX)),
         ("up confidence gradient on the latitude log-confidence", dict(dupc=LLC)),
         ("latitude confidence gradient on the up confidence's incoming gradient", dict(dlatc=GUPC)),
         ("half: up gradient ends one element inside the latitude gradient", dict(dt=1, dup=DLAT - 2 * HX + 2)),
         ("a gradient on a plane of a group not asked for", dict(dup=None, dlat=UPR)),
         ("float raws off a 4-byte boundary", dict(latr=LATR + 2)), ("half raws off a 2-byte boundary", dict(dt=2, upr=UPR + 1)),
         ("incoming gradient off a 4-byte boundary", dict(dt=1, glat=GLAT + 2)), ("float gradient off a 4-byte boundary", dict(dup=DUP + 2)),
         ("half gradient off a 2-byte boundary", dict(dt=1, dlatc=DLATC + 1))]
B_NEIGHBOURS = [dict(), dict(dt=1), dict(dt=2), dict(H=1, W=1), dict(H=5, W=7),
                dict(dupc=None, dlat=None, dlatc=None), dict(dup=None, dupc=None, dlatc=None), dict(dup=None, dlat=None, dlatc=None),
                dict(dup=None, dupc=None, dlat=None),
                dict(dup=None, upr=None, gup=None), dict(dlat=None, glat=None), dict(dupc=None, ulc=None, gupc=None),
                dict(dlatc=None, llc=None, glatc=None, dupc=None, ulc=None, gupc=None),
                dict(dup=GUP + 2 * PX), dict(dlat=LATR - PX), dict(dt=1, dup=DLAT - 2 * HX), dict(dt=2, upr=UPR + 2, dlat=DLAT + 6),
                dict(gup=GUP + 4, dupc=DUPC + 12)]


def _backward(a):
    return _lib.load().gclm_pack_fields_backward(a["dt"], a["upr"], a["ulc"], a["latr"], a["llc"], a["B"], a["H"], a["W"], a["gup"],
                                                 a["gupc"], a["glat"], a["glatc"], a["dup"], a["dupc"], a["dlat"], a["dlatc"], None)


@pytest.mark.parametrize("what,change", B_BAD, ids=[b[0] for b in B_BAD])
def test_backward_refuses_invalid_arguments_before_any_hip_call(what, change):
    assert set(change) <= set(B_OK) and 1 <= len(change) <= 4
    assert _backward({**B_OK, **change}) == -3, what


def test_an_empty_batch_succeeds_and_launches_nothing():
    for dt in (0, 1, 2):
        assert _typed({**T_OK, "dt": dt, "B": 0}) == 0
        assert _backward({**B_OK, "dt": dt, "B": 0}) == 0


def test_the_valid_neighbours_reach_the_launch():
    """The neighbours of the refused calls -- ranges that only touch, every dtype, absent confidences, every subset of the
    gradients, a group left out with all its planes -- are valid and reach the launch, which fails without a device: -10."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: a valid call would launch on fake addresses")
    for change in T_NEIGHBOURS:
        assert _typed({**T_OK, **change}) == -10, change
    for change in B_NEIGHBOURS:
        assert _backward({**B_OK, **change}) == -10, change


# ------------------------------------------------------------------ the build
def test_neither_epilogue_kernel_has_scratch_or_lds_in_any_instantiation(tmp_path):
    k = kernel_metadata(tmp_path)
    forward = {n: v for n, v in k.items() if "pack_fields_kernelILi" in n}
    backward = {n: v for n, v in k.items() if "pack_fields_backward_kernelILi" in n}
    # forward <VEC, DT>: float32 at 4 and 1 pixels per lane, the two 16-bit types at 8 and 1; backward <DT, VEC>: the same six
    assert sorted(n[n.index("ILi"):n.index("EEEv") + 1] for n in forward) == ["ILi1ELi0E", "ILi1ELi1E", "ILi1ELi2E", "ILi4ELi0E",
                                                                             "ILi8ELi1E", "ILi8ELi2E"], sorted(forward)
    assert sorted(n[n.index("ILi"):n.index("EEEv") + 1] for n in backward) == ["ILi0ELi1E", "ILi0ELi4E", "ILi1ELi1E", "ILi1ELi8E",
                                                                              "ILi2ELi1E", "ILi2ELi8E"], sorted(backward)
    for n, v in {**forward, **backward}.items():
        assert v["scratch"] == 0 and v["lds"] == 0, (n, v)


# ------------------------------------------------------------------ the calls pack_fields makes
def _raws(dtype=torch.float32):
    g = torch.Generator().manual_seed(1)
    return [torch.randn(s, generator=g).to(dtype) for s in ((2, 2, 2, 2), (2, 1, 2, 2), (2, 2, 2), (2, 1, 2, 2))]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=str)
def test_half_raws_are_handed_over_as_they_are(rec, dtype):      # noqa: F811
    up_raw, lat_raw, ulc, llc = _raws(dtype)
    out = fields.pack_fields(up_raw, lat_raw, ulc, llc, sin_latitude=True)
    assert all(v.dtype == torch.float32 for v in out.values()) and out["up_confidence"].shape == (2, 2, 2)
    assert rec.calls == [("gclm_pack_fields_typed", (
        _lib.LOGIT_DTYPE_IDS[str(dtype)[6:]], p(up_raw), p(ulc), p(lat_raw), p(llc), 2, 2, 2, p(out["up_field"]),
        p(out["up_confidence"]), p(out["latitude_field"]), p(out["latitude_confidence"]), p(out["sin_latitude"]), STREAM))]


def test_mixed_or_strided_half_raws_and_inplace_take_the_float32_call(rec):      # noqa: F811
    up_raw, lat_raw, ulc, llc = _raws(torch.bfloat16)
    fields.pack_fields(up_raw, lat_raw.half(), ulc, llc)
    fields.pack_fields(up_raw.transpose(2, 3), lat_raw)
    fields.pack_fields(up_raw, lat_raw, inplace=True)
    assert [c[0] for c in rec.calls] == ["gclm_pack_fields_ex"] * 3


def test_no_graph_without_grad_mode_or_with_inplace(rec):      # noqa: F811
    up_raw, lat_raw, ulc, llc = (t.requires_grad_() for t in _raws())
    with torch.no_grad():
        out = fields.pack_fields(up_raw, lat_raw, ulc, llc)
    assert all(not v.requires_grad for v in out.values())
    out = fields.pack_fields(up_raw.detach(), lat_raw.detach(), ulc.detach())
    assert all(v.grad_fn is None for v in out.values())
    out = fields.pack_fields(up_raw.detach().clone().requires_grad_(), lat_raw.detach().clone(), inplace=True)
    assert all(v.grad_fn is None for v in out.values())
    assert [c[0] for c in rec.calls] == ["gclm_pack_fields_ex"] * 3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_graph_forward_is_the_plain_call_and_backward_one_call_on_the_saved_raws(rec, dtype):      # noqa: F811
    up_raw, lat_raw, ulc, llc = (t.requires_grad_() for t in _raws(dtype))
    out = fields.pack_fields(up_raw, lat_raw, ulc, llc, sin_latitude=True)
    entry = "gclm_pack_fields_ex" if dtype is torch.float32 else "gclm_pack_fields_typed"
    assert [c[0] for c in rec.calls] == [entry]
    assert rec.calls[0][1][-13:-6] == (p(up_raw), p(ulc), p(lat_raw), p(llc), 2, 2, 2)
    assert all(out[k].grad_fn is not None for k in out if k != "sin_latitude") and not out["sin_latitude"].requires_grad
    g = [torch.ones_like(out[k]) for k in ("up_field", "latitude_field", "up_confidence", "latitude_confidence")]
    grads = torch.autograd.grad([out[k] for k in ("up_field", "latitude_field", "up_confidence", "latitude_confidence")],
                                [up_raw, lat_raw, ulc, llc], g)
    name, args = rec.calls[1]
    assert name == "gclm_pack_fields_backward" and len(rec.calls) == 2
    assert args[:8] == (_lib.LOGIT_DTYPE_IDS[str(dtype)[6:]], p(up_raw), p(ulc), p(lat_raw), p(llc), 2, 2, 2)
    assert args[8:12] == (p(g[0]), p(g[2]), p(g[1]), p(g[3]))
    assert args[12:] == (p(grads[0]), p(grads[2]), p(grads[1]), p(grads[3]), STREAM)
    assert [t.shape for t in grads] == [t.shape for t in (up_raw, lat_raw, ulc, llc)] and all(t.dtype is dtype for t in grads)


def test_backward_leaves_out_what_is_not_asked_for(rec):      # noqa: F811
    up_raw, lat_raw, ulc, llc = _raws()
    lat_raw.requires_grad_()
    ulc.requires_grad_()
    out = fields.pack_fields(up_raw, lat_raw, ulc, llc)
    # the latitude alone receives a gradient: the up confidence's raws get None, the others ask for nothing
    g = torch.ones_like(out["latitude_field"])
    grads = torch.autograd.grad(out["latitude_field"], [lat_raw, ulc], g, allow_unused=True)
    assert grads[1] is None
    args = rec.calls[1][1]
    assert args[1:5] == (None, None, p(lat_raw), None) and args[8:12] == (None, None, p(g), None)
    assert args[12:16] == (None, None, p(grads[0]), None)
    # an output whose raws ask for nothing: no call at all
    out = fields.pack_fields(up_raw, lat_raw, ulc, llc)
    assert torch.autograd.grad(out["up_field"].sum() + out["latitude_confidence"].sum(), [lat_raw, ulc], allow_unused=True) == (None, None)
    assert [c[0] for c in rec.calls] == ["gclm_pack_fields_ex", "gclm_pack_fields_backward", "gclm_pack_fields_ex"]


def test_mixed_and_strided_raws_get_their_gradients_in_their_own_dtype_and_shape(rec):      # noqa: F811
    up_raw, lat_raw, ulc, llc = _raws()
    up_raw = up_raw.transpose(2, 3).contiguous().transpose(2, 3).requires_grad_()       # strided
    lat_raw = lat_raw.to(torch.bfloat16).requires_grad_()                               # another dtype than the rest
    out = fields.pack_fields(up_raw, lat_raw, ulc, llc)
    grads = torch.autograd.grad(out["up_field"].sum() + out["latitude_field"].sum(), [up_raw, lat_raw])
    assert rec.calls[1][1][0] == 0 and [c[0] for c in rec.calls] == ["gclm_pack_fields_ex", "gclm_pack_fields_backward"]
    assert grads[0].shape == up_raw.shape and grads[0].dtype is torch.float32
    assert grads[1].shape == lat_raw.shape and grads[1].dtype is torch.bfloat16


def test_cpu_tensors_are_still_refused():
    up_raw, lat_raw = torch.zeros(1, 2, 2, 2), torch.zeros(1, 1, 2, 2)
    for a, b in ((up_raw, lat_raw), (up_raw.clone().requires_grad_(), lat_raw), (up_raw.bfloat16(), lat_raw.bfloat16())):
        with pytest.raises(RuntimeError, match="must live on a HIP device"):
            fields.pack_fields(a, b)
