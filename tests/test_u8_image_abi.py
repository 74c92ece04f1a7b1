"""CPU: the uint8 image calls without a device -- gclm_undistort_image_u8 and gclm_reproject_image_u8 are declared, exported,
bound and documented; every invalid argument is refused before any HIP call, overlaps to the byte; the gate of
tests/test_u8_image.py (tests/u8_image_gate.py) keeps the float gates' conditions on every case, passes an honest float32
evaluation that is rounded and clamped, and fails its mutants; Camera.undistort_image / reproject_image / upright_image on a
uint8 CPU image are the rounded, clamped float32 composition in the input's memory format; and the byte kernels exist for
every model and layout without scratch or LDS, beside an unchanged set of float kernels."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT
from geocalib_amd import Gravity, _lib, camera_models
from abi_harness import LLVM, assert_declared_exported_and_bound
import reproject_gate as rg
import u8_image_gate as u8g
import undistort_gate as ug

UND_ARGS = ["int", "const float*", "int", "const unsigned char*"] + ["int"] * 7 + ["unsigned char*", "void*"]
REP_ARGS = ["int", "const float*", "int", "const float*", "int", "const float*", "int", "const unsigned char*"] + ["int"] * 9 + \
           ["unsigned char*", "unsigned char*", "void*"]


def test_entry_points_are_declared_exported_bound_and_documented():
    args = assert_declared_exported_and_bound("gclm_undistort_image_u8", UND_ARGS)
    assert len(args) == 13 and [a for a in args if a is C.c_int] == [C.c_int] * 9
    args = assert_declared_exported_and_bound("gclm_reproject_image_u8", REP_ARGS)
    assert len(args) == 20 and [a for a in args if a is C.c_int] == [C.c_int] * 13
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "| `gclm_undistort_image_u8` |" in doc and "| `gclm_reproject_image_u8` |" in doc
    header = open(os.path.join(ROOT, "include", "gclm.h")).read()
    assert "gclm_undistort_image_u8 and gclm_reproject_image_u8 added, also within 610" in header


# ------------------------------------------------------------------ refusals
# fake, never dereferenced device addresses: every call below must be refused before the first HIP call.  The byte images sit
# at odd addresses on purpose: they carry no alignment requirement.
SCAM, TCAM, ROT, SRC, DST, VALID = 0x100000, 0x300000, 0x500000, 0x800001, 0x4000003, 0x5000001
R_OK = dict(sm=1, scam=SCAM, tm=0, tcam=TCAM, nb=1, rot=ROT, nr=1, src=SRC, B=2, C=3, Hin=41, Win=59, Hs=30, Ws=44, H=48, W=64,
            il=1, dst=DST, valid=VALID)
DST_BYTES, VALID_BYTES, SRC_BYTES = 2 * 3 * 48 * 64, 2 * 48 * 64, 2 * 3 * 41 * 59
R_BAD = [("NULL source camera", dict(scam=None)), ("NULL target camera", dict(tcam=None)), ("NULL source", dict(src=None)),
         ("NULL destination", dict(dst=None)), ("source model -1", dict(sm=-1)), ("source model 4", dict(sm=4)),
         ("target model -1", dict(tm=-1)), ("target model 4", dict(tm=4)), ("B = 0", dict(B=0)), ("B > 65535", dict(B=65536)),
         ("C = 0", dict(C=0)), ("Hin = 0", dict(Hin=0)), ("Win = 0", dict(Win=0)), ("H = 0", dict(H=0)), ("W = 0", dict(W=0)),
         ("Hs = 1", dict(Hs=1)), ("Ws = 1", dict(Ws=1)), ("H * W > 2^31 - 1", dict(H=65536, W=32768)),
         ("cam_batch 0", dict(nb=0)), ("cam_batch 3 of B = 2", dict(nb=3)), ("rot_batch 0", dict(nr=0)),
         ("rot_batch 3 of B = 2", dict(nr=3)), ("rot_batch 3 of B = 2 without a rotation", dict(nr=3, rot=None)),
         ("interleaved = 2", dict(il=2)), ("interleaved = -1", dict(il=-1)), ("interleaved with C = 5", dict(C=5)),
         ("destination starts one byte before the source's end", dict(dst=SRC + SRC_BYTES - 1)),
         ("source starts one byte before the destination's end", dict(src=DST + DST_BYTES - 1)),
         ("destination is the source", dict(dst=SRC)),
         ("destination ends one byte inside the source camera", dict(dst=SCAM - DST_BYTES + 1)),
         ("destination starts at the target camera's last byte", dict(dst=TCAM + 31)),
         ("destination starts at the rotation's last byte", dict(dst=ROT + 35)),
         ("mask starts at the source's last byte", dict(valid=SRC + SRC_BYTES - 1)),
         ("mask starts at the source camera's last byte", dict(valid=SCAM + 31)),
         ("mask ends one byte inside the target camera", dict(valid=TCAM - VALID_BYTES + 1)),
         ("mask starts at the rotation's last byte", dict(valid=ROT + 35)),
         ("mask inside the destination", dict(valid=DST + 100)),
         ("destination ends one byte inside the mask", dict(dst=VALID - DST_BYTES + 1)),
         ("source camera off a 4-byte boundary", dict(scam=SCAM + 2)), ("rotation off a 4-byte boundary", dict(rot=ROT + 2))]
R_NEIGHBOURS = [dict(), dict(il=0), dict(il=0, C=5), dict(C=4), dict(valid=None), dict(rot=None), dict(nb=2, nr=2),
                dict(H=1, W=1), dict(dst=SRC + SRC_BYTES), dict(src=DST + DST_BYTES), dict(valid=DST + DST_BYTES),
                dict(dst=VALID - DST_BYTES), dict(dst=TCAM + 32), dict(src=SRC + 1, dst=DST + 2)]

CAM, USRC, UDST = 0x100000, 0x200001, 0x4000003
U_OK = dict(model=1, cam=CAM, nb=1, src=USRC, B=2, C=3, Hin=40, Win=60, H=48, W=64, il=1, dst=UDST)
U_SRC_BYTES, U_DST_BYTES = 2 * 3 * 40 * 60, 2 * 3 * 48 * 64
U_BAD = [("NULL camera", dict(cam=None)), ("NULL source", dict(src=None)), ("NULL destination", dict(dst=None)),
         ("B = 0", dict(B=0)), ("C = 0", dict(C=0)), ("Hin = 0", dict(Hin=0)), ("Win = 0", dict(Win=0)),
         ("H = 1", dict(H=1)), ("W = 1", dict(W=1)), ("H = 0", dict(H=0)), ("cam_batch 0", dict(nb=0)),
         ("cam_batch 3 of B = 2", dict(nb=3)), ("model -1", dict(model=-1)), ("model 4", dict(model=4)),
         ("B > 65535", dict(B=65536)), ("H * W > 2^31 - 1", dict(H=65536, W=32768)),
         ("interleaved = 2", dict(il=2)), ("interleaved = -1", dict(il=-1)), ("interleaved with C = 5", dict(C=5)),
         ("destination starts one byte before the source's end", dict(dst=USRC + U_SRC_BYTES - 1)),
         ("source starts one byte before the destination's end", dict(src=UDST + U_DST_BYTES - 1)),
         ("same buffer", dict(dst=USRC))]
U_NEIGHBOURS = [dict(), dict(il=0), dict(il=0, C=5), dict(C=4), dict(nb=2), dict(dst=USRC + U_SRC_BYTES),
                dict(src=UDST + U_DST_BYTES), dict(src=USRC + 1, dst=UDST + 2)]


def _reproject(a):
    return _lib.load().gclm_reproject_image_u8(a["sm"], a["scam"], a["tm"], a["tcam"], a["nb"], a["rot"], a["nr"], a["src"], a["B"],
                                               a["C"], a["Hin"], a["Win"], a["Hs"], a["Ws"], a["H"], a["W"], a["il"], a["dst"],
                                               a["valid"], None)


def _undistort(a):
    return _lib.load().gclm_undistort_image_u8(a["model"], a["cam"], a["nb"], a["src"], a["B"], a["C"], a["Hin"], a["Win"], a["H"],
                                               a["W"], a["il"], a["dst"], None)


@pytest.mark.parametrize("what,change", R_BAD, ids=[b[0] for b in R_BAD])
def test_reproject_refuses_invalid_arguments_before_any_hip_call(what, change):
    assert _reproject({**R_OK, **change}) == -3, what


@pytest.mark.parametrize("what,change", U_BAD, ids=[b[0] for b in U_BAD])
def test_undistort_refuses_invalid_arguments_before_any_hip_call(what, change):
    assert _undistort({**U_OK, **change}) == -3, what


def test_the_refusal_tables_change_one_thing_at_a_time():
    assert all(set(change) <= set(R_OK) and 1 <= len(change) <= 2 for _, change in R_BAD)
    assert all(set(change) <= set(U_OK) and 1 <= len(change) <= 2 for _, change in U_BAD)


def test_the_valid_neighbours_reach_the_launch():
    """The neighbours of the refused calls -- ranges that only touch, the other layout, C = 5 planar, odd addresses -- are valid
    and reach the launch, which fails without a device: -10, not -3."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: a valid call would launch on fake addresses")
    for change in R_NEIGHBOURS:
        assert _reproject({**R_OK, **change}) == -10, change
    for change in U_NEIGHBOURS:
        assert _undistort({**U_OK, **change}) == -10, change


# ------------------------------------------------------------------ the gate's own conditions, for every case
@pytest.fixture(scope="module")
def parts():
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = u8g.reproject_parts(case)
        return cache[case]
    return get


@pytest.mark.parametrize("case", rg.CASES, ids=[rg.case_id(c) for c in rg.CASES])
def test_reproject_gate_passes_an_honest_rounded_float32_evaluation(parts, case):
    p = parts(case)
    share = p["ex"].double().mean(dim=(1, 2)).max().item()
    assert p["img"].dtype == torch.uint8 and p["img"].max() > 200 and p["img"].float().std() > 20
    out = u8g.quantise(ug.bilinear32(p["img"].float(), *rg.sample_at(p["c32"])))
    ratio = u8g.worst_ratio(out, p["ref"], p["bound"])
    print(f"{rg.case_id(case)}: delta {p['delta']:.2e} px, excluded {share:.4f}, honest rounded float32 worst ratio {ratio:.3f}")
    assert share <= rg.CAP, share                       # the float gate's condition on the cases, inherited unchanged
    assert ratio <= 1, ratio


@pytest.mark.parametrize("case", ug.CASES, ids=[u8g.undistort_id(c) for c in ug.CASES])
def test_undistort_gate_passes_an_honest_rounded_float32_evaluation(case):
    model, k1, k2, B, nb, C, H, W, Hin, Win, kind = case
    p = u8g.undistort_parts(case)
    jx, jy = ug.coordinates(model, p["cams"], H, W, Hin, Win, torch.float32)
    out = u8g.quantise(ug.bilinear32(p["img"].float(), jx, jy))
    ratio = u8g.worst_ratio(out, p["ref"], p["bound"])
    print(f"{u8g.undistort_id(case)}: delta {p['delta']:.2e} px, honest rounded float32 worst ratio {ratio:.3f}")
    assert ratio <= 1, ratio


MUTANTS = ["truncation", "source read as 0..1", "channels reversed", "shift"]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_gate_fails_each_mutant(parts, mutant):
    case = next(c for c in rg.CASES if (c[0], c[4], c[7], c[12]) == ("pinhole", "pinhole", "none", "noise"))
    p = parts(case)
    img = p["img"].float()
    honest = ug.bilinear32(img / 255 if mutant == "source read as 0..1" else img, *rg.sample_at(p["c32"]))
    if mutant == "truncation":
        out = honest.floor().clamp(0, 255).to(torch.uint8)
    else:
        out = u8g.quantise(honest)
    if mutant == "channels reversed":
        out = out.flip(1)
    elif mutant == "shift":
        out = torch.roll(out, 1, dims=-1)
    ratio = u8g.worst_ratio(out, p["ref"], p["bound"])
    print(f"{mutant}: worst ratio {ratio:.3g}")
    assert ratio > 1, (mutant, ratio)


# ------------------------------------------------------------------ the public methods on the CPU
def _layouts(img):
    cl = img.contiguous(memory_format=torch.channels_last)
    assert not cl.is_contiguous() and cl.is_contiguous(memory_format=torch.channels_last)
    return (img, False), (cl, True)


@pytest.mark.parametrize("model", ug.MODELS)
def test_undistort_image_on_uint8(model):
    cams = ug.make_cameras(model, 1, 30, 41, seed=3)
    cam = camera_models[model](cams)
    img = u8g.to_bytes(ug.make_images("noise", 2, 3, 36, 50, seed=4))
    want = cam.undistort_image(img.float()).round().clamp(0, 255).to(torch.uint8)
    assert want.float().std() > 20
    for im, cl in _layouts(img):
        out = cam.undistort_image(im)
        assert out.dtype == torch.uint8 and out.shape == (2, 3, 30, 41) and torch.equal(out, want)
        assert out.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)


@pytest.mark.parametrize("case", rg.CASES[:8], ids=[rg.case_id(c) for c in rg.CASES[:8]])
def test_reproject_image_on_uint8(parts, case):
    p = parts(case)
    src, tgt = camera_models[case[0]](p["src"]), camera_models[case[4]](p["tgt"])
    want, want_valid = src.reproject_image(p["img"].float(), tgt, p["rot"], return_valid=True)
    want = want.round().clamp(0, 255).to(torch.uint8)
    for im, cl in _layouts(p["img"]):
        out, valid = src.reproject_image(im, tgt, p["rot"], return_valid=True)
        assert out.dtype == torch.uint8 and torch.equal(out, want) and torch.equal(valid, want_valid)
        assert out.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
        assert torch.equal(src.reproject_image(im, tgt, p["rot"]), want)


def test_upright_image_on_uint8():
    cams = ug.make_cameras("simple_radial", 1, 30, 44, seed=9)
    cam, img = camera_models["simple_radial"](cams), u8g.to_bytes(ug.make_images("noise", 3, 2, 30, 44, seed=9))
    grav = Gravity.from_rp(torch.tensor([0.3, -0.5, 0.1]), torch.tensor([0.2, 0.4, -0.3]))
    for level in (False, True):
        want, want_valid = cam.upright_image(img.float(), grav, level_pitch=level, return_valid=True)
        want = want.round().clamp(0, 255).to(torch.uint8)
        for im, cl in _layouts(img):
            out, valid = cam.upright_image(im, grav, level_pitch=level, return_valid=True)
            assert out.dtype == torch.uint8 and torch.equal(out, want) and torch.equal(valid, want_valid) and valid.any()
            assert out.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)


def test_other_dtypes_keep_their_behaviour():
    cam = camera_models["radial"](ug.make_cameras("radial", 1, 20, 30, seed=5))
    assert cam.undistort_image(torch.rand(1, 1, 20, 30, dtype=torch.float64)).dtype == torch.float64
    assert cam.reproject_image(torch.rand(1, 1, 20, 30)).dtype == torch.float32
    with pytest.raises(RuntimeError):                                  # grid_sample takes no integers: as before
        cam.reproject_image(torch.zeros(1, 1, 20, 30, dtype=torch.int16))


# ------------------------------------------------------------------ code objects
# Most VGPRs of any instantiation, as the build gives them: undistort_u8 planar 18, interleaved 24;
# reproject_u8 planar 19, interleaved 21 (the interleaved kernels hold the dword path's four taps).  Pinned a few registers
# above: all far below the 64 the float kernels are held to, so every SIMD holds its 8 waves.
VGPR_MAX = {("undistort", 0): 24, ("undistort", 1): 28, ("reproject", 0): 24, ("reproject", 1): 28}


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="LLVM tools missing")
def test_byte_kernels_exist_for_every_model_and_layout_without_scratch(tmp_path):
    from test_kernel_audit import kernel_metadata
    k = kernel_metadata(tmp_path)
    # the byte instantiations of the one kernel template per warp: element type `h` (unsigned char), then the layout
    und = {n: v for n, v in k.items() if re.search(r"undistort_image_kernelILi\dEhLb\dEEEv", n)}
    rep = {n: v for n, v in k.items() if re.search(r"reproject_kernelILi\dELi\dELb\dEhLb\dEEEv", n)}
    assert len(und) == 8 and len(rep) == 64, (sorted(und), sorted(rep))
    for il in range(2):
        for m in range(4):
            v = [v for n, v in und.items() if f"undistort_image_kernelILi{m}EhLb{il}E" in n]
            assert len(v) == 1 and v[0]["vgpr"] <= VGPR_MAX[("undistort", il)], (m, il, v)
            for t in range(4):
                for r in range(2):
                    v = [v for n, v in rep.items() if f"reproject_kernelILi{m}ELi{t}ELb{r}EhLb{il}E" in n]
                    assert len(v) == 1 and v[0]["vgpr"] <= VGPR_MAX[("reproject", il)], (m, t, r, il, v)
    assert all(v["scratch"] == 0 and v["lds"] == 0 for v in {**und, **rep}.values()), {**und, **rep}
    print("most VGPRs:", {(name, il): max(v["vgpr"] for n, v in group.items() if f"EhLb{il}EEEv" in n)
                          for name, group in (("undistort", und), ("reproject", rep)) for il in range(2)})
    # the symbol counts the existing audits pin are what they were
    count = lambda s: sum(s in n for n in k)  # noqa: E731
    float_count = lambda s: sum(bool(re.search(s + r"\w*EfLb0EEEv", n)) for n in k)  # noqa: E731
    assert float_count("reproject_kernelILi") == 32 and float_count("undistort_image_kernelILi") == 4
    assert count("reproject_kernel") == 32 + 64 and count("undistort_image_kernel") == 4 + 8
    assert count("sweep_kernelILi") == 100 and count("fused_step_kernelILi") == 56
