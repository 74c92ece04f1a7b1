"""CPU: Camera.reproject_image / upright_image and gclm_reproject_image without a device -- the entry point is declared,
exported, bound and documented, every invalid argument is refused before any HIP call, the gate of
tests/test_reproject_image.py (tests/reproject_gate.py) keeps its conditions on every case and passes an honest float32
evaluation, the public methods in float64 equal the yardstick, the rotation convention of upright_image is held to a known
answer (and its transpose fails it), and the kernels carry no scratch and no LDS."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from conftest import ROOT
from geocalib_amd import Gravity, _lib, camera_models
from geocalib_amd.perspective_fields import get_perspective_field
from abi_harness import LLVM, assert_declared_exported_and_bound
import reproject_gate as rg
import undistort_gate as ug

ARGS = ["int", "const float*", "int", "const float*", "int", "const float*", "int", "const float*"] + ["int"] * 8 + \
       ["float*", "unsigned char*", "void*"]


def test_entry_point_is_declared_exported_bound_and_documented():
    args = assert_declared_exported_and_bound("gclm_reproject_image", ARGS)
    assert len(args) == 19 and [a for a in args if a is C.c_int] == [C.c_int] * 12
    assert "| `gclm_reproject_image` |" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "gclm_reproject.hip" in open(os.path.join(ROOT, "geocalib_amd", "csrc", "Makefile")).read()
    for cls in camera_models.values():
        assert callable(getattr(cls, "reproject_image", None)) and callable(getattr(cls, "upright_image", None))


# fake, never dereferenced device addresses: every call below must be refused before the first HIP call
SCAM, TCAM, ROT, SRC, DST, VALID = 0x100000, 0x300000, 0x500000, 0x800000, 0x4000000, 0x5000000
OK = dict(sm=1, scam=SCAM, tm=0, tcam=TCAM, nb=1, rot=ROT, nr=1, src=SRC, B=2, C=3, Hin=41, Win=59, Hs=30, Ws=44, H=48, W=64,
          dst=DST, valid=VALID)
DST_BYTES, VALID_BYTES, SRC_BYTES = 4 * 2 * 3 * 48 * 64, 2 * 48 * 64, 4 * 2 * 3 * 41 * 59
BAD = [("NULL source camera", dict(scam=None)), ("NULL target camera", dict(tcam=None)), ("NULL source", dict(src=None)),
       ("NULL destination", dict(dst=None)), ("source model -1", dict(sm=-1)), ("source model 4", dict(sm=4)),
       ("target model -1", dict(tm=-1)), ("target model 4", dict(tm=4)), ("B = 0", dict(B=0)), ("B > 65535", dict(B=65536)),
       ("C = 0", dict(C=0)), ("Hin = 0", dict(Hin=0)), ("Win = 0", dict(Win=0)), ("H = 0", dict(H=0)), ("W = 0", dict(W=0)),
       ("Hs = 1", dict(Hs=1)), ("Ws = 1", dict(Ws=1)), ("H * W > 2^31 - 1", dict(H=65536, W=32768)),
       ("cam_batch 0", dict(nb=0)), ("cam_batch 3 of B = 2", dict(nb=3)), ("rot_batch 0", dict(nr=0)),
       ("rot_batch 3 of B = 2", dict(nr=3)), ("rot_batch 3 of B = 2 without a rotation", dict(nr=3, rot=None)),
       ("destination overlaps the source", dict(dst=SRC + 4096)),
       ("source starts inside the destination", dict(src=DST + DST_BYTES - 4)),
       ("destination is the source", dict(dst=SRC)),
       ("destination overlaps the source camera", dict(dst=SCAM - DST_BYTES + 4)),
       ("destination overlaps the target camera", dict(dst=TCAM + 28)),
       ("destination overlaps the rotation", dict(dst=ROT + 32)),
       ("mask overlaps the source", dict(valid=SRC + SRC_BYTES - 1)),
       ("mask overlaps the source camera", dict(valid=SCAM + 31)),
       ("mask overlaps the target camera", dict(valid=TCAM - VALID_BYTES + 1)),
       ("mask overlaps the rotation", dict(valid=ROT + 35)),
       ("mask inside the destination", dict(valid=DST + 100)),
       ("destination ends inside the mask", dict(dst=VALID - DST_BYTES + 4)),
       ("destination off a 4-byte boundary", dict(dst=DST + 2)), ("source off a 4-byte boundary", dict(src=SRC + 1)),
       ("rotation off a 4-byte boundary", dict(rot=ROT + 2))]


def _call(a):
    return _lib.load().gclm_reproject_image(a["sm"], a["scam"], a["tm"], a["tcam"], a["nb"], a["rot"], a["nr"], a["src"], a["B"],
                                            a["C"], a["Hin"], a["Win"], a["Hs"], a["Ws"], a["H"], a["W"], a["dst"], a["valid"], None)


@pytest.mark.parametrize("what,change", BAD, ids=[b[0] for b in BAD])
def test_invalid_arguments_are_refused_before_any_hip_call(what, change):
    assert _call({**OK, **change}) == -3, what


def test_the_refusal_table_changes_one_thing_at_a_time():
    """Every refused call is the valid call with one argument (or one batch and its pointer) changed; the neighbours of the
    overlapping ranges that only touch are valid and reach the launch, which fails without a device: not -3."""
    assert all(set(change) <= set(OK) and 1 <= len(change) <= 2 for _, change in BAD)
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: a valid call would launch on fake addresses")
    for change in (dict(), dict(valid=None), dict(rot=None), dict(nb=2, nr=2), dict(H=1, W=1), dict(dst=SRC + SRC_BYTES),
                   dict(valid=DST + DST_BYTES), dict(dst=TCAM + 32)):
        assert _call({**OK, **change}) == -10, change


# ------------------------------------------------------------------ the gate's own conditions, for every case
@pytest.fixture(scope="module")
def parts():
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = rg.case_parts(case)
        return cache[case]
    return get


@pytest.mark.parametrize("case", rg.CASES, ids=[rg.case_id(c) for c in rg.CASES])
def test_gate_conditions_and_an_honest_float32_evaluation(parts, case):
    p = parts(case)
    H, W = case[10], case[11]
    share = p["ex"].double().mean(dim=(1, 2)).max().item()
    seen = p["valid"].double().mean().item()
    c32 = p["c32"]
    out32 = ug.bilinear32(p["img"], *rg.sample_at(c32))
    ratio = rg.worst_ratio(out32, p["ref"], p["bound"])
    valid32 = rg.in_image(c32, rg.HIN, rg.WIN).expand(rg.B, -1, -1)
    print(f"{rg.case_id(case)}: delta {p['delta']:.2e} px, excluded {share:.4f} of the worst image, valid {seen:.3f}, "
          f"honest float32 worst ratio {ratio:.3f}")
    assert share <= rg.CAP, share
    assert p["ref"].shape == (rg.B, rg.C, H, W) and p["delta"] < 0.05
    assert ratio <= 0.5, ratio
    assert torch.equal(valid32 | p["mask_free"], p["valid"] | p["mask_free"])
    if case[7] == "yaw100":
        assert seen == 0 and (p["ref"] == 0).all() and (~p["c64"]["visible"]).double().mean() > 0.5
    else:
        assert seen > 0.05, seen                        # (the case is not trivially empty)


def test_the_fold_and_the_clamp_lie_inside_the_image(parts):
    """simple_radial k1 = -0.3 at f = 0.5 W folds inside the image (pixels fail inside_model); simple_divisional k1 = 2 crosses
    its tau = 0 clamp there."""
    by = {(c[0], c[1], c[4]): c for c in rg.CASES}
    p = parts(by[("simple_radial", -0.3, "pinhole")])
    folded = p["c64"]["visible"] & ~p["c64"]["ok"]
    assert 0.01 < folded.double().mean().item() < 0.5
    case = by[("simple_divisional", 2.0, "simple_radial")]
    tau = 1 - 4 * 2.0 * parts(case)["c64"]["r2s"]
    assert 0.01 < (tau <= 0).double().mean().item() < 0.9 and (tau.abs() < 0.02).any()


MUTANTS = ["transposed rotation", "shift", "no visibility test", "no fold test", "nominal size ignored", "border"]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_gate_fails_each_mutant(parts, mutant):
    by = {(c[0], c[1], c[4], c[7]): c for c in rg.CASES}
    case = {"transposed rotation": by[("radial", None, "pinhole", "roll25")], "shift": by[("pinhole", None, "pinhole", "none")],
            "no visibility test": by[("radial", None, "simple_divisional", "yaw100")],
            "no fold test": by[("simple_radial", -0.3, "pinhole", "none")],
            "nominal size ignored": by[("simple_divisional", None, "pinhole", "none")],
            "border": by[("radial", -0.7, "pinhole", "level")]}[mutant]
    p = parts(case)
    src, tgt, rot, img = p["src"], p["tgt"], p["rot"], p["img"]
    geo = dict(H=case[10], W=case[11], Hs=rg.HS, Ws=rg.WS, Hin=rg.HIN, Win=rg.WIN)
    c = dict(p["c64"])
    padding = "zeros"
    if mutant == "transposed rotation":
        c = rg.coordinates(case[0], src, case[4], tgt, rot.transpose(-1, -2), **geo)
    elif mutant == "shift":
        c["ix"] = c["ix"] + 0.05
    elif mutant == "no visibility test":
        full = rg.coordinates(case[0], src, case[4], tgt, rot, **geo)
        c["ok"] = full["mono"] > 0
    elif mutant == "no fold test":
        c["ok"] = c["visible"]
    elif mutant == "nominal size ignored":
        c = rg.coordinates(case[0], src, case[4], tgt, rot, **{**geo, "Hs": rg.HIN, "Ws": rg.WIN})
    else:
        padding = "border"
    gx, gy = rg.sample_at(c)
    out = ug.grid_sample64(img.double(), gx, gy, padding_mode=padding)
    if padding == "border":
        out = torch.where((gx == -2)[:, None].expand_as(out), torch.zeros_like(out), out)
    ratio = rg.worst_ratio(out, p["ref"], p["bound"])
    print(f"{mutant} on {rg.case_id(case)}: worst ratio {ratio:.3g}")
    assert ratio > 1, (mutant, ratio)


@pytest.mark.parametrize("model", ug.MODELS)
def test_yardstick_with_identity_and_default_target_is_the_undistort_yardstick(model):
    H, W, Hin, Win = 31, 40, 45, 29
    cams = ug.make_cameras(model, 3, H, W, seed=3)
    pin = torch.cat([cams[:, :6], torch.zeros(3, 2)], -1)
    ix, iy = ug.coordinates(model, cams, H, W, Hin, Win)
    for rot in (None, torch.eye(3)[None]):
        c = rg.coordinates(model, cams, "pinhole", pin, rot, H, W, H, W, Hin, Win)
        assert (c["ix"] - ix).abs().max() <= 1e-12 and (c["iy"] - iy).abs().max() <= 1e-12
        assert c["visible"].all()


# ------------------------------------------------------------------ the public methods
@pytest.mark.parametrize("case", rg.CASES, ids=[rg.case_id(c) for c in rg.CASES])
def test_public_method_in_float64_equals_the_yardstick(parts, case):
    p = parts(case)
    src, tgt = camera_models[case[0]](p["src"].double()), camera_models[case[4]](p["tgt"].double())
    rot = None if p["rot"] is None else p["rot"].double()
    out, valid = src.reproject_image(p["img"].double(), tgt, rot, return_valid=True)
    assert out.dtype == torch.float64 and out.shape == p["ref"].shape and valid.dtype == torch.bool
    keep = torch.isfinite(p["bound"])
    assert (out - p["ref"])[keep].abs().max() <= 1e-9
    assert torch.equal(valid | p["mask_free"], p["valid"] | p["mask_free"])
    assert torch.equal(src.reproject_image(p["img"].double(), tgt, rot), out)
    if rot is not None and rot.shape[0] == 1:
        assert torch.equal(src.reproject_image(p["img"].double(), tgt, rot[0]), out)          # a (3, 3) rotation


def test_default_target_is_the_source_without_distortion():
    cams = ug.make_cameras("radial", 1, 30, 44, seed=8).double()
    img = ug.make_images("smooth", 2, 3, 30, 44, seed=8).double()
    cam = camera_models["radial"](cams)
    out = cam.reproject_image(img)
    assert torch.equal(out, cam.reproject_image(img, camera_models["pinhole"](cams[:, :6])))
    und = cam.undistort_image(img)                      # the reference's composition: no fold test, its own cancelling forms
    c = rg.coordinates("radial", cams, "pinhole", cam.pinhole()._data, None, 30, 44, 30, 44, 30, 44)
    ok = c["ok"].expand(2, -1, -1)[:, None].expand_as(out)
    assert (out - und)[ok].abs().max() <= 1e-9 and (out[~ok] == 0).all()


# Known answer: the latitude field of a tilted pinhole camera, warped upright, is the latitude field of the upright camera.
# Float64 composition, worst error over the valid pixels of all twelve runs below: 0.0098 deg, bilinear interpolation of the
# field alone; gate 0.02 deg = 2 x that.  With M transposed: 5.3 deg (the (5, 3) deg camera) to 87 deg.
LAT_GATE_DEG = 0.02
LAT_RUNS = [(H, W, r, p, lv) for H, W in ((30, 44), (48, 64)) for r, p in ((25.0, -15.0), (-40.0, 30.0), (5.0, 3.0))
            for lv in (False, True)]


def latitude_known_answer(H, W, roll, pitch, level, device="cpu", dtype=torch.float64, transpose=False):
    """Worst error in degrees, over the valid pixels, of the warped latitude field against the upright camera's."""
    cam = camera_models["pinhole"](torch.tensor([[W, H, 0.8 * W, 0.8 * W, W / 2, H / 2, 0, 0]], dtype=dtype, device=device))
    rp = torch.tensor([[math.radians(roll), math.radians(pitch)]], dtype=dtype, device=device)
    grav = Gravity.from_rp(rp[:, 0], rp[:, 1])
    upright = Gravity.from_rp(torch.zeros_like(rp[:, 0]), torch.zeros_like(rp[:, 1]) if level else grav.pitch)
    lat = get_perspective_field(cam, grav)[1]
    want = get_perspective_field(cam, upright)[1]
    if transpose:
        M = upright.R @ grav.R.transpose(-1, -2)
        got, valid = cam.reproject_image(lat, rotation=M.transpose(-1, -2), return_valid=True)
    else:
        got, valid = cam.upright_image(lat, grav, level_pitch=level, return_valid=True)
    assert got.shape == want.shape == (1, 1, H, W) and valid.shape == (1, H, W) and valid.float().mean() > 0.3
    return torch.rad2deg((got - want)[valid[:, None]].abs().max()).item()


def test_upright_image_levels_the_latitude_field():
    worst = max(latitude_known_answer(*run) for run in LAT_RUNS)
    print(f"float64 composition: worst latitude error {worst:.4f} deg (gate {LAT_GATE_DEG})")
    assert worst <= LAT_GATE_DEG, worst


def test_the_transposed_rotation_fails_the_known_answer():
    errs = [latitude_known_answer(*run, transpose=True) for run in LAT_RUNS]
    print(f"M transposed: latitude errors {min(errs):.1f} .. {max(errs):.1f} deg")
    assert min(errs) > 10 * LAT_GATE_DEG, errs


def test_upright_image_is_reproject_image_with_rt_rs_transposed():
    cams = ug.make_cameras("simple_radial", 1, 30, 44, seed=9).double()
    cam, img = camera_models["simple_radial"](cams), ug.make_images("noise", 3, 2, 30, 44, seed=9).double()
    grav = Gravity.from_rp(torch.tensor([0.3, -0.5, 0.1]).double(), torch.tensor([0.2, 0.4, -0.3]).double())
    for level in (False, True):
        R_t = Gravity.from_rp(torch.zeros(3).double(), torch.zeros(3).double() if level else grav.pitch).R
        want = cam.reproject_image(img, rotation=R_t @ grav.R.transpose(-1, -2))
        assert torch.equal(cam.upright_image(img, grav, level_pitch=level), want)
    assert (cam.upright_image(img, grav) - cam.upright_image(img, grav, level_pitch=True)).abs().max() > 0.1


def test_batch_and_shape_errors_name_their_reason():
    cams = ug.make_cameras("radial", 3, 20, 30, seed=5)
    cam, img = camera_models["radial"](cams), torch.rand(2, 1, 20, 30)
    with pytest.raises(ValueError, match="source camera batch 3"):
        cam.reproject_image(img)
    one = camera_models["radial"](cams[:1])
    with pytest.raises(ValueError, match="target camera batch 3"):
        one.reproject_image(img, target=cam)
    with pytest.raises(ValueError, match="rotation batch 3"):
        one.reproject_image(img, rotation=torch.eye(3).expand(3, 3, 3))
    with pytest.raises(ValueError, match="`rotation` must be"):
        one.reproject_image(img, rotation=torch.eye(4))
    with pytest.raises(ValueError, match="`target` must be a camera"):
        one.reproject_image(img, target=cams)
    with pytest.raises(ValueError, match="expected a .B, C, H, W. image"):
        one.reproject_image(img[0])
    with pytest.raises(ValueError, match="rotation batch 3"):
        one.upright_image(img, Gravity.from_rp(torch.zeros(3), torch.zeros(3)))
    cams[1, 0] = 31
    with pytest.raises(AssertionError, match="same size"):
        cam.reproject_image(torch.rand(3, 1, 20, 30))
    with pytest.raises(AssertionError, match="same size"):
        camera_models["radial"](cams[:1]).reproject_image(torch.rand(3, 1, 20, 30), target=cam)


# ------------------------------------------------------------------ code objects
@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="LLVM tools missing")
def test_reproject_kernels_carry_no_scratch_and_no_lds(tmp_path):
    from test_kernel_audit import kernel_metadata
    # the float instantiations of the one kernel template: element type `f`, planar (the byte ones: test_u8_image_abi.py)
    k = {n: v for n, v in kernel_metadata(tmp_path).items() if re.search(r"reproject_kernelILi\dELi\dELb\dEfLb0EEEv", n)}
    assert len(k) == 32, sorted(k)
    for s in range(4):
        for t in range(4):
            for r in range(2):
                assert any(f"reproject_kernelILi{s}ELi{t}ELb{r}EfLb0E" in n for n in k), (s, t, r, sorted(k))
    assert all(v["scratch"] == 0 and v["lds"] == 0 for v in k.values()), k
    assert all(v["vgpr"] <= 64 for v in k.values()), k
