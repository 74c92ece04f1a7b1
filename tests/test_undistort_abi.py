"""CPU: Camera.undistort_image and gclm_undistort_image without a device -- the entry point is declared, exported and bound,
every invalid argument is refused before any HIP call, the torch path of every model equals a float64 restatement of the
reference composition, the parity gate of tests/test_undistort_image.py passes an honest float32 evaluation and fails
its mutants, and the kernels carry no scratch and no LDS."""
import ctypes as C
import os
import re
import shutil

import pytest
import torch

from geocalib_amd import _lib, camera_models
from abi_harness import LLVM, assert_declared_exported_and_bound
import undistort_gate as ug

ARGS = ["int", "const float*", "int", "const float*", "int", "int", "int", "int", "int", "int", "float*", "void*"]


def test_entry_point_is_declared_exported_and_bound():
    args = assert_declared_exported_and_bound("gclm_undistort_image", ARGS)
    assert len(args) == 12
    assert [a for a in args if a is C.c_int] == [C.c_int] * 8 and args[1] is args[3] is args[10] is args[11] is C.c_void_p


# fake, never dereferenced device addresses: every call below must be refused before the first HIP call
CAM, SRC, DST = 0x100000, 0x200000, 0x4000000
OK = dict(model=1, cam=CAM, nb=1, src=SRC, B=2, C=3, Hin=48, Win=64, H=48, W=64, dst=DST)
BAD = [("NULL camera", dict(cam=None)), ("NULL source", dict(src=None)), ("NULL destination", dict(dst=None)),
       ("B = 0", dict(B=0)), ("C = 0", dict(C=0)), ("Hin = 0", dict(Hin=0)), ("Win = 0", dict(Win=0)),
       ("H = 1", dict(H=1)), ("W = 1", dict(W=1)), ("H = 0", dict(H=0)), ("cam_batch 0", dict(nb=0)),
       ("cam_batch 3 of B = 2", dict(nb=3)), ("model -1", dict(model=-1)), ("model 4", dict(model=4)),
       ("B > 65535", dict(B=65536, nb=1)), ("H * W > 2^31 - 1", dict(H=65536, W=32768)),
       ("destination overlaps the source", dict(dst=SRC + 4096)),
       ("source starts inside the destination", dict(src=DST + 4 * 2 * 3 * 48 * 64 - 4)),
       ("same buffer", dict(dst=SRC))]


@pytest.mark.parametrize("what,change", BAD, ids=[b[0] for b in BAD])
def test_invalid_arguments_are_refused_before_any_hip_call(what, change):
    a = {**OK, **change}
    rc = _lib.load().gclm_undistort_image(a["model"], a["cam"], a["nb"], a["src"], a["B"], a["C"], a["Hin"], a["Win"], a["H"],
                                          a["W"], a["dst"], None)
    assert rc == -3, (what, rc)


@pytest.mark.parametrize("model", ug.MODELS)
def test_undistort_image_exists_on_every_model(model):
    cls = camera_models[model]
    assert callable(getattr(cls, "undistort_image", None))
    cam = cls(ug.make_cameras(model, 1, 24, 32, seed=1))
    out = cam.undistort_image(torch.rand(2, 3, 24, 32))
    assert out.shape == (2, 3, 24, 32) and out.dtype == torch.float32


CPU_CASES = [("pinhole", 1, 3, 30, 41, 30, 41), ("simple_radial", 1, 3, 30, 41, 30, 41), ("radial", 3, 3, 30, 41, 36, 50),
             ("simple_divisional", 3, 3, 30, 41, 25, 33), ("simple_divisional", 1, 3, 31, 40, 31, 40),
             ("radial", 1, 3, 31, 40, 45, 29)]


@pytest.mark.parametrize("model,nb,B,H,W,Hin,Win", CPU_CASES)
@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_torch_path_equals_float64_reference_composition(model, nb, B, H, W, Hin, Win, kind):
    """Camera batch 1 broadcast over B = 3 and camera batch 3, Hin != H.  The float64 restatement runs the reference's own
    formula (simple_divisional: its cancelling form), so the torch path differs by float32 rounding only."""
    cams = ug.make_cameras(model, nb, H, W, seed=3)
    if model == "simple_divisional":
        cams[:, 6] = torch.tensor([0.8, -2.0, 2.9])[:nb]        # |k r2| not tiny: the cancelling form keeps its digits
    img = ug.make_images(kind, B, 2, Hin, Win, seed=4)
    out = camera_models[model](cams).undistort_image(img)
    ix, iy = ug.coordinates(model, cams, H, W, Hin, Win, cancelling=True)
    ref = ug.grid_sample64(img.double(), ix, iy)
    assert out.shape == ref.shape == (B, 2, H, W)
    assert torch.allclose(out.double(), ref, rtol=0, atol=2e-3 if kind == "noise" else 1e-4), (out.double() - ref).abs().max()


def test_camera_batch_must_match_and_share_one_size():
    cams = ug.make_cameras("radial", 3, 20, 30, seed=5)
    with pytest.raises(AssertionError):
        camera_models["radial"](cams).undistort_image(torch.rand(2, 1, 20, 30))
    cams[1, 0] = 31
    with pytest.raises(AssertionError):
        camera_models["radial"](cams).undistort_image(torch.rand(3, 1, 20, 30))


# ------------------------------------------------------------------ the GPU test's gate, checked here
def _case_parts(case):
    model, k1, k2, B, nb, C, H, W, Hin, Win, kind = case
    cams, img = ug.case_inputs(case)
    delta = ug.coordinate_bound(model, cams, H, W, Hin, Win)
    ix, iy = ug.coordinates(model, cams, H, W, Hin, Win)
    src64 = img.double()
    return model, cams, img, src64, delta, ix, iy, ug.grid_sample64(src64, ix, iy), ug.gate(src64, ix, iy, delta)


SELF_CHECK = [c for c in ug.CASES if c[3] <= 7]


@pytest.mark.parametrize("case", SELF_CHECK, ids=[f"{c[0]}-{c[1]}-{c[-1]}-{c[8]}x{c[9]}" for c in SELF_CHECK])
def test_gate_passes_an_honest_float32_evaluation(case):
    model, cams, img, src64, delta, ix, iy, ref, bound = _case_parts(case)
    H, W, Hin, Win = case[6], case[7], case[8], case[9]
    jx, jy = ug.coordinates(model, cams, H, W, Hin, Win, torch.float32)
    ratio = ug.worst_ratio(ug.bilinear32(img, jx, jy), ref, bound)
    print(f"{case[:2]} delta {delta:.2e} px, honest float32 worst ratio {ratio:.3f}")
    assert ratio <= 0.5, ratio


def _mutant_ratio(case, mutant):
    model, cams, img, src64, delta, ix, iy, ref, bound = _case_parts(case)
    H, W, Hin, Win = case[6], case[7], case[8], case[9]
    if mutant == "shift":
        out = ug.grid_sample64(src64, ix + 0.05, iy)
    elif mutant == "k1":
        c2 = cams.clone()
        c2[:, 6] *= 1 + 1e-3
        out = ug.grid_sample64(src64, *ug.coordinates(model, c2, H, W, Hin, Win))
    elif mutant == "align_corners":
        out = ug.grid_sample64(src64, ix, iy, align_corners=False)
    elif mutant == "border":
        out = ug.grid_sample64(src64, ix, iy, padding_mode="border")
    else:
        jx, jy = ug.coordinates(model, cams, H, W, Hin, Win, torch.float32, cancelling=True)
        out = ug.bilinear32(img, jx, jy)
    return ug.worst_ratio(out, ref, bound)


_C = {c[:2]: c for c in ug.CASES}
MUTANTS = [("shift", _C[("radial", None)]), ("shift", _C[("pinhole", None)]), ("k1", _C[("simple_radial", None)]),
           ("k1", _C[("radial", -0.7)]), ("align_corners", _C[("simple_divisional", None)]),
           ("align_corners", _C[("pinhole", None)]), ("border", _C[("simple_radial", 0.7)]),
           ("border", _C[("simple_divisional", 3.0)]), ("cancelling", _C[("simple_divisional", 1e-4)]),
           ("cancelling", _C[("simple_divisional", -1e-6)])]


@pytest.mark.parametrize("mutant,case", MUTANTS, ids=[f"{m}-{c[0]}-{c[1]}" for m, c in MUTANTS])
def test_gate_fails_each_mutant(mutant, case):
    ratio = _mutant_ratio(case, mutant)
    print(f"{mutant} on {case[:2]}: worst ratio {ratio:.3g}")
    assert ratio > 1, (mutant, ratio)


# ------------------------------------------------------------------ code objects
@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="LLVM tools missing")
def test_undistort_kernels_carry_no_scratch_and_no_lds(tmp_path):
    from test_kernel_audit import kernel_metadata
    # the float instantiations of the one kernel template: element type `f`, planar (the byte ones: test_u8_image_abi.py)
    k = {n: v for n, v in kernel_metadata(tmp_path).items() if re.search(r"undistort_image_kernelILi\dEfLb0EEEv", n)}
    assert len(k) == 4, sorted(k)
    for m in range(4):
        assert any(f"undistort_image_kernelILi{m}EfLb0E" in n for n in k), (m, sorted(k))
    assert all(v["scratch"] == 0 and v["lds"] == 0 for v in k.values()), k
    assert all(v["vgpr"] <= 64 for v in k.values()), k
