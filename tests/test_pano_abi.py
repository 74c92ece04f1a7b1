"""CPU: Camera.get_img_from_pano and gclm_render_from_pano without a device -- the entry point is declared, exported and
bound, every invalid argument is refused before any HIP call, the torch path equals the reference's get_img_from_pano bit
for bit, the parity gate of tests/test_pano_image.py passes an honest float32 evaluation and fails its mutants, and the
kernels carry no scratch and no LDS."""
import ctypes as C
import math
import os

import pytest
import torch

from geocalib_amd import _lib, camera_models
from geocalib_amd.gravity import Gravity
from abi_harness import LLVM, assert_declared_exported_and_bound
import pano_gate as pg
import undistort_gate as ug

ARGS = ["int", "const float*", "int", "const float*", "const float* const*", "const int*", "int", "int", "int", "int",
        "float*", "void*"]


def test_entry_point_is_declared_exported_and_bound():
    args = assert_declared_exported_and_bound("gclm_render_from_pano", ARGS)
    assert len(args) == 12
    assert [args[i] for i in (0, 2, 6, 7, 8, 9)] == [C.c_int] * 6
    assert args[1] is args[3] is args[10] is args[11] is C.c_void_p
    assert args[4] is C.POINTER(C.c_void_p) and args[5] is C.POINTER(C.c_int)


# fake, never dereferenced device addresses: every call below must be refused before the first HIP call
CAM, ROT, SRC, DST = 0x100000, 0x180000, 0x200000, 0x40000000
OK = dict(model=1, cam=CAM, nb=1, rot=ROT, srcs=[SRC, SRC], hw=[64, 128, 64, 128], n=2, C=3, H=48, W=64, dst=DST)
BAD = [("NULL camera", dict(cam=None)), ("NULL rotations", dict(rot=None)), ("NULL source table", dict(srcs=None)),
       ("NULL size table", dict(hw=None)), ("NULL destination", dict(dst=None)), ("NULL source", dict(srcs=[SRC, None])),
       ("n = 0", dict(n=0)), ("n > 65535", dict(n=65536)), ("C = 0", dict(C=0)), ("H = 1", dict(H=1)), ("W = 1", dict(W=1)),
       ("H * W > 2^31 - 1", dict(H=65536, W=32768)), ("Hs = 1", dict(hw=[64, 128, 1, 128])),
       ("Ws = 1", dict(hw=[64, 1, 64, 128])), ("Ws = 0", dict(hw=[64, 128, 64, 0])), ("cam_batch 0", dict(nb=0)),
       ("cam_batch 3 of n = 2", dict(nb=3)), ("model -1", dict(model=-1)), ("model 4", dict(model=4)),
       ("destination overlaps a source", dict(dst=SRC + 4096)),
       ("second source starts inside the destination", dict(srcs=[SRC, DST + 4 * 2 * 3 * 48 * 64 - 4])),
       ("destination overlaps the rotations", dict(dst=ROT - 64)), ("same buffer", dict(dst=SRC))]


@pytest.mark.parametrize("what,change", BAD, ids=[b[0] for b in BAD])
def test_invalid_arguments_are_refused_before_any_hip_call(what, change):
    a = {**OK, **change}
    srcs = None if a["srcs"] is None else (C.c_void_p * len(a["srcs"]))(*a["srcs"])
    hw = None if a["hw"] is None else (C.c_int * len(a["hw"]))(*a["hw"])
    n = a["n"]
    if srcs is not None and n > len(a["srcs"]):          # tables as long as n claims
        srcs, hw = (C.c_void_p * n)(*([SRC] * n)), (C.c_int * (2 * n))(*([64, 128] * n))
    rc = _lib.load().gclm_render_from_pano(a["model"], a["cam"], a["nb"], a["rot"], srcs, hw, n, a["C"], a["H"], a["W"],
                                           a["dst"], None)
    assert rc == -3, (what, rc)


# ------------------------------------------------------------------ the torch path against the reference
def _inputs(model, n, seed):
    g = torch.Generator().manual_seed(seed)
    W, H = 48, 36
    f = 20 + 30 * torch.rand(n, generator=g)
    lo, hi = ug.DIST_RANGE[model]
    k1 = lo + (hi - lo) * torch.rand(n, generator=g)
    k2 = (lo + (hi - lo) * torch.rand(n, generator=g)) * (model == "radial")
    data = torch.stack([torch.full((n,), float(W)), torch.full((n,), float(H)), f, f * 1.03, W / 2 + torch.rand(n, generator=g),
                        H / 2 - torch.rand(n, generator=g), k1 * (model != "pinhole"), k2], -1)
    rp = torch.rand(n, 2, generator=g) - 0.5
    yaws = 6 * torch.rand(n, generator=g) - 3
    return data, rp, yaws


# resize factors that give scale >= 1 (bicubic) and < 1 (area) within one call
RESIZE = torch.tensor([0.4, 1.7, 0.9, 2.5])


@pytest.mark.parametrize("model", pg.MODELS)
@pytest.mark.parametrize("resize", [False, True], ids=["plain", "resize"])
@pytest.mark.parametrize("form", ["n_cams_n_yaws", "1_cam_n_yaws", "n_cams_1_yaw"])
def test_torch_path_equals_the_reference_bit_for_bit(model, resize, form):
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip("reference checkout not available")
    ref = ref_import.load()
    n = 4
    data, rp, yaws = _inputs(model, n, seed=7)
    pano = ug.make_images("noise", 1, 3, 64, 128, seed=8)[0]
    d = data[:1] if form == "1_cam_n_yaws" else data
    y = yaws[:1] if form == "n_cams_1_yaw" else yaws
    rf = (RESIZE[:1] if form == "n_cams_1_yaw" else RESIZE) if resize else None
    # the reference indexes vfov[i] per yaw, so it can only render one camera over n yaws with resize_factor if the
    # camera is repeated; the rendering is the same
    d_ref = data[:1].expand(n, -1) if (form == "1_cam_n_yaws" and resize) else d
    ours = camera_models[model](d).get_img_from_pano(pano, Gravity.from_rp(rp[:, 0], rp[:, 1]), y, rf)
    theirs = ref.camera.camera_models[model](d_ref).get_img_from_pano(
        pano, ref.gravity.Gravity.from_rp(rp[:, 0], rp[:, 1]), y, rf)
    assert ours.shape == theirs.shape == ((1 if form == "n_cams_1_yaw" else n), 3, 36, 48)
    assert torch.equal(ours, theirs), (ours - theirs).abs().max()


def test_scalar_yaw_and_one_camera_render_one_image():
    data, rp, _ = _inputs("simple_radial", 1, seed=9)
    out = camera_models["simple_radial"](data).get_img_from_pano(torch.rand(3, 32, 64), Gravity.from_rp(rp[:, 0], rp[:, 1]),
                                                                 0.5, 1.0)
    assert out.shape == (1, 3, 36, 48)


def test_batches_that_do_not_broadcast_are_refused():
    data, rp, yaws = _inputs("radial", 3, seed=10)
    g = Gravity.from_rp(rp[:, 0], rp[:, 1])
    with pytest.raises(ValueError):
        camera_models["radial"](data).get_img_from_pano(torch.rand(3, 32, 64), g, yaws[:2])
    with pytest.raises(ValueError):
        camera_models["radial"](data[:2]).get_img_from_pano(torch.rand(3, 32, 64), g, yaws)
    with pytest.raises(ValueError):
        camera_models["radial"](data).get_img_from_pano(torch.rand(2, 3, 32, 64), g, yaws)


def test_one_panorama_per_image_equals_separate_calls():
    data, rp, yaws = _inputs("simple_divisional", 3, seed=11)
    panos = ug.make_images("noise", 3, 3, 40, 80, seed=12)
    cam, g = camera_models["simple_divisional"](data), Gravity.from_rp(rp[:, 0], rp[:, 1])
    for rf in (None, torch.tensor([0.5, 1.2, 2.0])):
        out = cam.get_img_from_pano(panos, g, yaws, rf)
        for i in range(3):
            one = cam[i:i + 1].get_img_from_pano(panos[i], g[i:i + 1], yaws[i:i + 1], None if rf is None else rf[i:i + 1])
            assert torch.equal(out[i:i + 1], one), i


# ------------------------------------------------------------------ the GPU test's gate, checked here
SELF_CHECK = [c for c in pg.CASES if c[2] <= 8]


def _ids(cases):
    return [f"{c[0]}-{c[1]}-n{c[2]}-C{c[4]}-{c[7]}x{c[8]}-p{c[11]}-y{c[12]}" for c in cases]


@pytest.mark.parametrize("case", SELF_CHECK, ids=_ids(SELF_CHECK))
def test_gate_passes_an_honest_float32_evaluation(case):
    model, H, W, Hs, Ws = case[0], case[5], case[6], case[7], case[8]
    cams, rot, pano = pg.case_inputs(case)[:3]
    ys = pg.Yardstick(model, cams, rot, H, W, pano.double())
    jx, jy, _, _ = pg.coordinates(model, cams, rot, H, W, Hs, Ws, torch.float32)
    ratio = ys.worst_ratio(pg.bilinear32(pano, jx, jy))
    print(f"{case[:2]} kappa {ys.kappa:.2f}, honest float32 worst ratio {ratio:.3f}")
    assert ratio <= 0.5, ratio


def _mutant_ratio(case, mutant):
    model, H, W, Hs, Ws = case[0], case[5], case[6], case[7], case[8]
    cams, rot, pano, yaws, rolls, pitches = pg.case_inputs(case)
    ys = pg.Yardstick(model, cams, rot, H, W, pano.double())
    src = pano.double()
    if mutant == "yaw_sign":
        out = pg.grid_sample64(src, *pg.coordinates(model, cams, pg.rotations(rolls, pitches, -yaws), H, W, Hs, Ws)[:2])
    elif mutant == "wrap":
        out = pg.wrap_sample(src, *pg.coordinates(model, cams, rot, H, W, Hs, Ws, mutant="wrap")[:2])
    else:
        out = pg.grid_sample64(src, *pg.coordinates(model, cams, rot, H, W, Hs, Ws, mutant=mutant)[:2])
    return ys.worst_ratio(out)


MUTANTS = [("atan2_swap", pg.CASES[0]), ("atan2_swap", pg.CASES[6]), ("yaw_sign", pg.CASES[1]), ("yaw_sign", pg.CASES[7]),
           ("distort", pg.CASES[2]), ("distort", pg.CASES[3]), ("Ws", pg.CASES[0]), ("Ws", pg.CASES[5]),
           ("half_pixel", pg.CASES[8]), ("half_pixel", pg.CASES[3]), ("wrap", pg.CASES[4]), ("wrap", pg.CASES[6])]


@pytest.mark.parametrize("mutant,case", MUTANTS, ids=[f"{m}-{c[0]}-{c[1]}-y{c[12]}" for m, c in MUTANTS])
def test_gate_fails_each_mutant(mutant, case):
    ratio = _mutant_ratio(case, mutant)
    print(f"{mutant} on {case[:2]}: worst ratio {ratio:.3g}")
    assert ratio > 1, (mutant, ratio)


def test_seam_pixels_accept_either_branch():
    """yaw = pi puts the seam in view: a pixel exactly on it may land at column 0 or Ws - 1."""
    case = pg.CASES[4]
    model, H, W, Hs, Ws = case[0], case[5], case[6], case[7], case[8]
    cams, _, pano = pg.case_inputs(case)[:3]
    cams = cams.clone()
    cams[:, 4] = (W - 1) / 2                           # an exactly representable centre column on the seam
    rot = pg.rotations([0.0], [0.0], [math.pi])
    ys = pg.Yardstick(model, cams, rot, H, W, pano.double())
    assert ys.seam.any()
    jx, jy, _, _ = pg.coordinates(model, cams, rot, H, W, Hs, Ws, torch.float32)
    flipped = torch.where(ys.seam, torch.where(jx > Ws / 2, jx - (Ws - 1), jx + (Ws - 1)), jx)
    assert ys.worst_ratio(pg.bilinear32(pano, flipped, jy)) <= 0.5
    assert math.isfinite(ys.kappa)


# ------------------------------------------------------------------ code objects
@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="LLVM tools missing")
def test_pano_kernels_carry_no_scratch_and_no_lds(tmp_path):
    from test_kernel_audit import kernel_metadata
    k = {n: v for n, v in kernel_metadata(tmp_path).items() if "render_from_pano_kernel" in n}
    assert len(k) >= 4, sorted(k)
    for m in range(4):
        assert any(f"render_from_pano_kernelILi{m}E" in n for n in k), (m, sorted(k))
    assert all(v["scratch"] == 0 and v["lds"] == 0 for v in k.values()), k
    assert all(v["vgpr"] <= 64 for v in k.values()), k
