"""CPU: gclm_perspective_fields without a device -- the entry point is declared, exported and bound, every invalid argument
is refused before any HIP call, the float64 yardstick of tests/perspective_gate.py equals today's torch path in float64
and the reference's own float64 outputs, its simple_divisional closed forms equal float64 autograd of _distort_scale, the
gate passes an honest float32 evaluation and fails its mutants, and the kernels carry no scratch and no LDS."""
import ctypes as C
import os

import pytest
import torch

from geocalib_amd import Gravity, _lib, camera_models, perspective_fields as pf
from abi_harness import LLVM, assert_declared_exported_and_bound
import perspective_gate as pg

ARGS = ["int", "const float*", "const float*", "int", "int", "int", "int", "float*", "float*", "void*"]


def test_entry_point_is_declared_exported_and_bound():
    args = assert_declared_exported_and_bound("gclm_perspective_fields", ARGS)
    assert len(args) == 10
    assert [a for a in args if a is C.c_int] == [C.c_int] * 5 and args[0] is C.c_int
    assert args[1] is args[2] is args[7] is args[8] is args[9] is C.c_void_p


# fake, never dereferenced device addresses: every call below must be refused before the first HIP call
CAM, GRAV, UP, LAT = 0x100000, 0x200000, 0x4000000, 0x8000000
OK = dict(model=1, cam=CAM, grav=GRAV, B=2, H=48, W=64, norm=1, up=UP, lat=LAT)
UP_BYTES = 2 * 48 * 64 * 2 * 4
BAD = [("NULL camera", dict(cam=None)), ("NULL gravity", dict(grav=None)), ("both outputs NULL", dict(up=None, lat=None)),
       ("B = 0", dict(B=0)), ("B > 65535", dict(B=65536)), ("H = 0", dict(H=0)), ("W = 0", dict(W=0)),
       ("H * W > 2^31 - 1", dict(H=65536, W=32768)), ("model -1", dict(model=-1)), ("model 4", dict(model=4)),
       ("normalize 2", dict(norm=2)), ("normalize -1", dict(norm=-1)),
       ("latitude overlaps up", dict(lat=UP + UP_BYTES - 4)), ("up overlaps latitude", dict(up=LAT - 8)),
       ("up overlaps the camera", dict(up=CAM - 8)), ("latitude overlaps the gravity", dict(lat=GRAV + 20)),
       ("up overlaps the gravity", dict(up=GRAV)), ("latitude overlaps the camera", dict(lat=CAM + 60)),
       ("up not 8-byte aligned", dict(up=UP + 4)), ("latitude not 4-byte aligned", dict(lat=LAT + 2)),
       ("tile grid over 2^32 threads", dict(H=2 ** 31 - 1, W=1))]


@pytest.mark.parametrize("what,change", BAD, ids=[b[0] for b in BAD])
def test_invalid_arguments_are_refused_before_any_hip_call(what, change):
    a = {**OK, **change}
    rc = _lib.load().gclm_perspective_fields(a["model"], a["cam"], a["grav"], a["B"], a["H"], a["W"], a["norm"], a["up"],
                                             a["lat"], None)
    assert rc == -3, (what, rc)


# ------------------------------------------------------------------ the yardstick
def _torch64(model, cams, gravs, normalize=True):
    cam, grav = camera_models[model](cams.double()), Gravity(gravs.double())
    grav._data = gravs.double()                   # as stored: the yardstick does not renormalise either
    up = pf.get_up_field(cam, grav, normalize=normalize)
    return up, pf.get_latitude_field(cam, grav)[..., 0]


YARD = [("pinhole", None, 31, 40, "random"), ("simple_radial", None, 31, 40, "pitch+"), ("radial", None, 30, 41, "roll-"),
        ("simple_divisional", 0.8, 31, 40, "random"), ("simple_divisional", -2.0, 30, 41, "pitch-"),
        ("simple_divisional", 3.0, 31, 40, "roll+")]


@pytest.mark.parametrize("model,k1,H,W,kind", YARD)
@pytest.mark.parametrize("normalize", [True, False])
def test_yardstick_equals_the_torch_path_in_float64(model, k1, H, W, kind, normalize):
    """simple_divisional: the torch path's s' cancels in float64 too where |k1 r2| is tiny (near the principal point), so
    those pixels are left out there."""
    cams, gravs = pg.make_cameras(model, 3, H, W, k1, seed=3), pg.make_gravity(3, kind, seed=4)
    up, lat = _torch64(model, cams, gravs, normalize)
    ref = pg.fields(model, cams, gravs, H, W, clamp_hi=pg.LAT_HI64)
    q = ref["up"] if normalize else ref["q"]
    keep = torch.ones(3, H, W, dtype=torch.bool)
    if model == "simple_divisional":
        u = (torch.arange(W, dtype=torch.float64) - cams[:, 4, None, None].double()) / cams[:, 2, None, None].double()
        v = (torch.arange(H, dtype=torch.float64)[:, None] - cams[:, 5, None, None].double()) / cams[:, 3, None, None].double()
        keep = (cams[:, 6, None, None].double() * (u * u + v * v)).abs() >= 1e-3
    scale = max(1.0, q.abs().max().item())
    assert (up - q).abs()[keep].max().item() <= 1e-12 * scale, (up - q).abs()[keep].max()
    assert (lat - ref["lat"]).abs().max().item() <= 1e-12


@pytest.mark.parametrize("model", pg.MODELS)
def test_yardstick_matches_the_reference_float64_outputs(model):
    """tests/golden/golden_host_api.npz: the reference's get_perspective_field in float64 on its cameras (a 12 x 16 sample);
    the reference renormalises the gravity in float64 (Gravity()), so the yardstick is given that gravity here."""
    from test_host_api import host_api_golden
    g = host_api_golden()
    cams, gravs = g[f"api/{model}/camera"], g[f"api/{model}/gravity"]
    g64 = torch.nn.functional.normalize(gravs.double(), dim=-1)
    W, H = (int(v) for v in cams[0, :2].tolist())
    ref = pg.fields(model, cams, g64, H, W, clamp_hi=pg.LAT_HI64)
    rows, cols = torch.linspace(0, H - 1, 12).round().long(), torch.linspace(0, W - 1, 16).round().long()
    up = ref["up"].permute(0, 3, 1, 2)[..., rows, :][..., cols]
    lat = ref["lat"][:, None][..., rows, :][..., cols]
    assert torch.allclose(up, g[f"api/{model}/out64/up_field"], rtol=0, atol=1e-12)
    assert torch.allclose(lat, g[f"api/{model}/out64/latitude_field"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("k1", [3.0, 2.0, 0.8, -0.5, -2.0])
def test_divisional_closed_forms_equal_float64_autograd(k1):
    """s and s' of the yardstick (the kernel's forms) against float64 autograd of SimpleDivisional._distort_scale, across
    the singular circle 4 k1 r2 = 1 (tau >= 1e-6 for s'; beyond it the reference clamps and the yardstick copies it).  Where
    |k1 r2| < 1e-3 the reference's forms cancel in float64 as well, so those points are left out."""
    r2 = torch.linspace(1e-4, 0.5, 2001, dtype=torch.float64)
    cam = camera_models["simple_divisional"](torch.tensor([[40.0, 30.0, 30.0, 30.0, 20.0, 15.0, k1, 0.0]], dtype=torch.float64))
    x = r2.clone().requires_grad_(True)
    s_ref = cam._distort_scale(x[None, :, None])
    (ds_ref,) = torch.autograd.grad(s_ref.sum(), x)
    k = torch.tensor(k1, dtype=torch.float64)
    s, sp, _ = pg.scales("simple_divisional", k, k * 0, r2)
    tau = 1 - 4 * k1 * r2
    big = (k1 * r2).abs() >= 1e-3
    inside = (tau >= 1e-6) & big
    assert torch.allclose(s[big], s_ref.detach().reshape(-1)[big], rtol=1e-10, atol=0)
    assert inside.any() and torch.allclose(sp[inside], ds_ref[inside], rtol=1e-7, atol=0)
    assert torch.allclose(sp[big], cam._distort_scale_dr2(r2[None, :, None]).reshape(-1)[big], rtol=1e-7, atol=0)


# ------------------------------------------------------------------ the GPU test's gate, checked here
def _gate(case):
    model, k1, k2, B, H, W, kind, normalize = case
    B = min(B, 3)
    cams, gravs = pg.make_cameras(model, B, H, W, k1, k2, 0), pg.make_gravity(B, kind, 0)
    ref = pg.fields(model, cams, gravs, H, W)
    kq, ks = pg.kappas(model, cams, gravs, H, W, ref=ref)
    return model, cams, gravs, H, W, normalize, ref, pg.gates(ref, kq, ks)


def _ratios(out, ref, bounds, normalize):
    b_up, b_q, b_lat = bounds
    up = pg.worst_ratio(out["up"], ref["up"], b_up) if normalize else pg.worst_ratio(out["q"], ref["q"], b_q)
    return up, pg.worst_ratio(out["lat"], ref["lat"], b_lat)


SELF = [c for c in pg.CASES if c[3] <= 7]


@pytest.mark.parametrize("case", SELF, ids=[f"{c[0]}-{c[1]}-{c[4]}x{c[5]}-{c[6]}-{c[7]}" for c in SELF])
def test_gate_passes_an_honest_float32_evaluation(case):
    model, cams, gravs, H, W, normalize, ref, bounds = _gate(case)
    out = pg.fields(model, cams, gravs, H, W, torch.float32)
    r_up, r_lat = _ratios(out, ref, bounds, normalize)
    print(f"{case}: honest float32 worst ratios up {r_up:.3f} lat {r_lat:.3f}")
    assert r_up <= 0.5 and r_lat <= 0.5, (r_up, r_lat)


def _vanishing_gravity(model, cams, H, W):
    """Gravities along the float64 viewing ray of one pixel per camera: sin(latitude) = 1 there, the clamp acts."""
    ref = pg.fields(model, cams, torch.tensor([[0.0, 0.0, 1.0]]).expand(cams.shape[0], 3), H, W)
    c = cams.double()
    y, x = H // 3, W // 3
    u, v = (x - c[:, 4]) / c[:, 2], (y - c[:, 5]) / c[:, 3]
    _, _, t = pg.scales(model, c[:, 6], c[:, 7], u * u + v * v)
    ray = torch.stack([u * t, v * t, torch.ones_like(u)], -1)
    assert ref["lat"].shape[1:] == (H, W)
    return torch.nn.functional.normalize(ray, dim=-1).float()


# (mutant, case, which field) -- each mutant must push its field past the gate
_C = {(c[0], c[1], c[6], c[7]): c for c in pg.CASES}
MUTANTS = [("offset", _C[("simple_radial", None, "random", True)], "up"),
           ("offset", _C[("radial", 0.7, "pitch-", True)], "up"),
           ("swap", _C[("simple_radial", None, "random", True)], "lat"),
           ("swap", _C[("simple_divisional", None, "random", True)], "lat"),
           ("noclamp", _C[("pinhole", None, "random", True)], "lat"),
           ("noclamp", _C[("radial", None, "random", True)], "lat"),
           ("halfpx", _C[("pinhole", None, "random", True)], "up"),
           ("halfpx", _C[("simple_divisional", 3.0, "random", True)], "lat"),
           ("fxfy", _C[("radial", None, "random", True)], "up"),
           ("fxfy", _C[("pinhole", None, "pitch-", False)], "lat"),
           ("renorm", _C[("pinhole", None, "pitch-", False)], "up"),
           ("renorm", _C[("simple_radial", None, "random", True)], "lat"),
           ("cancelling", _C[("simple_divisional", 1e-4, "random", True)], "up"),
           ("cancelling", _C[("simple_divisional", -1e-6, "pitch-", False)], "up")]


@pytest.mark.parametrize("mutant,case,field", MUTANTS, ids=[f"{m}-{c[0]}-{c[1]}-{c[6]}-{f}" for m, c, f in MUTANTS])
def test_gate_fails_each_mutant(mutant, case, field):
    model, cams, gravs, H, W, normalize, ref, bounds = _gate(case)
    if mutant == "noclamp":          # a pixel that looks straight along gravity
        gravs = _vanishing_gravity(model, cams, H, W)
        ref = pg.fields(model, cams, gravs, H, W)
        bounds = pg.gates(ref, *pg.kappas(model, cams, gravs, H, W, ref=ref))
    if mutant == "renorm":           # a stored gravity that is not a unit vector
        gravs = gravs * 1.001
        ref = pg.fields(model, cams, gravs, H, W)
        bounds = pg.gates(ref, *pg.kappas(model, cams, gravs, H, W, ref=ref))
    dtype = torch.float32 if mutant == "cancelling" else torch.float64
    out = pg.fields(model, cams, gravs, H, W, dtype, mutant=mutant)
    r_up, r_lat = _ratios(out, ref, bounds, normalize)
    ratio = r_up if field == "up" else r_lat
    print(f"{mutant} on {case[:3]} {case[6]}: worst ratio {ratio:.3g}")
    assert ratio > 1, (mutant, ratio)


# ------------------------------------------------------------------ code objects
@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="LLVM tools missing")
def test_perspective_kernels_carry_no_scratch_and_no_lds(tmp_path):
    from test_kernel_audit import kernel_metadata
    k = {n: v for n, v in kernel_metadata(tmp_path).items() if "perspective_field_kernel" in n}
    for m in range(4):
        assert any(f"perspective_field_kernelILi{m}E" in n for n in k), (m, sorted(k))
    print({n: v["vgpr"] for n, v in k.items()})
    assert all(v["scratch"] == 0 and v["lds"] == 0 for v in k.values()), k
    assert all(v["vgpr"] <= 32 for v in k.values()), k
