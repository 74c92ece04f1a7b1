"""CPU: gclm_field_loss / gclm_field_loss_grad without a device -- the entry points are declared, exported and bound, every
invalid argument is refused before any HIP call, the workspace size is monotone, the float64 yardstick of
tests/field_loss_gate.py equals losses.perspective_field_loss on CPU float64 inputs and stands within float32 rounding of the
reference's recorded losses and gradients, losses.field_loss passes gradcheck, the gate passes an honest float32 restatement
of the kernels and fails its mutants, the Python wrappers hand the C entries the arguments of include/gclm.h, and both paths
return the reference's keys and raise the same errors."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from geocalib_amd import Gravity, _call, _lib, camera_models, fields, losses
from abi_harness import HEADER, LLVM, assert_declared_exported_and_bound
import field_error_gate as fg
import field_loss_gate as lg
import perspective_gate as pg
from test_host_calls import MAX, STREAM, p, rec  # noqa: F401  (the recorder fixture, not edited)

SHARED = ["int", "const float*", "const float*", "int", "int", "int", "const float*", "const float*", "const float*", "const float*",
          "int", "int"]
ARGS = SHARED + ["void*", "size_t", "float*", "void*"]
GRAD_ARGS = SHARED + ["const float*", "float*", "float*", "void*"]


def test_entry_points_are_declared_exported_and_bound():
    for name, args in (("gclm_field_loss", ARGS), ("gclm_field_loss_grad", GRAD_ARGS)):
        for a, t in zip(assert_declared_exported_and_bound(name, args), args):
            assert t in ("int", "size_t") or a is C.c_void_p, (name, a, t)
    assert assert_declared_exported_and_bound("gclm_field_loss_workspace", ["int"] * 3, ret="size_t") == [C.c_int] * 3
    header = open(HEADER).read()
    changelog = header[header.index("ABI version:"):header.index("#define GCLM_VERSION")]
    assert all(n in changelog for n in ("gclm_field_loss,", "gclm_field_loss_grad", "gclm_field_loss_workspace"))
    for name, i in lg.LOSS_IDS.items():          # the enum, the binding and the gate agree
        assert f"GCLM_FIELD_LOSS_{name.upper()} = {i}" in header and _lib.FIELD_LOSS_IDS[name] == i
    assert tuple(_lib.FIELD_LOSS_IDS) == losses.LOSS_TYPES


# fake, never dereferenced device addresses: every call below must be refused before the first HIP call
CAM, GRAV, UP, LAT, UPC, LATC = 0x100000, 0x200000, 0x4000000, 0x8000000, 0xC000000, 0x10000000
WS, OUT, SCALE, GUP, GLAT = 0x20000000, 0x30000000, 0x38000000, 0x40000000, 0x50000000
PX_BYTES = 2 * 48 * 64 * 4
OK = dict(model=1, cam=CAM, grav=GRAV, B=2, H=48, W=64, up=UP, lat=LAT, upc=UPC, latc=LATC, ul=0, ll=4, ws=WS, ws_bytes=1 << 24,
          out=OUT, scale=SCALE, gup=GUP, glat=GLAT)
BOTH = [("NULL camera", dict(cam=None)), ("NULL gravity", dict(grav=None)),
        ("both fields NULL", dict(up=None, lat=None, upc=None, latc=None, gup=None, glat=None)),
        ("up confidence without up", dict(up=None, gup=None)), ("latitude confidence without latitude", dict(lat=None, glat=None)),
        ("B = 0", dict(B=0)), ("B > 65535", dict(B=65536)), ("H = 0", dict(H=0)), ("W = 0", dict(W=0)),
        ("H * W > 2^31 - 1", dict(H=65536, W=32768, ws_bytes=1 << 62)), ("tile grid over 2^32 threads", dict(H=2 ** 31 - 1, W=1, ws_bytes=1 << 62)),
        ("model -1", dict(model=-1)), ("model 4", dict(model=4)), ("up loss -1", dict(ul=-1)), ("up loss 5", dict(ul=5)),
        ("latitude loss -1", dict(ll=-1)), ("latitude loss 5", dict(ll=5)), ("dot for latitude", dict(ll=2)),
        ("dot for an absent latitude", dict(ll=2, lat=None, latc=None, glat=None)),
        ("camera misaligned", dict(cam=CAM + 2)), ("gravity misaligned", dict(grav=GRAV + 1)), ("up misaligned", dict(up=UP + 1)),
        ("latitude misaligned", dict(lat=LAT + 2)), ("up confidence misaligned", dict(upc=UPC + 3)),
        ("latitude confidence misaligned", dict(latc=LATC + 2))]
FORWARD = [("NULL out", dict(out=None)), ("NULL workspace", dict(ws=None)), ("workspace too small", dict(ws_bytes=380)),
           ("out misaligned", dict(out=OUT + 2)), ("workspace misaligned", dict(ws=WS + 1)),
           ("out overlaps the camera", dict(out=CAM + 32)), ("out overlaps the gravity", dict(out=GRAV - 8)),
           ("out overlaps up", dict(out=UP + 2 * PX_BYTES - 4)), ("workspace overlaps the up confidence", dict(ws=UPC + PX_BYTES - 4)),
           ("workspace overlaps latitude", dict(ws=LAT - 4)), ("workspace overlaps out", dict(ws=OUT - 4))]
GRAD = [("NULL scale", dict(scale=None)), ("up gradient without up", dict(up=None, upc=None)),
        ("latitude gradient without latitude", dict(lat=None, latc=None)), ("up without its gradient", dict(gup=None)),
        ("latitude without its gradient", dict(glat=None)), ("scale misaligned", dict(scale=SCALE + 2)),
        ("up gradient misaligned", dict(gup=GUP + 1)), ("latitude gradient misaligned", dict(glat=GLAT + 2)),
        ("up gradient overlaps up", dict(gup=UP + 2 * PX_BYTES - 4)), ("up gradient is up", dict(gup=UP)),
        ("latitude gradient overlaps latitude", dict(glat=LAT)), ("up gradient overlaps the latitude confidence", dict(gup=LATC - 4)),
        ("latitude gradient overlaps the up confidence", dict(glat=UPC + PX_BYTES - 4)), ("up gradient overlaps the scale", dict(gup=SCALE - 2 * PX_BYTES + 4)),
        ("latitude gradient overlaps the scale", dict(glat=SCALE + 12)), ("latitude gradient overlaps the camera", dict(glat=CAM - PX_BYTES + 4)),
        ("latitude gradient overlaps the gravity", dict(glat=GRAV + 20)), ("the gradients overlap", dict(glat=GUP + 2 * PX_BYTES - 4))]


def _forward(a):
    return _lib.load().gclm_field_loss(a["model"], a["cam"], a["grav"], a["B"], a["H"], a["W"], a["up"], a["lat"], a["upc"], a["latc"],
                                       a["ul"], a["ll"], a["ws"], a["ws_bytes"], a["out"], None)


def _grad(a):
    return _lib.load().gclm_field_loss_grad(a["model"], a["cam"], a["grav"], a["B"], a["H"], a["W"], a["up"], a["lat"], a["upc"],
                                            a["latc"], a["ul"], a["ll"], a["scale"], a["gup"], a["glat"], None)


@pytest.mark.parametrize("what,change", BOTH + FORWARD, ids=[b[0] for b in BOTH + FORWARD])
def test_invalid_arguments_of_the_forward_are_refused_before_any_hip_call(what, change):
    assert _forward({**OK, **change}) == -3, what


@pytest.mark.parametrize("what,change", BOTH + GRAD, ids=[b[0] for b in BOTH + GRAD])
def test_invalid_arguments_of_the_gradient_are_refused_before_any_hip_call(what, change):
    assert _grad({**OK, **change}) == -3, what


def test_workspace_size_is_monotone_and_zero_for_invalid_sizes():
    ws = _lib.load().gclm_field_loss_workspace
    assert 0 < ws(2, 48, 64) <= OK["ws_bytes"]
    for grow in ((3, 48, 64), (2, 49, 64), (2, 48, 65)):
        assert ws(*grow) > ws(2, 48, 64), grow
    for B, H, W in ((1, 1, 1), (7, 479, 641), (1024, 480, 640)):
        assert ws(B, H, W) <= ws(B + 1, H, W) and ws(B, H, W) <= ws(B, H + 1, W) <= ws(B, H + 1, W + 1)
    assert ws(1024, 480, 640) < 32 << 20
    for bad in ((0, 48, 64), (65536, 48, 64), (2, 0, 64), (2, 48, 0), (2, 65536, 32768), (2, 2 ** 31 - 1, 1)):
        assert ws(*bad) == 0, bad


# ------------------------------------------------------------------ the yardstick
SMALL = [c for c in fg.CASES if not c[5] and c[1:4] == fg.SHAPES[0]]


def _calibration(case, dtype=torch.float64):
    T = lg.target(case)
    cam, grav = camera_models[case[0]](T["cams"].to(dtype)), Gravity(T["gravs"].to(dtype))
    grav._data = T["gravs"].to(dtype)             # as stored: the yardstick does not renormalise either
    return cam, grav


@pytest.mark.parametrize("case", SMALL, ids=lg.case_id)
def test_yardstick_equals_the_torch_path_in_float64(case):
    """Losses and gradients agree to 1e-9 relative (plus 1e-12); the up field of simple_divisional to 1e-5, since the torch
    path's s' cancels in float64 too where |k1 r2| is tiny (tests/test_perspective_abi.py)."""
    cam, grav = _calibration(case)
    tol = 1e-5 if case[0] == "simple_divisional" else 1e-9
    gout = lg.grad_output(case[1]).double()
    for types in lg.loss_types(case):
        for which in lg.SUBSETS:
            y = lg.yardstick(case, which, types)
            data = {k: v.double() for k, v in fg.subset(lg.target(case)["data"], which).items()}
            leaves = {k: data[k].requires_grad_(True) for k in data if k.endswith("field")}
            out = losses.perspective_field_loss({**data, **leaves}, cam, grav, types[0], types[1], True, *lg.WEIGHTS)
            total = 0
            for i, (name, k) in enumerate((("up", "up"), ("latitude", "lat"))):
                if f"{name}_field" not in data:
                    assert f"{name}_total" not in out
                    continue
                assert torch.allclose(out[f"{name}_total"], y["loss"][:, i], rtol=tol, atol=1e-12), (types, which, name)
                assert torch.equal(out[f"{name}_total"], out[f"{name}-{types[i]}-loss"])
                total = total + (gout[:, i] * out[f"{name}_total"]).sum()
            total.backward()
            for name, k in (("up", "up"), ("latitude", "lat")):
                if f"{name}_field" in data:
                    G = y[f"G_{k}"]
                    und = y[f"und_{k}"]           # (torch's sign at a residual of exactly 0 is 0 on both sides)
                    assert torch.allclose(leaves[f"{name}_field"].grad[~und], G[~und], rtol=tol, atol=1e-12 + tol * G.abs().max().item()), \
                        (types, which, name)


def test_yardstick_stands_within_float32_rounding_of_the_reference():
    """tests/golden/field_loss_reference.npz (make_golden_field_loss.py): the reference's float32 losses and autograd
    gradients on recorded inputs against the formulas of the gate in float64 on the same inputs.  Losses within
    16 U sum |l| w, gradients within 16 U |g| per pixel (U = 2^-24): the margin is float32 rounding, not the code under test.
    Measured on the recorded file: 3.34 U (losses), 6.27 U (gradients); printed."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "field_loss_reference.npz"))
    gout = torch.from_numpy(g["grad_output"]).double()
    worst_l = worst_g = 0.0
    n = 0
    for field, C_ in (("up", 2), ("latitude", 1)):
        pred, t, conf = (torch.from_numpy(g[f"{field}_{k}"]).double() for k in ("pred", "target", "conf"))
        assert pred.shape == (3, C_, 12, 20) and g[f"{field}_pred"].dtype == np.float32
        res = (pred - t).abs()
        assert res.min() >= 4e-5 and res.max() <= 0.31 and (res < lg.HUBER_DELTA).any() and (res > lg.HUBER_DELTA).any()
        for kind in lg.LOSS_IDS:
            if kind == "dot" and field != "up":
                continue
            l, d = lg.pixel_loss(kind, pred, t)
            for mode in ("conf_on", "conf_off", "noconf"):
                w = conf / conf.sum((1, 2), keepdim=True) if mode == "conf_on" else torch.full_like(conf, 1 / 240)
                want, bound = (l * w).sum((1, 2)), 16 * lg.U * (l.abs() * w).sum((1, 2))
                got = torch.from_numpy(g[f"{field}/{kind}/{mode}/loss"]).double()
                worst_l = max(worst_l, ((got - want).abs() / (bound / 16)).max().item())
                assert ((got - want).abs() <= bound).all(), (field, kind, mode)
                if mode == "conf_off":
                    assert bool(g[f"{field}/{kind}/conf_off/grad_equals_noconf"])
                    continue
                G = gout[:, None, None, None] * d * w[:, None]
                got = torch.from_numpy(g[f"{field}/{kind}/{mode}/grad"]).double()
                worst_g = max(worst_g, ((got - G).abs() / (lg.U * G.abs()).clamp(min=1e-300)).max().item())
                assert ((got - G).abs() <= 16 * lg.U * G.abs()).all(), (field, kind, mode)
                n += 1
    print(f"golden: worst loss ratio {worst_l:.2f} U, worst gradient ratio {worst_g:.2f} U over {n} gradient planes")
    assert n == 18


@pytest.mark.parametrize("kind", ["l2", "cauchy", "dot"])
def test_field_loss_passes_gradcheck(kind):
    g = torch.Generator().manual_seed(5)
    C_ = 2 if kind == "dot" else 1
    pred = (0.02 * torch.randn(1, C_, 4, 5, generator=g, dtype=torch.float64)).requires_grad_(True)
    t = (0.02 * torch.randn(1, C_, 4, 5, generator=g, dtype=torch.float64)).requires_grad_(True)
    conf = torch.rand(1, 4, 5, generator=g, dtype=torch.float64) + 0.1
    assert torch.autograd.gradcheck(lambda a, b: losses.field_loss(a, b, conf, kind), (pred, t))
    assert torch.autograd.gradcheck(lambda a: losses.field_loss(a, t.detach(), None, kind), (pred,))
    leaf = conf.clone().requires_grad_(True)      # the confidence is detached
    assert not losses.field_loss(pred.detach(), t.detach(), leaf, kind).requires_grad


# ------------------------------------------------------------------ the GPU test's gate, checked here
@pytest.mark.parametrize("case", lg.CASES, ids=lg.case_id)
def test_gate_passes_an_honest_float32_restatement(case):
    """... with room to spare, and the yardstick alone keeps the undecided l1 signs within 1 % of every image but the last
    (the exact-target image)."""
    for types in lg.loss_types(case):
        for which in lg.SUBSETS:
            y = lg.yardstick(case, which, types)
            v = lg.verdict(y, lg.restate(case, which, types))
            kappas = {k: round(x, 2) for k, x in y.items() if k.startswith("kappa")}
            print(f"{lg.case_id(case)} {types} {which}: honest float32 {v} {kappas}")
            assert lg.passes(v) and max(v["loss"], v["den"], v["g_up"], v["g_lat"]) <= 0.5, (types, which, v)
            for k in ("up", "lat"):
                if f"undecided_{k}" in y:
                    assert y[f"undecided_{k}"][:-1].max() <= 0.01, (types, which, k, y[f"undecided_{k}"])
                    if types[0 if k == "up" else 1] == "l1":
                        assert y[f"undecided_{k}"][-1] > 0.01          # the designated image does exercise the rule


_C = {(c[0], c[2], c[3], c[5]): c for c in lg.CASES if c[4] == "random"}
# (mutant, case, loss types, subset, what it must push past its gate)
MUTANTS = [("plainmean", _C["pinhole", 37, 53, False], ("l1", "l1"), "all", "loss"),
           ("plainmean", _C["radial", 30, 200, False], ("huber", "huber"), "lat", "loss"),
           ("grad_hw", _C["simple_radial", 37, 53, False], ("l2", "l2"), "all", "g_up"),
           ("grad_hw", _C["pinhole", 11, 70, False], ("l1", "l1"), "lat", "g_lat"),
           ("l1flip", _C["pinhole", 37, 53, False], ("l1", "l1"), "all", "g_up"),
           ("l1flip", _C["simple_divisional", 9, 132, True], ("l1", "l1"), "noconf", "g_lat"),
           ("huber1", _C["radial", 37, 53, False], ("huber", "huber"), "all", "loss"),
           ("huber1", _C["simple_radial", 30, 200, True], ("huber", "huber"), "noconf", "g_lat"),
           ("cauchy_nohalf", _C["pinhole", 37, 53, False], ("cauchy", "l1"), "all", "loss"),
           ("cauchy_nohalf", _C["simple_divisional", 37, 53, False], ("dot", "cauchy"), "lat", "loss"),
           ("dot_pt", _C["pinhole", 37, 53, False], ("dot", "cauchy"), "all", "loss"),
           ("dot_pt", _C["radial", 37, 53, False], ("dot", "cauchy"), "up", "loss"),
           ("unnorm", _C["simple_radial", 37, 53, False], ("l1", "l1"), "all", "loss"),
           ("unnorm", _C["simple_divisional", 37, 53, False], ("dot", "cauchy"), "up", "g_up"),
           ("scale0", _C["pinhole", 37, 53, False], ("l1", "l1"), "all", "g_up"),
           ("scale0", _C["radial", 30, 200, False], ("huber", "huber"), "noconf", "g_lat"),
           ("upscale_lat", _C["pinhole", 37, 53, False], ("l2", "l2"), "all", "g_lat"),
           ("upscale_lat", _C["simple_radial", 9, 132, False], ("l1", "l1"), "noconf", "g_lat"),
           ("lastcol", _C["pinhole", 9, 132, True], ("l1", "l1"), "all", "loss"),
           ("lastcol", _C["simple_divisional", 30, 200, True], ("huber", "huber"), "noconf", "g_up")]


@pytest.mark.parametrize("mutant,case,types,which,what", MUTANTS, ids=[f"{m}-{lg.case_id(c)}-{t[0]}-{t[1]}-{s}-{w}" for m, c, t, s, w in MUTANTS])
def test_gate_fails_each_mutant(mutant, case, types, which, what):
    assert types in lg.loss_types(case)          # a combination the GPU test runs
    v = lg.verdict(lg.yardstick(case, which, types), lg.restate(case, which, types, mutant=mutant))
    print(f"{mutant} on {lg.case_id(case)} {types} {which}: {v}")
    assert not lg.passes(v) and v[what] > 1, (mutant, v)


def test_every_loss_type_runs_on_every_model_and_the_cases_reach_every_path():
    for model in pg.MODELS:
        ups = {t[0] for c in lg.CASES if c[0] == model for t in lg.loss_types(c)}
        lats = {t[1] for c in lg.CASES if c[0] == model for t in lg.loss_types(c)}
        assert ups == set(lg.LOSS_IDS) and lats == set(lg.LOSS_IDS) - {"dot"}, model
        assert all(("l1", "l1") in lg.loss_types(c) and ("huber", "huber") in lg.loss_types(c) for c in lg.CASES)
        paths = {fg.pixels_per_lane(c[3], c[5]) for c in lg.CASES if c[0] == model}
        assert paths == {1, 2, 4}, model
    assert any(c[3] == 132 for c in lg.CASES) and any(c[2] % 4 for c in lg.CASES) and any(c[5] for c in lg.CASES)
    assert (lg.grad_output(3) == 0).any(0).all() and len(set(lg.GOUT_UP)) == 3


# ------------------------------------------------------------------ the call path (the recorder of test_host_calls.py)
def _inputs(B, H=2, W=2):
    g = torch.Generator().manual_seed(0)
    cam = torch.tensor([[float(W), float(H), 1.5, 1.5, W / 2, H / 2, 0.05, 0.0]]).repeat(B, 1)
    grav = torch.tensor([[0.0, 1.0, 0.0]]).repeat(B, 1)
    return cam, grav, torch.randn(B, 2, H, W, generator=g), torch.rand(B, 1, H, W, generator=g), torch.rand(B, H, W, generator=g), \
        torch.rand(B, H, W, generator=g)


def test_wrappers_hand_over_the_arguments_of_the_header(rec):  # noqa: F811
    cam, grav, up, lat, upc, latc = _inputs(2)
    out = fields.field_loss("radial", cam, grav, up, lat, upc, latc, "dot", "huber")
    assert out.shape == (2, 4)
    (n0, a0), (n1, a1) = rec.calls
    assert (n0, a0) == ("gclm_field_loss_workspace", (2, 2, 2)) and n1 == "gclm_field_loss"
    ws = a1[12]
    assert a1 == (2, p(cam), p(grav), 2, 2, 2, p(up), p(lat), p(upc), p(latc), 2, 4, ws, 0, p(out), STREAM)
    assert isinstance(ws, int) and ws != p(out) and not rec.entered
    del rec.calls[:]
    scale = torch.rand(2, 2)
    gu, gl = fields.field_loss_grad("radial", cam, grav, scale, up, lat, upc, latc, "cauchy", "l2")
    assert gu.shape == up.shape and gl.shape == lat.shape
    assert rec.calls == [("gclm_field_loss_grad", (2, p(cam), p(grav), 2, 2, 2, p(up), p(lat), p(upc), p(latc), 3, 1, p(scale), p(gu),
                                                   p(gl), STREAM))]


def test_wrappers_pass_null_for_absent_planes_and_refuse_what_the_entry_would(rec):  # noqa: F811
    cam, grav, up, lat, upc, latc = _inputs(2)
    out = fields.field_loss("pinhole", cam, grav, None, lat)
    assert rec.calls[1][1][6:12] == (None, p(lat), None, None, 0, 0)
    del rec.calls[:]
    gu, gl = fields.field_loss_grad("pinhole", cam, grav, torch.rand(2, 2), up, None, upc, None, "huber")
    a = rec.calls[0][1]
    assert gl is None and a[6:12] == (p(up), None, p(upc), None, 4, 0) and a[13:] == (p(gu), None, STREAM)
    for bad in (dict(), dict(lat=lat, up_conf=upc), dict(up=up, up_loss="l3"), dict(lat=lat, lat_loss="dot")):
        with pytest.raises(ValueError):
            fields.field_loss("pinhole", cam, grav, **bad)
    with pytest.raises(ValueError):
        fields.field_loss_grad("pinhole", cam, grav, torch.rand(3, 2), up, lat)


def test_wrappers_slice_and_advance_every_pointer(rec):  # noqa: F811
    B = MAX + 3
    cam, grav, up, lat, upc, latc = _inputs(B, 1, 1)
    out = fields.field_loss("pinhole", cam, grav, up, lat, upc, latc)
    (_, w), (_, first), (_, second) = rec.calls
    assert w == (MAX, 1, 1)                      # one workspace, sized for the largest call
    ws = first[12]
    assert first == (0, p(cam), p(grav), MAX, 1, 1, p(up), p(lat), p(upc), p(latc), 0, 0, ws, 0, p(out), STREAM)
    assert second == (0, p(cam) + MAX * 32, p(grav) + MAX * 12, 3, 1, 1, p(up) + MAX * 8, p(lat) + MAX * 4, p(upc) + MAX * 4,
                      p(latc) + MAX * 4, 0, 0, ws, 0, p(out) + MAX * 16, STREAM)
    del rec.calls[:]
    scale = torch.rand(B, 2)
    gu, gl = fields.field_loss_grad("pinhole", cam, grav, scale, up, lat, upc, latc)
    (_, first), (_, second) = rec.calls
    assert first[12:] == (p(scale), p(gu), p(gl), STREAM)
    assert second[:4] == (0, p(cam) + MAX * 32, p(grav) + MAX * 12, 3) and \
        second[12:] == (p(scale) + MAX * 8, p(gu) + MAX * 8, p(gl) + MAX * 4, STREAM)


# ------------------------------------------------------------------ the public functions
def test_keys_and_errors_of_the_public_functions():
    case = SMALL[0]
    cam, grav = _calibration(case, torch.float32)
    data = lg.target(case)["data"]
    out = losses.perspective_field_loss(data, cam, grav, "dot", "cauchy")
    assert sorted(out) == ["latitude-cauchy-loss", "latitude_total", "perspective_total", "up-dot-loss", "up_total"]
    assert all(v.shape == (case[1],) and v.dtype == torch.float32 for v in out.values())
    assert torch.allclose(out["perspective_total"], out["up_total"] + out["latitude_total"])
    only = losses.perspective_field_loss({"latitude_field": data["latitude_field"], "up_confidence": data["up_confidence"]}, cam, grav)
    assert sorted(only) == ["latitude-l1-loss", "latitude_total", "perspective_total"]
    four_d = {**data, "up_confidence": data["up_confidence"][:, None]}       # (B, 1, H, W) confidences are reshaped
    assert torch.equal(losses.perspective_field_loss(four_d, cam, grav)["up_total"], losses.perspective_field_loss(data, cam, grav)["up_total"])
    off = losses.perspective_field_loss(data, cam, grav, use_uncertainty_loss=False)
    noconf = losses.perspective_field_loss(fg.subset(data, "noconf"), cam, grav)
    assert torch.equal(off["perspective_total"], noconf["perspective_total"])
    half = losses.perspective_field_loss({k: v.half() for k, v in data.items()}, cam, grav)        # cast as the reference casts
    assert half["up_total"].dtype == torch.float32
    for bad in (dict(up_loss="l3"), dict(latitude_loss="dot"), dict(latitude_loss="classification")):
        with pytest.raises(ValueError):
            losses.perspective_field_loss(data, cam, grav, **bad)
    with pytest.raises(ValueError):
        losses.perspective_field_loss({}, cam, grav)
    with pytest.raises(ValueError):
        losses.field_loss(data["up_field"], data["up_field"], None, "l3")
    both, scores = losses.perspective_decoder_loss(data, cam, grav, (2, 4), up_loss="huber")
    assert "up-huber-loss" in both and sorted(scores) == sorted(
        f"{f}_angle_{k}" for f in ("up", "latitude") for k in ("error", "error_weighted", "recall@2", "recall@4"))
    assert _call.MAX_CALL == MAX


def test_the_hip_path_raises_the_same_errors_before_any_call(rec, monkeypatch):  # noqa: F811
    """With the device check stood in for (the recorder), float32 "device" tensors take the HIP path: it refuses the loss types
    the torch path refuses, and hands the entry the ids of the others."""
    case = SMALL[0]
    cam, grav = _calibration(case, torch.float32)
    data = lg.target(case)["data"]
    monkeypatch.setattr(losses, "_hip_path", lambda tensors, c, g: True)
    monkeypatch.setattr(losses, "_field_loss_torch", lambda *a: pytest.fail("torch path called"))
    for bad in (dict(up_loss="l3"), dict(latitude_loss="dot")):
        with pytest.raises(ValueError):
            losses.perspective_field_loss(data, cam, grav, **bad)
    assert not rec.calls
    out = losses.perspective_field_loss(data, cam, grav, "dot", "huber", use_uncertainty_loss=False)
    assert [n for n, _ in rec.calls] == ["gclm_field_loss_workspace", "gclm_field_loss"]
    assert rec.calls[1][1][8:12] == (None, None, 2, 4) and sorted(out) == ["latitude-huber-loss", "latitude_total", "perspective_total",
                                                                         "up-dot-loss", "up_total"]


# ------------------------------------------------------------------ code objects
@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="LLVM tools missing")
def test_field_loss_kernels_carry_no_scratch(tmp_path):
    from test_kernel_audit import kernel_metadata
    k = {n: v for n, v in kernel_metadata(tmp_path).items() if "field_loss" in n}
    for m in range(4):
        for px in (1, 2, 4):
            assert any(f"field_loss_kernelILi{m}ELi{px}E" in n for n in k), (m, px, sorted(k))
            assert any(f"field_loss_grad_kernelILi{m}ELi{px}E" in n for n in k), (m, px, sorted(k))
    assert any("field_loss_finish_kernel" in n for n in k) and len(k) == 25          # model x PX per kernel: no loss-type instantiations
    print({n: v for n, v in k.items()})
    assert all(v["scratch"] == 0 for v in k.values()), k
    assert all(v["vgpr"] <= 64 and v["lds"] <= 2048 for v in k.values()), k


# ------------------------------------------------------------------ the caller's memory
def _device_call(which, case, dev):
    cams, gravs, data = fg.make_case(case)
    cam, grav = cams.to(dev), gravs.to(dev)
    planes = [data[k].to(dev) for k in ("up_field", "latitude_field", "up_confidence", "latitude_confidence")]
    if which == "loss":
        return lambda: [fields.field_loss(case[0], cam, grav, *planes, "l1", "huber")]
    scale = torch.tensor([[0.25, -1.5]], device=dev).repeat(case[1], 1)
    return lambda: fields.field_loss_grad(case[0], cam, grav, scale, *planes, "l1", "huber")


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["loss", "grad"])
def test_results_do_not_depend_on_what_the_handed_memory_held(monkeypatch, which):
    """gclm_field_loss / gclm_field_loss_grad at 30 x 200 (tile columns and rows both ragged) with the wrapper's torch.empty
    memory -- the workspace of the loss; the gradient takes none: its two output planes -- holding 0x00 bytes, 0xFF bytes, and
    what a call at 3 x 37 x 53 left: the same bits."""
    from workspace_fill import same_bits_whatever_the_memory_held
    dev = torch.device("cuda:0")
    same_bits_whatever_the_memory_held(monkeypatch, dev, _device_call(which, ("simple_radial", 2, 30, 200, "random", False), dev),
                                       _device_call(which, ("simple_radial", 3, 37, 53, "random", False), dev))
