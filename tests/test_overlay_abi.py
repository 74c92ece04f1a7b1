"""CPU: the field overlay without a device -- gclm_draw_fields and gclm_draw_fields_u8 are declared, exported, bound and
documented; every invalid argument is refused before any HIP call, overlaps to the byte, and the legal neighbours reach the
launch; the gate of tests/test_overlay.py (tests/overlay_gate.py) keeps its conditions on every case, passes the CPU torch path
and fails its mutants; viz.draw_perspective_fields on CPU tensors returns the input's dtype and memory format, exact copies with
the layers off or a NaN calibration; the built-in palette is matplotlib's; and the 12 kernels exist without scratch and with at
most 2 KB of LDS."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT
from geocalib_amd import Gravity, _lib, camera_models, viz
from abi_harness import LLVM, assert_declared_exported_and_bound
import overlay_gate as og

F_ARGS = ["int", "const float*", "const float*", "int", "const float*", "int", "int", "int", "int", "const float*",
          "const unsigned char*", "const unsigned char*", "const gclm_overlay_style*", "float*", "void*"]
U_ARGS = ["int", "const float*", "const float*", "int", "const unsigned char*", "int", "int", "int", "int", "int", "const float*",
          "const unsigned char*", "const unsigned char*", "const gclm_overlay_style*", "unsigned char*", "void*"]


def test_entry_points_are_declared_exported_bound_and_documented():
    args = assert_declared_exported_and_bound("gclm_draw_fields", F_ARGS)
    assert len(args) == 15 and [a for a in args if a is C.c_int] == [C.c_int] * 6
    args = assert_declared_exported_and_bound("gclm_draw_fields_u8", U_ARGS)
    assert len(args) == 16 and [a for a in args if a is C.c_int] == [C.c_int] * 7
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "| `gclm_draw_fields` |" in doc and "| `gclm_draw_fields_u8` |" in doc
    header = open(os.path.join(ROOT, "include", "gclm.h")).read()
    assert "gclm_draw_fields and gclm_draw_fields_u8 added, also within 610" in header
    # the binding's struct is the header's: the same fields in the same order, 64 bytes
    body = re.search(r"typedef struct gclm_overlay_style \{(.*?)\} gclm_overlay_style;", header, re.S).group(1)
    names = re.findall(r"(\w+)(?:\[4\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f for f, _ in _lib.GclmOverlayStyle._fields_] and C.sizeof(_lib.GclmOverlayStyle) == 64


# ------------------------------------------------------------------ refusals
# fake, never dereferenced device addresses: every call below must be refused before the first HIP call.  The byte images sit
# at odd addresses on purpose.
CAM, GRAV, SRC, DST, CONF, PAL, HEAT = 0x100000, 0x200000, 0x800001, 0x4000003, 0x6000000, 0x7000001, 0x7100003
OK = dict(model=1, cam=CAM, grav=GRAV, nb=1, src=SRC, B=2, C=3, H=48, W=64, il=1, conf=CONF, pal=PAL, heat=HEAT, dst=DST,
          st_layers=og.ALL, st_levels=15, st_line_halfwidth=1.0, st_arrow_step=12, st_arrow_x0=8, st_arrow_y0=10, st_arrow_length=7.0,
          st_arrow_halfwidth=1.0, st_arrow_tip=0.3, st_heat_alpha=0.4, st_tint_alpha=0.4, st_heat_lo=-4.0, st_heat_hi=0.0, st_size=64,
          style=True)
IMG, PLANE = 2 * 3 * 48 * 64, 2 * 48 * 64 * 4
NAN, INF = float("nan"), float("inf")
BAD = [("NULL camera", dict(cam=None)), ("NULL gravity", dict(grav=None)), ("NULL source", dict(src=None)),
       ("NULL destination", dict(dst=None)), ("NULL style", dict(style=False)), ("model -1", dict(model=-1)), ("model 4", dict(model=4)),
       ("B = 0", dict(B=0)), ("B > 65535", dict(B=65536)), ("C = 2", dict(C=2)), ("C = 5", dict(C=5)), ("C = 1", dict(C=1)),
       ("H = 0", dict(H=0)), ("W = 0", dict(W=0)), ("H * W > 2^31 - 1", dict(H=65536, W=32768)), ("cal_batch 0", dict(nb=0)),
       ("cal_batch 3 of B = 2", dict(nb=3)), ("interleaved = 2", dict(il=2)), ("interleaved = -1", dict(il=-1)),
       ("struct_size 60", dict(st_size=60)), ("struct_size 0", dict(st_size=0)), ("unknown layer bit", dict(st_layers=og.ALL | 32)),
       ("heat alpha 1.5", dict(st_heat_alpha=1.5)), ("heat alpha NaN", dict(st_heat_alpha=NAN)),
       ("tint alpha -0.1", dict(st_tint_alpha=-0.1)), ("tint alpha inf", dict(st_tint_alpha=INF)),
       ("hi = lo", dict(st_heat_hi=-4.0)), ("hi < lo", dict(st_heat_hi=-5.0)), ("hi NaN", dict(st_heat_hi=NAN)),
       ("lo -inf", dict(st_heat_lo=-INF)), ("levels 1", dict(st_levels=1)), ("levels even with the horizon", dict(st_levels=14)),
       ("negative line half-width", dict(st_line_halfwidth=-0.5)), ("line half-width NaN", dict(st_line_halfwidth=NAN)),
       ("arrow half-width inf", dict(st_arrow_halfwidth=INF)), ("negative arrow length", dict(st_arrow_length=-1.0)),
       ("arrow step 0", dict(st_arrow_step=0)), ("negative arrow origin", dict(st_arrow_x0=-1)),
       ("reach 12.25 of step 12", dict(st_arrow_length=10.75)), ("tip 1.5", dict(st_arrow_tip=1.5)), ("tip NaN", dict(st_arrow_tip=NAN)),
       ("tint without a palette", dict(pal=None)), ("heat without a palette", dict(heat=None)),
       ("heat without a confidence", dict(conf=None)),
       ("contours without a palette", dict(pal=None, st_layers=og.CONTOURS)),
       ("camera off a 4-byte boundary", dict(cam=CAM + 2)), ("gravity off a 4-byte boundary", dict(grav=GRAV + 1)),
       ("confidence off a 4-byte boundary", dict(conf=CONF + 2)),
       ("destination is the source", dict(dst=SRC)),
       ("destination starts at the source's last byte", dict(dst=SRC + IMG - 1)),
       ("source starts at the destination's last byte", dict(src=DST + IMG - 1)),
       ("destination ends one byte inside the camera", dict(dst=CAM - IMG + 1)),
       ("destination starts at the gravity's last byte", dict(dst=GRAV + 11)),
       ("destination starts at the confidence's last byte", dict(dst=CONF + PLANE - 1)),
       ("destination ends one byte inside the palette", dict(dst=PAL - IMG + 1)),
       ("destination starts at the heat palette's last byte", dict(dst=HEAT + 767))]
NEIGHBOURS = [dict(), dict(il=0), dict(C=4), dict(nb=2), dict(H=1, W=1), dict(st_levels=14, st_layers=og.ALL & ~og.HORIZON),
              dict(st_levels=2, st_layers=og.CONTOURS), dict(st_heat_alpha=0.0, st_tint_alpha=1.0), dict(st_line_halfwidth=0.0),
              dict(st_arrow_length=10.5), dict(st_arrow_tip=0.0), dict(st_arrow_tip=1.0),
              dict(st_arrow_step=0, st_arrow_length=99.0, st_arrow_tip=7.0, st_layers=og.ALL & ~og.ARROWS),      # arrows off: not read
              dict(pal=None, st_layers=og.HORIZON | og.ARROWS), dict(conf=None, heat=None, st_layers=og.ALL & ~og.HEAT),
              dict(st_layers=0, conf=None, pal=None, heat=None),
              dict(dst=SRC + IMG), dict(src=DST + IMG), dict(dst=GRAV + 12), dict(dst=CONF + PLANE), dict(dst=HEAT + 768),
              dict(dst=CAM - IMG), dict(src=SRC + 1, dst=DST + 2)]


def _style(a):
    st = _lib.GclmOverlayStyle()
    st.struct_size = a["st_size"]
    for k, v in a.items():
        if k.startswith("st_") and k != "st_size":
            setattr(st, k[3:], v)
    return C.byref(st) if a["style"] else None


def _draw_u8(a):
    return _lib.load().gclm_draw_fields_u8(a["model"], a["cam"], a["grav"], a["nb"], a["src"], a["B"], a["C"], a["H"], a["W"], a["il"],
                                           a["conf"], a["pal"], a["heat"], _style(a), a["dst"], None)


def _draw_f32(a):
    """The float entry on the same table: no layout flag, the images on 4-byte boundaries and four times as long."""
    src, dst = (None if a[k] is None else a[k] & ~3 for k in ("src", "dst"))
    return _lib.load().gclm_draw_fields(a["model"], a["cam"], a["grav"], a["nb"], src, a["B"], a["C"], a["H"], a["W"], a["conf"],
                                        a["pal"], a["heat"], _style(a), dst, None)


PLAIN = [b for b in BAD if not ({"il", "src", "dst"} & set(b[1])) or b[0].startswith("NULL")]


@pytest.mark.parametrize("what,change", BAD, ids=[b[0] for b in BAD])
def test_draw_fields_u8_refuses_invalid_arguments_before_any_hip_call(what, change):
    assert _draw_u8({**OK, **change}) == -3, what


@pytest.mark.parametrize("what,change", PLAIN, ids=[b[0] for b in PLAIN])
def test_draw_fields_refuses_invalid_arguments_before_any_hip_call(what, change):
    assert _draw_f32({**OK, **change}) == -3, what


def test_draw_fields_refuses_overlaps_and_misaligned_images():
    F_SRC, F_DST, n = 0x800000, 0x4000000, 4 * IMG
    for change in (dict(src=F_SRC + 2), dict(dst=F_DST + 1), dict(dst=F_SRC), dict(dst=F_SRC + n - 4), dict(src=F_DST + n - 4),
                   dict(dst=CONF + PLANE - 4), dict(dst=CAM - n + 4)):
        a = {**OK, "src": F_SRC, "dst": F_DST, **change}
        assert _lib.load().gclm_draw_fields(a["model"], a["cam"], a["grav"], a["nb"], a["src"], a["B"], a["C"], a["H"], a["W"],
                                            a["conf"], a["pal"], a["heat"], _style(a), a["dst"], None) == -3, change


def test_the_refusal_table_changes_one_thing_at_a_time():
    assert all(set(change) <= set(OK) and 1 <= len(change) <= 2 for _, change in BAD)


def test_the_valid_neighbours_reach_the_launch():
    """The neighbours of the refused calls -- ranges that only touch, the other layout, the extremes of every interval, layers
    whose inputs are absent because they are off -- are valid and reach the launch, which fails without a device: -10."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: a valid call would launch on fake addresses")
    for change in NEIGHBOURS:
        assert _draw_u8({**OK, **change}) == -10, change
    for change in NEIGHBOURS[:16]:
        assert _draw_f32({**OK, **change}) == -10, change


# ------------------------------------------------------------------ the gate's own conditions, for every case
@pytest.fixture(scope="module")
def parts():
    cache = {}

    def get(case, tie=False):
        if (case, tie) not in cache:
            cache[(case, tie)] = og.parts(case, tie)
        return cache[(case, tie)]
    return get


def _cpu_call(c, p, img, **changes):
    cam, grav = camera_models[c.model](p["cams"]), Gravity(p["gravs"])
    grav._data = p["gravs"]                                      # (as given: the constructor renormalises)
    args = dict(tint=bool(c.layers & og.TINT), contours=bool(c.layers & og.CONTOURS), horizon=bool(c.layers & og.HORIZON),
                up=bool(c.layers & og.ARROWS), confidence=p["conf"] if c.layers & og.HEAT else None, palette=p["pal"],
                heat_palette=p["heat"], style=p["style"])
    return viz.draw_perspective_fields(img, cam, grav, **{**args, **changes})


@pytest.mark.parametrize("case", og.CASES, ids=[og.case_id(c) for c in og.CASES])
def test_conditions_hold_and_the_cpu_path_passes_the_gate(parts, case):
    p = parts(case)
    assert p["share"] <= og.CAP, p["share"]                       # a condition on the cases
    assert p["img"].float().std() > 20 and 0 < p["bound"] < 1
    out = _cpu_call(case, p, p["img"])
    ratio = og.worst_ratio(out, p)
    out_f = _cpu_call(case, p, p["img_f"])
    ratio_f = og.worst_ratio(out_f, p, floats=True)
    print(f"{og.case_id(case)}: bound {p['bound']:.3g} / {p['bound_f']:.3g} byte steps, excluded {p['share']:.4f}, CPU path worst "
          f"ratio {ratio:.3f} (bytes) {ratio_f:.3f} (floats)")
    assert out.dtype == torch.uint8 and out_f.dtype == torch.float32 and ratio <= 1 and ratio_f <= 1
    if case.C == 4:
        assert torch.equal(out[:, 3], p["img"][:, 3]) and torch.equal(out_f[:, 3], p["img_f"][:, 3])
    if case.layers == og.ALL and case.H >= 41:
        assert (out[:, :3] != p["img"][:, :3]).double().mean() > 0.9          # something was drawn


MUTANTS = ["half-pixel offset", "level step 180/15", "half-width + 1", "tint alpha 0.5", "swapped channel order",
           "arrows one cell off", "tip at 30 degrees", "nearest-bin palette"]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_gate_fails_each_mutant(parts, mutant):
    case = next(c for c in og.CASES if c.layers == og.ALL and c.grav == "horizon" and c.model == "simple_radial")
    p = parts(case)
    out, _ = og.render(case, p, torch.float32, mutant=mutant)
    ratio = og.worst_ratio(og.quantise(out), p)
    honest = og.worst_ratio(og.quantise(og.render(case, p, torch.float32)[0]), p)
    print(f"{mutant}: worst ratio {ratio:.3g} (honest {honest:.3f})")
    assert honest <= 1 < ratio, (mutant, ratio)


def test_ties_gate_passes_the_cpu_path_and_fails_round_half_up(parts):
    c = og.TIE_CASE
    p = parts(c, True)
    wrong, ties = og.ties_to_even(_cpu_call(c, p, p["img"]), p)
    assert wrong == 0 and ties > 1000
    exact, _ = og.render(c, p, torch.float32)
    up = (exact + 0.5).floor().clamp(0, 255).to(torch.uint8)
    wrong, _ = og.ties_to_even(up, p)
    assert og.worst_ratio(up, p) <= 1 and wrong > 100             # the value gate cannot tell; the ties gate does


# ------------------------------------------------------------------ the public call on the CPU
def test_cpu_call_keeps_dtype_and_memory_format_and_copies_exactly(parts):
    c = next(c for c in og.CASES if c.C == 4 and c.H == 41)
    p = parts(c)
    want = _cpu_call(c, p, p["img"])
    cl = p["img"].contiguous(memory_format=torch.channels_last)
    out = _cpu_call(c, p, cl)
    assert want.is_contiguous() and out.is_contiguous(memory_format=torch.channels_last) and not out.is_contiguous()
    assert torch.equal(out, want) and _cpu_call(c, p, p["img_f"]).is_contiguous()
    off = dict(tint=False, contours=False, horizon=False, up=False, confidence=None)
    for img in (p["img"], cl, p["img_f"]):
        copy = _cpu_call(c, p, img, **off)
        assert torch.equal(copy, img) and copy.data_ptr() != img.data_ptr()
        nan = {**p, "cams": torch.full_like(p["cams"], float("nan"))}
        assert torch.equal(_cpu_call(c, nan, img, confidence=None), img)
    with pytest.raises(ValueError):
        _cpu_call(c, p, p["img"][:, :2])
    with pytest.raises(ValueError):                                # the reach condition is the call's
        _cpu_call(c, {**p, "style": viz.OverlayStyle.default(41, 59, arrow_length=30.0)}, p["img"])
    with pytest.raises(ValueError):
        _cpu_call(c, {**p, "style": viz.OverlayStyle.default(41, 59, levels=14)}, p["img"], horizon=True)


def test_default_style_is_the_demos():
    st = viz.OverlayStyle.default(480, 640)
    assert (st.line_halfwidth, st.arrow_step, st.arrow_x0, st.arrow_y0, st.arrow_length) == (1.5, 48, 32, 43, 30.0)
    assert (st.arrow_tip, st.tint_alpha, st.heat_alpha, st.levels, st.heat_range) == (0.3, 0.4, 0.4, 15, (-4.0, 0.0))
    assert viz.OverlayStyle.default(1280, 1920).line_halfwidth == 5.0 and viz.OverlayStyle.default(48, 64).line_halfwidth == 0.5
    viz.OverlayStyle.default(1, 1).check(og.ALL & ~og.ARROWS)


def test_builtin_seismic_is_matplotlibs_and_palettes_are_cached():
    pal = viz.resolve_palette("seismic", "cpu")
    assert pal.dtype == torch.uint8 and pal.shape == (256, 3) and viz.resolve_palette("seismic", "cpu") is pal
    assert pal[0].tolist() == [0, 0, 76] and pal[-1].tolist() == [128, 0, 0] and pal[127].min() > 250
    try:
        import matplotlib
    except ImportError:
        with pytest.raises(RuntimeError, match="matplotlib"):
            viz.resolve_palette("turbo", "cpu")
        return
    theirs = torch.from_numpy(matplotlib.colormaps["seismic"](torch.linspace(0, 1, 256).numpy(), bytes=True)[:, :3].copy())
    assert (pal.int() - theirs.int()).abs().max() <= 1
    assert viz.resolve_palette("turbo", "cpu").shape == (256, 3)
    with pytest.raises(ValueError):
        viz.resolve_palette("no such colormap", "cpu")


# ------------------------------------------------------------------ code objects
@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="LLVM tools missing")
def test_the_twelve_kernels_exist_without_scratch_and_within_2_kb_of_lds(tmp_path):
    from test_kernel_audit import kernel_metadata
    k = {n: v for n, v in kernel_metadata(tmp_path).items() if "overlay_kernel" in n}
    assert len(k) == 12, sorted(k)
    for m in range(4):
        for kind in ("EfLb0E", "EhLb0E", "EhLb1E"):               # float planar, bytes planar, bytes interleaved
            v = [v for n, v in k.items() if f"overlay_kernelILi{m}{kind}" in n]
            assert len(v) == 1, (m, kind)
    print({n: v for n, v in k.items()})
    assert all(v["scratch"] == 0 and v["lds"] <= 2048 for v in k.values()), k
    assert all(v["vgpr"] <= 52 for v in k.values()), k            # as built: 42 .. 47; 8 waves per SIMD up to 64
