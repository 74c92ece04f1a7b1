"""GPU: the field overlay on the HIP path (gclm_draw_fields, gclm_draw_fields_u8; viz.draw_perspective_fields) against the
float64 yardstick of tests/overlay_gate.py, whose conditions test_overlay_abi.py checks on the CPU.

Every case runs through the C ABI on flat buffers of the test's own -- byte images at odd offsets inside a larger buffer with
guard bytes on both sides -- and through the public call, in every image kind: bytes planar, bytes interleaved, float32."""
import ctypes
import functools

import pytest
import torch

from geocalib_amd import Gravity, _call, _lib, camera_models, viz
import overlay_gate as og

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD, FRONT = 77, 5            # guard byte; the byte offset of source and destination inside their buffers (odd: no dword path)


@functools.lru_cache(maxsize=None)
def parts(c, tie=False):
    """The yardstick of one case, computed once on the CPU and left unchanged."""
    return og.parts(c, tie)


def flat(img, interleaved):
    return (img.permute(0, 2, 3, 1) if interleaved else img).contiguous().reshape(-1)


def unflat(buf, c, interleaved):
    return buf.view(c.B, c.H, c.W, c.C).permute(0, 3, 1, 2) if interleaved else buf.view(c.B, c.C, c.H, c.W)


def abi_draw(c, p, kind, layers=None, cams=None, front=FRONT, stream=None):
    """One C call of case `c` on flat device buffers: kind "planar" / "interleaved" (bytes, placed `front` bytes into buffers
    of GUARD bytes) or "float".  Returns the output (B, C, H, W) on the CPU after checking the guards."""
    layers = c.layers if layers is None else layers
    cams = (p["cams"] if cams is None else cams).to(DEV)
    gravs, conf, pal, heat = (p[k].to(DEV) for k in ("gravs", "conf", "pal", "heat"))
    st = p["style"].c_struct(layers)
    n = c.B * c.C * c.H * c.W
    stream = _call.raw_stream(DEV) if stream is None else stream
    head = (_lib.CAMERA_MODEL_IDS[c.model], cams.data_ptr(), gravs.data_ptr(), c.nb)
    tail = (conf.data_ptr(), pal.data_ptr(), heat.data_ptr(), ctypes.byref(st))
    if kind == "float":
        src, dst = p["img_f"].to(DEV).contiguous(), torch.full((n,), -1.0, device=DEV)
        _call.call("gclm_draw_fields", *head, src.data_ptr(), c.B, c.C, c.H, c.W, *tail, dst.data_ptr(), stream, device=DEV)
        torch.cuda.synchronize()
        return dst.view(c.B, c.C, c.H, c.W).cpu()
    il = kind == "interleaved"
    big_src = torch.full((n + 16,), GUARD, dtype=torch.uint8, device=DEV)
    big_dst = torch.full((n + 16,), GUARD, dtype=torch.uint8, device=DEV)
    big_src[front:front + n] = flat(p["img"], il).to(DEV)
    _call.call("gclm_draw_fields_u8", *head, big_src[front:].data_ptr(), c.B, c.C, c.H, c.W, int(il), *tail,
               big_dst[front:].data_ptr(), stream, device=DEV)
    torch.cuda.synchronize()
    assert (big_dst[:front] == GUARD).all() and (big_dst[front + n:] == GUARD).all(), "guard bytes written"
    return unflat(big_dst[front:front + n], c, il).cpu()


def gravity_of(vec):
    """A Gravity holding `vec` as given (the constructor renormalises, which may move a component by an ulp)."""
    g = Gravity(vec)
    g._data = vec
    return g


def api_draw(c, p, kind, **changes):
    """The public call of case `c`; returns the output on the CPU after checking dtype and memory format."""
    L = og
    cam = camera_models[c.model](p["cams"].to(DEV))
    grav = gravity_of(p["gravs"].to(DEV))
    if kind == "float":
        img = p["img_f"].to(DEV)
    else:
        img = p["img"].to(DEV)
        img = img.contiguous(memory_format=torch.channels_last) if kind == "interleaved" else img
    args = dict(tint=bool(c.layers & L.TINT), contours=bool(c.layers & L.CONTOURS), horizon=bool(c.layers & L.HORIZON),
                up=bool(c.layers & L.ARROWS), confidence=p["conf"].to(DEV) if c.layers & L.HEAT else None, palette=p["pal"],
                heat_palette=p["heat"], style=p["style"])
    out = viz.draw_perspective_fields(img, cam, grav, **{**args, **changes})
    torch.cuda.synchronize()
    assert out.dtype == img.dtype and out.shape == img.shape and out.is_cuda and out.data_ptr() != img.data_ptr()
    assert out.is_contiguous(memory_format=torch.channels_last if kind == "interleaved" else torch.contiguous_format)
    return out.cpu()


KINDS = ("planar", "interleaved", "float")


@functools.lru_cache(maxsize=None)
def outputs(c):
    p = parts(c)
    return {kind: (abi_draw(c, p, kind), api_draw(c, p, kind)) for kind in KINDS}


@pytest.mark.parametrize("case", og.CASES, ids=[og.case_id(c) for c in og.CASES])
def test_parity_against_float64(case):
    p = parts(case)
    assert p["share"] <= og.CAP
    outs = outputs(case)
    for kind in KINDS:
        abi, api = outs[kind]
        ratio = og.worst_ratio(abi, p, floats=kind == "float")
        print(f"{og.case_id(case)} {kind}: bound {p['bound']:.3g} byte steps, worst ratio to the gate {ratio:.3f}")
        assert ratio <= 1, (kind, ratio)
        assert torch.equal(abi, api), kind                       # the public call is that C call
        if case.C == 4:                                          # channel 3 is copied
            assert torch.equal(abi[:, 3], (p["img_f"] if kind == "float" else p["img"])[:, 3]), kind
    assert torch.equal(outs["planar"][0], outs["interleaved"][0])      # the two layouts write the same bytes


def test_ties_round_to_even():
    c = og.TIE_CASE
    p = parts(c, True)
    for kind in ("planar", "interleaved"):
        out = abi_draw(c, p, kind)
        wrong, ties = og.ties_to_even(out, p)
        assert ties > 1000 and wrong == 0, (kind, wrong, ties)
        assert og.worst_ratio(out, p) <= 1


def test_the_dword_path_writes_the_bytes_of_the_byte_path():
    c = next(c for c in og.CASES if c.C == 4 and c.H == 41)
    p = parts(c)
    aligned = abi_draw(c, p, "interleaved", front=8)              # C = 4, both images on a dword: one dword per pixel
    assert torch.equal(aligned, outputs(c)["interleaved"][0])
    assert torch.equal(aligned, abi_draw(c, p, "interleaved", front=6))


@pytest.mark.parametrize("kind", KINDS)
def test_layers_off_and_a_nan_calibration_give_exact_copies(kind):
    c = next(c for c in og.CASES if c.C == 4 and c.H == 41)
    p = parts(c)
    src = p["img_f"] if kind == "float" else p["img"]
    assert torch.equal(abi_draw(c, p, kind, layers=0), src)
    nan = p["cams"].clone()
    nan[:, 2] = float("nan")
    assert torch.equal(abi_draw(c, p, kind, layers=og.ALL & ~og.HEAT, cams=nan), src)
    off = api_draw(c, p, kind, tint=False, contours=False, horizon=False, up=False, confidence=None)
    assert torch.equal(off, src)
    one = p["cams"].clone()                                       # nb = 1 here: a per-image batch with one NaN camera
    cams = one.expand(c.B, -1).clone()
    cams[1, 4] = float("nan")
    c3 = c._replace(nb=3)
    p3 = {**p, "cams": cams, "gravs": p["gravs"].expand(c.B, -1).contiguous()}
    out = abi_draw(c3, p3, kind, layers=og.ALL & ~og.HEAT)
    clean = abi_draw(c, p, kind, layers=og.ALL & ~og.HEAT)
    assert torch.equal(out[1], src[1]) and torch.equal(out[0], clean[0]) and torch.equal(out[2], clean[2])


def test_two_runs_are_bit_identical_and_a_side_stream_works():
    c = og.CASES[0]
    p = parts(c)
    for kind in KINDS:
        first = outputs(c)[kind][0]
        assert torch.equal(abi_draw(c, p, kind), first)
        side = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(side):
            assert _call.raw_stream(DEV) == side.cuda_stream
            assert torch.equal(abi_draw(c, p, kind, stream=side.cuda_stream), first)
            assert torch.equal(api_draw(c, p, kind), first)


def test_a_batch_of_65537_crosses_the_launch_slicing():
    B = 65536 + 1
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (B, 3, 1, 1), generator=g, dtype=torch.uint8)
    f = 40 + torch.arange(B, dtype=torch.float32) / 1000
    cams = torch.stack([torch.ones(B), torch.ones(B), f, f, torch.zeros(B), torch.zeros(B), torch.zeros(B), torch.zeros(B)], -1)
    pitch = torch.linspace(-1.4, 1.4, B, dtype=torch.float64)
    gravs = torch.stack([torch.zeros_like(pitch), -torch.cos(pitch), torch.sin(pitch)], -1).to(torch.float32)
    style = viz.OverlayStyle.default(1, 1)
    want = viz.draw_perspective_fields(img, camera_models["pinhole"](cams), gravity_of(gravs), contours=False, style=style)
    out = viz.draw_perspective_fields(img.to(DEV), camera_models["pinhole"](cams.to(DEV)), gravity_of(gravs.to(DEV)), contours=False,
                                      style=style)
    torch.cuda.synchronize()
    diff = (out.cpu().int() - want.int()).abs()
    assert diff.max() <= 1 and (diff > 0).double().mean() < 0.01         # float32 against float32: a byte moves at a near tie only
    assert (out.cpu() != img).any(dim=1).double().mean() > 0.9           # ... and the images past the first slice are drawn
    assert (out.cpu()[65535:] != img[65535:]).any()


def test_the_default_style_and_named_palettes_draw():
    img = torch.randint(0, 256, (2, 3, 480, 640), dtype=torch.uint8, device=DEV)
    cams = torch.tensor([[640, 480, 500, 500, 320, 240, 0, 0]], dtype=torch.float32, device=DEV)
    grav = Gravity.from_rp(torch.tensor([0.1], device=DEV), torch.tensor([0.2], device=DEV))
    out = viz.draw_perspective_fields(img, camera_models["pinhole"](cams), grav, horizon=True, up=True)
    want = viz.draw_perspective_fields(img.cpu(), camera_models["pinhole"](cams.cpu()), gravity_of(grav._data.cpu()), horizon=True, up=True)
    torch.cuda.synchronize()
    diff = (out.cpu().int() - want.int()).abs()
    assert diff.max() <= 1 and (diff > 0).double().mean() < 0.01
    st = viz.OverlayStyle.default(480, 640)
    green = (out.cpu() == torch.tensor(st.arrow_color, dtype=torch.uint8)[None, :, None, None]).all(1)
    assert green[:, st.arrow_y0, st.arrow_x0].all()                       # an arrow starts at its anchor
