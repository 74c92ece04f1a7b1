"""GPU: the uint8 image calls on the HIP path (gclm_undistort_image_u8, gclm_reproject_image_u8) in both layouts, against the
float64 yardsticks of tests/undistort_gate.py and tests/reproject_gate.py fed the byte image.

Gate (tests/u8_image_gate.py, its conditions checked on CPU by test_u8_image_abi.py): |out - ref| <= bound + 0.5, the float
gate plus half a step of the quantiser; the mask as for the float call.  Beside it: values known exactly (ties, copies), the
same bytes from unaligned buffers, and the edges of the shape space held to the float kernel's own output."""
import functools

import pytest
import torch

from geocalib_amd import Gravity, _call, _lib, camera as camera_module, camera_models
import reproject_gate as rg
import u8_image_gate as u8g
import undistort_gate as ug

pytestmark = pytest.mark.gpu

LAYOUTS = ("planar", "interleaved")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def in_layout(img, layout):
    """`img` (B, C, H, W) as torch holds that layout: contiguous, or channels_last (the memory of (B, H, W, C))."""
    return img.contiguous() if layout == "planar" else img.contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------------ the C ABI on buffers of the test's own
def flat(img, interleaved):
    """The bytes of `img` (B, C, H, W) in the call's memory order."""
    return (img.permute(0, 2, 3, 1) if interleaved else img).contiguous().reshape(-1)


def unflat(buf, B, C, H, W, interleaved):
    return buf.view(B, H, W, C).permute(0, 3, 1, 2) if interleaved else buf.view(B, C, H, W)


def abi_reproject(sm, scam, tm, tcam, rot, src, shape, Hs, Ws, H, W, interleaved, dst, valid=None):
    """gclm_reproject_image_u8 on flat byte buffers `src`, `dst` (any byte offset into a larger allocation)."""
    B, C, Hin, Win = shape
    ids = _lib.CAMERA_MODEL_IDS
    _call.call("gclm_reproject_image_u8", ids[sm], scam.data_ptr(), ids[tm], tcam.data_ptr(), scam.shape[0], _call.ptr(rot),
               1 if rot is None else rot.shape[0], src.data_ptr(), B, C, Hin, Win, Hs, Ws, H, W, int(interleaved), dst.data_ptr(),
               _call.ptr(valid), _call.raw_stream(src.device), device=src.device)
    torch.cuda.synchronize()


def abi_undistort(model, cam, src, shape, H, W, interleaved, dst):
    B, C, Hin, Win = shape
    _call.call("gclm_undistort_image_u8", _lib.CAMERA_MODEL_IDS[model], cam.data_ptr(), cam.shape[0], src.data_ptr(), B, C, Hin,
               Win, H, W, int(interleaved), dst.data_ptr(), _call.raw_stream(src.device), device=src.device)
    torch.cuda.synchronize()


def pinhole(W, H, f, cx, cy, n=1):
    return torch.tensor([[W, H, f, f, cx, cy, 0, 0]], dtype=torch.float32).expand(n, -1).contiguous()


def random_bytes(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, C, H, W), generator=g, dtype=torch.uint8)


# ------------------------------------------------------------------ parity
BIG = ("simple_radial", None, None, None, "pinhole", None, None, "roll25", 1, 1, 479, 641, "noise")     # many tiles, W % 4 = 1
R_CASES = rg.CASES + [BIG]


@functools.lru_cache(maxsize=None)
def parts(case):
    """The yardstick of one case, computed once on the CPU and left unchanged."""
    return u8g.reproject_parts(case)


@functools.lru_cache(maxsize=None)
def outputs(case):
    """The device's output of one case in both layouts, (image, mask) on the CPU, computed once."""
    p, dev = parts(case), torch.device("cuda:0")
    src, tgt = camera_models[case[0]](p["src"].to(dev)), camera_models[case[4]](p["tgt"].to(dev))
    rot = None if p["rot"] is None else p["rot"].to(dev)
    res = {}
    for layout in LAYOUTS:
        img = in_layout(p["img"].to(dev), layout)
        out, valid = src.reproject_image(img, tgt, rot, return_valid=True)
        torch.cuda.synchronize()
        assert out.dtype == torch.uint8 and out.is_cuda and valid.dtype == torch.bool
        assert out.is_contiguous(memory_format=torch.contiguous_format if layout == "planar" else torch.channels_last)
        assert torch.equal(src.reproject_image(img, tgt, rot), out)             # without the mask: the same image
        res[layout] = (out.cpu(), valid.cpu())
    return res


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", R_CASES, ids=[rg.case_id(c) for c in R_CASES])
def test_reproject_parity_against_float64(dev, case, layout):
    p = parts(case)
    out, valid = outputs(case)[layout]
    assert out.shape == p["ref"].shape and valid.shape == p["valid"].shape
    ratio = u8g.worst_ratio(out, p["ref"], p["bound"])
    wrong = ((valid != p["valid"]) & ~p["mask_free"]).sum().item()
    print(f"{rg.case_id(case)} {layout}: delta {p['delta']:.2e} px, worst ratio to the gate {ratio:.3f}, mask pixels off {wrong}")
    assert ratio <= 1, ratio
    assert wrong == 0, wrong
    if case[7] == "yaw100":
        assert (out == 0).all() and not valid.any()


@pytest.mark.parametrize("case", R_CASES, ids=[rg.case_id(c) for c in R_CASES])
def test_reproject_layouts_agree(dev, case):
    """The two instantiations may contract the four-term sum differently, which moves a sample by a few ulp and a byte by at
    most one step, at a near tie; nothing else may differ."""
    (a, va), (b, vb) = (outputs(case)[layout] for layout in LAYOUTS)
    diff = (a.int() - b.int()).abs()
    print(f"{rg.case_id(case)}: {int((diff > 0).sum())} of {diff.numel()} bytes differ between the layouts")
    assert diff.max() <= 1 and torch.equal(va, vb)


@pytest.mark.parametrize("case", ug.CASES, ids=[u8g.undistort_id(c) for c in ug.CASES])
def test_undistort_parity_against_float64_in_both_layouts(dev, case):
    model, k1, k2, B, nb, C, H, W, Hin, Win, kind = case
    p = u8g.undistort_parts(case, device=dev)
    cam = camera_models[model](p["cams"].to(dev))
    outs = []
    for layout in LAYOUTS:
        out = cam.undistort_image(in_layout(p["img"].to(dev), layout))
        torch.cuda.synchronize()
        assert out.shape == (B, C, H, W) and out.dtype == torch.uint8 and out.is_cuda
        assert out.is_contiguous(memory_format=torch.contiguous_format if layout == "planar" else torch.channels_last)
        ratio = u8g.worst_ratio(out, p["ref"], p["bound"])
        print(f"{u8g.undistort_id(case)} {layout}: delta {p['delta']:.2e} px, worst ratio to the gate {ratio:.3f}")
        assert ratio <= 1, ratio
        outs.append(out)
    assert (outs[0].int() - outs[1].int()).abs().max() <= 1


def test_hip_path_is_taken_without_a_copy(dev, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("torch composition called")

    monkeypatch.setattr(camera_module, "_reproject_torch", refuse)
    monkeypatch.setattr(torch.nn.functional, "grid_sample", refuse)
    monkeypatch.setattr(camera_module.F, "grid_sample", refuse)
    cam = camera_models["radial"](ug.make_cameras("radial", 1, 64, 96, seed=13).to(dev))
    img = random_bytes(2, 3, 64, 96, seed=1).to(dev)
    for layout in LAYOUTS:
        im = in_layout(img, layout)
        t, flag = _call.dev_u8(im, "img")
        assert t.data_ptr() == im.data_ptr() and flag == (layout == "interleaved")
        assert cam.undistort_image(im).shape == cam.reproject_image(im).shape == (2, 3, 64, 96)
    five = in_layout(random_bytes(2, 5, 64, 96, seed=2).to(dev), "interleaved")          # C > 4: copied to planar
    t, flag = _call.dev_u8(five, "img")
    assert flag == 0 and t.is_contiguous() and t.data_ptr() != five.data_ptr()
    out = cam.reproject_image(five)
    assert out.is_contiguous(memory_format=torch.channels_last) and torch.equal(out, cam.reproject_image(five.contiguous()))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ values known exactly
@pytest.mark.parametrize("interleaved", (0, 1), ids=LAYOUTS)
@pytest.mark.parametrize("C", (1, 3, 4))
def test_exact_ties_round_to_even(dev, C, interleaved):
    """Pinhole to pinhole, f = 64, the target's principal point half a pixel to the right: every intermediate is a short
    dyadic rational, so the sample is exactly (left + right) / 2, with 0 beyond the left edge; about half of them are ties."""
    B, H, W = 2, 8, 32
    img = random_bytes(B, C, H, W, seed=20 + C)
    left = torch.cat([torch.zeros_like(img[..., :1]), img[..., :-1]], -1).int()
    total = left + img.int()
    half = total // 2
    want = torch.where(total % 2 == 1, half + (half & 1), half).to(torch.uint8)          # ties to even, in integers
    assert (total % 2 == 1).double().mean() >= 0.4
    dst = torch.full((B * C * H * W,), 255, dtype=torch.uint8, device=dev)
    abi_reproject("pinhole", pinhole(W, H, 64, 16, 4).to(dev), "pinhole", pinhole(W, H, 64, 16.5, 4).to(dev), None,
                  flat(img, interleaved).to(dev), (B, C, H, W), H, W, H, W, interleaved, dst)
    assert torch.equal(unflat(dst, B, C, H, W, interleaved).cpu(), want)


@pytest.mark.parametrize("interleaved", (0, 1), ids=LAYOUTS)
@pytest.mark.parametrize("C", (1, 2, 3, 4))
@pytest.mark.parametrize("W", (53, 130))
def test_identity_is_a_byte_exact_copy(dev, W, C, interleaved):
    """The same pinhole camera on both sides, an exactly representable principal point, Win = W: odd, and two tiles with a
    ragged tail.  (reproject_image multiplies by 1 / f and by f again: exact for f = 64.)"""
    B, H = 2, 9
    img = random_bytes(B, C, H, W, seed=30 + C)
    src = flat(img, interleaved).to(dev)
    cam = pinhole(W, H, 64, W / 2, H / 2).to(dev)
    dst = torch.zeros_like(src)
    abi_reproject("pinhole", cam, "pinhole", cam, None, src, (B, C, H, W), H, W, H, W, interleaved, dst)
    assert torch.equal(dst, src)
    shifted = torch.cat([src[:1], src])[1:]          # the source one byte off a dword, the destination on it: another path
    assert shifted.data_ptr() % 4 == 1
    dst.zero_()
    abi_reproject("pinhole", cam, "pinhole", cam, None, shifted, (B, C, H, W), H, W, H, W, interleaved, dst)
    assert torch.equal(dst, src)
    for model in ug.MODELS:
        dst.zero_()
        abi_undistort(model, pinhole(W, H, 0.7 * W, W / 2, H / 2).to(dev), src, (B, C, H, W), H, W, interleaved, dst)
        assert torch.equal(dst, src), model


@pytest.mark.parametrize("interleaved", (0, 1), ids=LAYOUTS)
@pytest.mark.parametrize("C", (3, 4))
def test_unaligned_bases_give_the_same_bytes(dev, C, interleaved):
    """The first parity case again, source and destination at byte offsets 1, 2, 3 into larger buffers (C = 4: a fourth
    channel added, so that the dword path of the aligned run is held to the byte path of the others)."""
    case = rg.CASES[0]
    p = parts(case)
    img = p["img"] if C == 3 else torch.cat([p["img"], p["img"][:, :1].flip(-1)], 1)
    H, W = case[10], case[11]
    shape = (rg.B, C, rg.HIN, rg.WIN)
    src, n_out = flat(img, interleaved).to(dev), rg.B * C * H * W
    scam, tcam = p["src"].to(dev), p["tgt"].to(dev)
    want, want_valid = torch.zeros(n_out, dtype=torch.uint8, device=dev), torch.zeros(rg.B * H * W, dtype=torch.uint8, device=dev)
    abi_reproject(case[0], scam, case[4], tcam, None, src, shape, rg.HS, rg.WS, H, W, interleaved, want, want_valid)
    assert want.data_ptr() % 4 == 0 and src.data_ptr() % 4 == 0 and want.float().std() > 20
    if C == 3:
        assert u8g.worst_ratio(unflat(want, rg.B, C, H, W, interleaved).cpu(), p["ref"], p["bound"]) <= 1
    for off_src, off_dst in ((1, 1), (2, 3), (3, 2), (0, 1), (1, 0)):
        big_src = torch.zeros(src.numel() + 8, dtype=torch.uint8, device=dev)
        big_dst = torch.full((n_out + 8,), 77, dtype=torch.uint8, device=dev)
        big_src[off_src:off_src + src.numel()] = src
        valid = torch.zeros_like(want_valid)
        abi_reproject(case[0], scam, case[4], tcam, None, big_src[off_src:], shape, rg.HS, rg.WS, H, W, interleaved,
                      big_dst[off_dst:], valid)
        assert torch.equal(big_dst[off_dst:off_dst + n_out], want) and torch.equal(valid, want_valid), (off_src, off_dst)
        assert (big_dst[:off_dst] == 77).all() and (big_dst[off_dst + n_out:] == 77).all()      # nothing written around it
    cam = ug.make_cameras("radial", 1, H, W, seed=2).to(dev)
    abi_undistort("radial", cam, src, shape, H, W, interleaved, want)
    big_src = torch.zeros(src.numel() + 8, dtype=torch.uint8, device=dev)
    big_dst = torch.full((n_out + 8,), 77, dtype=torch.uint8, device=dev)
    big_src[3:3 + src.numel()] = src
    abi_undistort("radial", cam, big_src[3:], shape, H, W, interleaved, big_dst[1:])
    assert torch.equal(big_dst[1:1 + n_out], want) and big_dst[0] == 77 and (big_dst[1 + n_out:] == 77).all()


# ------------------------------------------------------------------ the edges of the shape space
def against_the_float_kernel(src, tgt, rot, img, layout):
    """The byte call against the float call of the same arguments, rounded: both are float32 evaluations of one four-term sum
    of the same taps and weights and differ by its contraction alone, a few ulp of a sample, so a byte moves by at most one
    step (at a near tie), 0 stays 0, and the masks are equal."""
    out, valid = src.reproject_image(in_layout(img, layout), tgt, rot, return_valid=True)
    ref, ref_valid = src.reproject_image(img.float(), tgt, rot, return_valid=True)
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and out.shape == ref.shape and torch.equal(valid, ref_valid)
    assert (out.int() - u8g.quantise(ref).int()).abs().max() <= 1
    assert (out[ref == 0] == 0).all()
    return out, valid


EDGES = [("1 x 1 output", dict(H=1, W=1)), ("1 x 1 source", dict(Hin=1, Win=1)), ("W = 1", dict(W=1)), ("H = 1", dict(H=1)),
         ("B = 1", dict(B=1)), ("camera batch 3", dict(nb=3)), ("rotation batch 3", dict(nr=3)),
         ("camera and rotation batch 3", dict(nb=3, nr=3)), ("no rotation", dict(nr=0))]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("what,change", EDGES, ids=[e[0] for e in EDGES])
def test_edges_of_the_shape_space(dev, what, change, layout):
    a = {**dict(B=3, H=30, W=44, Hin=rg.HIN, Win=rg.WIN, nb=1, nr=1), **change}
    src = camera_models["simple_radial"](ug.make_cameras("simple_radial", a["nb"], rg.HS, rg.WS, 0.2, seed=41).to(dev))
    tgt_cams = ug.make_cameras("radial", a["nb"], 30, 44, -0.1, 0.05, seed=42)
    tgt_cams[:, 0], tgt_cams[:, 1] = a["W"], a["H"]
    if min(a["H"], a["W"]) == 1:
        tgt_cams[:, 4], tgt_cams[:, 5] = (a["W"] - 1) / 2 + 0.1, (a["H"] - 1) / 2 + 0.2       # the few pixels look at the source
    rot = rg.make_rotations("roll25", a["nr"]).to(dev) if a["nr"] else None
    img = random_bytes(a["B"], 3, a["Hin"], a["Win"], seed=43).to(dev)
    out, valid = against_the_float_kernel(src, camera_models["radial"](tgt_cams.to(dev)), rot, img, layout)
    assert out.shape == (a["B"], 3, a["H"], a["W"]) and valid.any() and (out != 0).any()
    if what == "1 x 1 source":                  # every visible pixel samples the one source pixel with weight 1
        seen = valid[:, None].expand_as(out)
        assert torch.equal(out[seen], img.expand(-1, -1, a["H"], a["W"])[seen]) and (out[~seen] == 0).all()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_nan_in_one_camera_zeroes_that_image_only(dev, layout):
    case = ("simple_radial", None, None, None, "radial", -0.1, 0.05, "roll25", 3, 3, 37, 53, "noise")
    src, tgt, rot, img = (t.to(dev) for t in rg.case_inputs(case, seed=3))
    img = in_layout(u8g.to_bytes(img), layout)
    run = lambda s, t: camera_models["simple_radial"](s).reproject_image(img, camera_models["radial"](t), rot,  # noqa: E731
                                                                       return_valid=True)
    clean, clean_valid = run(src, tgt)
    for which in ("src", "tgt"):
        bad = {"src": src.clone(), "tgt": tgt.clone()}
        bad[which][1, 2] = float("nan")
        out, valid = run(bad["src"], bad["tgt"])
        torch.cuda.synchronize()
        assert clean_valid[1].any() and (clean[1] != 0).any()
        assert (out[1] == 0).all() and not valid[1].any()
        for i in (0, 2):
            assert torch.equal(out[i], clean[i]) and torch.equal(valid[i], clean_valid[i])
    und = camera_models["simple_radial"](src.clone())
    und._data[1, 2] = float("nan")
    img2 = in_layout(random_bytes(3, 3, 30, 44, seed=5).to(dev), layout)
    out = und.undistort_image(img2)
    assert (out[1] == 0).all() and (out[0] != 0).any() and (out[2] != 0).any()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_upright_image_is_reproject_image_with_rt_rs_transposed(dev, layout):
    cams = ug.make_cameras("simple_radial", 1, 30, 44, seed=9).to(dev)
    cam = camera_models["simple_radial"](cams)
    img = in_layout(random_bytes(3, 3, 30, 44, seed=9).to(dev), layout)
    grav = Gravity.from_rp(torch.tensor([0.3, -0.5, 0.1], device=dev), torch.tensor([0.2, 0.4, -0.3], device=dev))
    for level in (False, True):
        zero = torch.zeros(3, device=dev)
        R_t = Gravity.from_rp(zero, zero if level else grav.pitch).R
        want, want_valid = cam.reproject_image(img, rotation=R_t @ grav.R.transpose(-1, -2), return_valid=True)
        out, valid = cam.upright_image(img, grav, level_pitch=level, return_valid=True)
        torch.cuda.synchronize()
        assert out.dtype == torch.uint8 and torch.equal(out, want) and torch.equal(valid, want_valid) and valid.any()
