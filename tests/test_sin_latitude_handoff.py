"""GPU: the head epilogue hands sin(latitude) to the solve (gclm_pack_fields_ex -> gclm_calibrate_ex / LMOptimizer's
data["sin_latitude"]).

- The sixth plane of the epilogue is the sweep's own sin of the packed latitude; the five planes do not change.
- A solve handed that plane gives the bits of a solve without it, on every path, and allocates no scratch plane.
- Where include/gclm.h says the plane is read, it is read by every sweep from the first (a plane of ANOTHER field gives
  that field's solve bit for bit); where it says the plane is ignored, the radians are read."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, compare_result, result_spread

from geocalib_amd import _lib
from geocalib_amd.fields import pack_fields

pytestmark = pytest.mark.gpu

TOL = {"focal": 1e-4, "dist": 1e-4, "gravity": 1e-4, "cost": 1e-4, "cov": 1e-3, "unc": 1e-3}
MODELS = ("pinhole", "simple_radial", "radial", "simple_divisional")
STEPS = 10


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device("cuda:0")


def raw_heads(fields, seed):
    """Raw head outputs whose epilogue gives back (about) `fields`: what a CNN would hand gclm_pack_fields."""
    g = torch.Generator(device=fields["latitude_field"].device).manual_seed(seed)
    lat = fields["latitude_field"]
    scale = 0.5 + torch.rand(lat.shape, generator=g, device=lat.device)
    logit = lambda c: torch.log(c.clamp(1e-4, 1 - 1e-4) / (1 - c.clamp(1e-4, 1 - 1e-4)))  # noqa: E731
    return (fields["up_field"] * scale, torch.atanh(torch.sin(lat).clamp(-0.99, 0.99)),
            logit(fields["up_confidence"]), logit(fields["latitude_confidence"]))


@pytest.fixture(scope="module")
def packed(dev):
    """512 images of 640x480 (pinhole fields; every model solves them), packed with the sixth plane -- and a second
    latitude lat' with its own plane."""
    from geocalib_amd.synth import synth_fields
    f, _, _ = synth_fields("simple_radial", 512, 480, 640, dev, seed=11)
    f2, _, _ = synth_fields("simple_radial", 512, 480, 640, dev, seed=12)
    up_raw, lat_raw, ulc, llc = raw_heads(f, 1)
    del f
    out = pack_fields(up_raw, lat_raw, ulc, llc, inplace=True, sin_latitude=True)
    _, lat_raw2, _, _ = raw_heads(f2, 2)
    del f2
    other = pack_fields(out["up_field"], lat_raw2, sin_latitude=True)
    out["latitude_field2"], out["sin_latitude2"] = other["latitude_field"], other["sin_latitude"]
    torch.cuda.synchronize()
    return out


def bits(*ts):
    return torch.cat([t.reshape(-1).view(torch.int32) for t in ts])


def calibrate(model, up, lat, upc, latc, slat, *, slat_mode=-1, row_pairs=-1, fused=-1, group_size=0, steps=STEPS,
              early_stop=0):
    """One gclm_calibrate_ex on a fresh handle: (bits of cam, grav and all 48 info slots, scratch-plane bytes held)."""
    lib = _lib.load()
    B, _, H, W = lat.shape
    cfg = _lib.GclmConfig.default(0)
    cfg.camera_model = _lib.CAMERA_MODEL_IDS[model]
    cfg.num_steps, cfg.early_stop = steps, early_stop
    cfg.shared_intrinsics, cfg.group_size = int(group_size > 0), group_size
    h = C.c_void_p()
    _lib.check(lib.gclm_create(C.byref(h), C.byref(cfg)), None, "gclm_create")
    try:
        for fn, mode in ((lib.gclm_set_slat_plane, slat_mode), (lib.gclm_set_row_pairs, row_pairs),
                         (lib.gclm_set_fused_steps, fused)):
            _lib.check(fn(h, mode), h, "mode")
        cam = torch.empty((B, 8), device=lat.device)
        grav = torch.empty((B, 3), device=lat.device)
        info = torch.empty((B, _lib.INFO_STRIDE), device=lat.device)
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        _lib.check(lib.gclm_calibrate_ex(h, p(up), p(lat), p(upc), p(latc), B, H, W, None, None, None, None, 0,
                                         cam.data_ptr(), grav.data_ptr(), info.data_ptr(), p(slat),
                                         torch.cuda.current_stream().cuda_stream), h, "gclm_calibrate_ex")
        torch.cuda.synchronize()
        return bits(cam, grav, info), lib.gclm_slat_plane_bytes(h)
    finally:
        lib.gclm_destroy(h)


# ------------------------------------------------------------------ 1. the epilogue

@pytest.mark.parametrize("H,W", [(48, 640), (239, 318)])        # float4 path, scalar path (H * W % 4 != 0)
@pytest.mark.parametrize("confidences", [True, False])
def test_sixth_plane_is_sin_of_the_packed_latitude_and_the_five_planes_do_not_move(dev, H, W, confidences):
    g = torch.Generator(device=dev).manual_seed(H + W)
    B = 3
    up_raw = torch.randn(B, 2, H, W, device=dev, generator=g)
    lat_raw = 3 * torch.randn(B, 1, H, W, device=dev, generator=g)
    lat_raw[0, 0, :2] = torch.tensor([30.0, -30.0], device=dev)[:, None]          # saturated tanh: +-asin(1 - 1e-5)
    ulc = torch.randn(B, H, W, device=dev, generator=g) if confidences else None
    llc = torch.randn(B, 1, H, W, device=dev, generator=g) if confidences else None
    ref = pack_fields(up_raw, lat_raw, ulc, llc)
    ex = pack_fields(up_raw, lat_raw, ulc, llc, sin_latitude=True)
    inp = pack_fields(up_raw.clone(), lat_raw.clone(), None if ulc is None else ulc.clone(),
                      None if llc is None else llc.clone(), inplace=True, sin_latitude=True)
    torch.cuda.synchronize()
    assert set(ex) == set(ref) | {"sin_latitude"} and set(inp) == set(ex)
    for k in ref:
        assert torch.equal(bits(ex[k]), bits(ref[k])), k
        assert torch.equal(bits(inp[k]), bits(ref[k])), k
    assert torch.equal(bits(inp["sin_latitude"]), bits(ex["sin_latitude"]))
    s = ex["sin_latitude"]
    assert s.shape == (B, 1, H, W) and s.dtype == torch.float32
    err = (s.double() - torch.sin(ex["latitude_field"].double())).abs().max().item()
    print(f"sin_latitude {H}x{W} confidences={confidences}: max |plane - sin64(latitude_field)| = {err:.3e}")
    assert err <= 3e-7


# ------------------------------------------------------------------ 2.-4. bits, where the plane is read, no allocation

def _configs():
    c = []
    for m in MODELS:
        c.append((m, "one-row walk B=64", 64, {"row_pairs": 0}, m != "pinhole"))
    for m in ("radial", "simple_divisional"):
        c.append((m, "row pairs B=64", 64, {"row_pairs": 1}, True))
    for m in MODELS:
        c.append((m, "one launch per step B=1", 1, {"fused": 1}, True))
        c.append((m, "one launch per step B=4", 4, {"fused": 1}, True))
        c.append((m, "shared intrinsics, groups of 16", 32, {"group_size": 16}, m != "pinhole"))
    return c


@pytest.mark.parametrize("model,path,B,kw,read", _configs(), ids=lambda v: v if isinstance(v, str) else None)
def test_handed_plane_gives_the_same_bits_and_is_read_from_the_first_sweep(dev, packed, model, path, B, kw, read):
    d = {k: v[:B] for k, v in packed.items()}
    up, lat, upc, latc = d["up_field"], d["latitude_field"], d["up_confidence"], d["latitude_confidence"]
    handed, nbytes = calibrate(model, up, lat, upc, latc, d["sin_latitude"], **kw)
    library, _ = calibrate(model, up, lat, upc, latc, None, slat_mode=1, **kw)
    none, _ = calibrate(model, up, lat, upc, latc, None, slat_mode=0, **kw)
    assert torch.equal(handed, none), (model, path, "handed plane")
    assert torch.equal(library, none), (model, path, "library plane")
    if read:
        assert nbytes == 0, (model, path, nbytes)
    # a plane of ANOTHER latitude field: read from the first sweep on, or not at all
    mixed, _ = calibrate(model, up, lat, upc, latc, d["sin_latitude2"], **kw)
    other, _ = calibrate(model, up, d["latitude_field2"], upc, latc, d["sin_latitude2"], **kw)
    assert not torch.equal(other, none), "lat' must move the result"
    assert torch.equal(mixed, other if read else none), (model, path, read)


@pytest.mark.parametrize("model", ["simple_radial", "radial"])
@pytest.mark.parametrize("planes", ["scalar path", "no latitude confidence", "no confidences"])
def test_plane_is_ignored_where_the_sweep_reads_radians(dev, packed, model, planes):
    B = 8
    d = {k: v[:B] for k, v in packed.items()}
    if planes == "scalar path":           # 318 columns of the same images
        d = {k: v[..., :318].contiguous() for k, v in d.items()}
    up, lat, upc, latc = d["up_field"], d["latitude_field"], d["up_confidence"], d["latitude_confidence"]
    if planes != "scalar path":
        latc = None
        upc = None if planes == "no confidences" else upc
    base, _ = calibrate(model, up, lat, upc, latc, None, slat_mode=0)
    assert torch.equal(calibrate(model, up, lat, upc, latc, d["sin_latitude"])[0], base)
    assert torch.equal(calibrate(model, up, lat, upc, latc, d["sin_latitude2"])[0], base)
    # ... also a handed plane that is not 16-byte aligned while the fields are (the scalar path reads radians anyway)
    if planes == "no latitude confidence":
        mis = torch.empty(lat.numel() + 1, device=dev)[1:].view(lat.shape)
        mis.copy_(d["sin_latitude2"])
        full = {k: v for k, v in d.items()}
        assert torch.equal(calibrate(model, full["up_field"], lat, full["up_confidence"], full["latitude_confidence"], mis)[0],
                           calibrate(model, full["up_field"], lat, full["up_confidence"], full["latitude_confidence"], None,
                                     slat_mode=0)[0])


def test_no_scratch_plane_is_allocated_when_the_plane_is_handed(dev, packed):
    d = {k: v[:64] for k, v in packed.items()}
    args = (d["up_field"], d["latitude_field"], d["up_confidence"], d["latitude_confidence"])
    _, with_plane = calibrate("simple_radial", *args, d["sin_latitude"])
    _, without = calibrate("simple_radial", *args, None)
    assert with_plane == 0 and without == 64 * 480 * 640 * 4, (with_plane, without)


def test_overlapped_streams_carry_the_plane(dev, packed):
    from geocalib_amd import LMOptimizer

    def run(data, slat_mode=None):
        opt = LMOptimizer({"camera_model": "simple_radial", "num_steps": STEPS, "early_stop": False}).eval()
        opt.overlap_streams = 2
        if slat_mode is not None:
            opt(dict(data))
            for h in opt._handles.values():
                _lib.check(_lib.load().gclm_set_slat_plane(h.ptr, slat_mode), h.ptr, "gclm_set_slat_plane")
        out = opt(dict(data))
        torch.cuda.synchronize()
        return bits(out["camera"]._data, out["gravity"]._data, out["final_cost"], out["covariance"])

    base = {k: packed[k] for k in ("up_field", "latitude_field", "up_confidence", "latitude_confidence")}
    none = run(base, slat_mode=0)
    assert torch.equal(run(base), none)                                           # the library's plane (built-in)
    assert torch.equal(run({**base, "sin_latitude": packed["sin_latitude"]}), none)
    other = run({**base, "latitude_field": packed["latitude_field2"], "sin_latitude": packed["sin_latitude2"]})
    assert not torch.equal(other, none)
    assert torch.equal(run({**base, "sin_latitude": packed["sin_latitude2"]}), other)


# ------------------------------------------------------------------ 5. a caller's own torch.sin against the goldens

def _run_with_torch_sin(data, model, dev):
    from geocalib_amd import LMOptimizer
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in data.items()}
    d["sin_latitude"] = torch.sin(d["latitude_field"])
    out = LMOptimizer({"camera_model": model, "num_steps": 20, "early_stop": False}).eval()(d)
    torch.cuda.synchronize()
    return {k: (v._data if hasattr(v, "_data") else v).detach().cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("model", ["pinhole", "simple_radial"])
def test_torch_sin_plane_matches_reference_full_size(dev, model):
    from oracle import synth
    full = np.load(os.path.join(GOLDEN, "golden_full.npz"))
    data, _, _ = synth.make_fields(1234, range(4), model, 480, 640)
    out = _run_with_torch_sin(data, model, dev)
    ref = {k.split("/", 1)[1]: full[k] for k in full.files if k.startswith(model + "/")}
    compare_result(out, ref, TOL)
    assert np.array_equal(out["stop_at"], ref["stop_at"])


@pytest.mark.parametrize("model,idx", [("radial", (0, 1)), ("simple_divisional", (2, 5))])
def test_torch_sin_plane_matches_reference_full_size_other_models(dev, model, idx):
    from oracle import synth
    g = np.load(os.path.join(GOLDEN, "golden_full_rd.npz"))
    data, _, _ = synth.make_fields(1234, idx, model, 480, 640)
    out = _run_with_torch_sin(data, model, dev)
    ref = {k.split("/", 1)[1]: g[k] for k in g.files if k.startswith(model + "/")}
    d = result_spread(out, ref)
    assert (d < 1e-4 + 10.0 * ref["spread"]).all(), (model, d, ref["spread"])
    assert np.isin(out["stop_at"], ref["stop_at_set"]).all()
    assert np.abs(out["covariance"] - ref["covariance"]).max() / np.abs(ref["covariance"]).max() < 1e-3


# ------------------------------------------------------------------ 6. end to end

@pytest.mark.parametrize("model", MODELS)
def test_geocalib_calibrate_with_the_handoff_is_bit_identical(dev, model):
    from geocalib_amd import GeoCalib

    def field_model(handoff):
        def run(img_data):
            img = img_data["image"]
            B, _, h, w = img.shape
            g = torch.Generator(device=img.device).manual_seed(7)
            yy = torch.linspace(-0.6, 0.4, h, device=img.device)[:, None].expand(h, w)
            up_raw = torch.stack([0.1 + 0.05 * torch.randn(B, h, w, device=img.device, generator=g),
                                  -torch.ones(B, h, w, device=img.device)], 1)
            lat_raw = (-1.5 * yy + 0.02 * torch.randn(B, h, w, device=img.device, generator=g))[:, None]
            conf = torch.randn(B, 1, h, w, device=img.device, generator=g)
            return pack_fields(up_raw, lat_raw, conf, conf, sin_latitude=handoff)
        return run

    img = torch.rand(3, 400, 560, device=dev)
    a = GeoCalib(field_model(False)).calibrate(img, camera_model=model)
    b = GeoCalib(field_model(True)).calibrate(img, camera_model=model)
    torch.cuda.synchronize()
    assert set(a) == set(b) and "sin_latitude" not in b
    assert b["latitude_field"].shape[-2:] == (400, 560)
    for k in a:
        va, vb = (a[k]._data, b[k]._data) if hasattr(a[k], "_data") else (a[k], b[k])
        assert torch.equal(bits(va.float()), bits(vb.float())), k
