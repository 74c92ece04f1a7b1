"""GPU: the classification-head epilogue (gclm_pack_fields_bins behind fields.pack_fields_from_logits) against the CPU torch
composition of the same tensors moved to the host.  Both gather from the same tables, so up and latitude are compared with
torch.equal -- no tolerance anywhere -- on both paths of the kernel (16-byte loads, one pixel per lane), the three logit
types, the bin counts 73 / 180, 5 / 7 and 2 / 1, with every planted pixel of tests/bins_gate.py in every lane slot.  The
confidences are gclm_pack_fields' bits, the sixth plane gives the bits of a solve without it, and an image past element 2^31
decodes like the first."""
import math

import pytest
import torch

import bins_gate as bg
from geocalib_amd import _call, _lib, perspective_encoding as pe
from geocalib_amd.fields import pack_fields, pack_fields_from_logits

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
BINS = [(73, 180), (5, 7), (2, 1)]                 # the reference's heads; a tiny pair; the smallest legal counts
# (B, h, w, misaligned): 16-byte loads; an odd pixel count (one pixel per lane); the first shape 4 bytes off alignment (one
# pixel per lane by misalignment); several workgroups per image
SHAPES = [(2, 6, 8, False), (2, 5, 7, False), (2, 6, 8, True), (3, 40, 52, False)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32)


def to_device(t, dev, misaligned=False):
    """`t` on the device, contiguous; `misaligned`: starting 4 bytes behind a 16-byte boundary."""
    if not misaligned:
        return t.to(dev)
    off = 4 // t.element_size()
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=dev)
    out = buf[off:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


def run_both(dev, up_logits, lat_logits, ulc=None, llc=None, misaligned=False, sin_latitude=True):
    want = pack_fields_from_logits(up_logits, lat_logits, ulc, llc, sin_latitude=sin_latitude)
    got = pack_fields_from_logits(to_device(up_logits, dev, misaligned), to_device(lat_logits, dev, misaligned),
                                  None if ulc is None else ulc.to(dev), None if llc is None else llc.to(dev), sin_latitude=sin_latitude)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in got.items()}, want


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("Ku,Kl", BINS, ids=["73-180", "5-7", "2-1"])
@pytest.mark.parametrize("B,h,w,misaligned", SHAPES, ids=["6x8", "5x7", "6x8-misaligned", "3x40x52"])
def test_fields_equal_the_cpu_composition_bit_for_bit(dev, B, h, w, misaligned, Ku, Kl, dtype):
    up_logits, lat_logits, where = bg.head_logits(B, Ku, Kl, h, w, seed=h * w + Ku, dtype=dtype)
    if h * w % 8 == 0:          # every kind in every lane slot of a vector unit (pixel index mod 8, hence mod 4)
        kinds = torch.cat([torch.roll(torch.arange(8), r) for r in range(8)]).tolist()
        assert len(where) == 64 and {(k, px % 8) for k, (_, px) in zip(kinds, where)} == {(k, s) for k in range(8) for s in range(8)}
    g = torch.Generator().manual_seed(B + w)
    ulc, llc = 3 * torch.randn(B, h, w, generator=g), 3 * torch.randn(B, 1, h, w, generator=g)
    got, want = run_both(dev, up_logits, lat_logits, ulc, llc, misaligned)
    assert list(got) == list(want) and all(got[k].shape == want[k].shape and got[k].dtype == torch.float32 for k in want)
    assert torch.equal(bits(got["up_field"]), bits(want["up_field"]))
    assert torch.equal(bits(got["latitude_field"]), bits(want["latitude_field"]))
    # the planted pixels decode to what their kind says (the CPU composition is held to the reference in test_pack_bins_abi.py)
    flat = got["up_field"].view(B, 2, h * w)
    assert all((flat[b, :, px] == 0).all() == (int(up_logits[b, :, px // w, px % w].float().argmax()) == Ku - 1) for b, px in where)
    # the sixth plane: the sweep's polynomial of the latitude just written, held to the bound gclm_pack_fields_ex's plane is
    # held to (tests/test_sin_latitude_handoff.py); what it guarantees is the solve's bits, checked below
    err = (got["sin_latitude"].double() - torch.sin(got["latitude_field"].double())).abs().max().item()
    assert err <= 3e-7, err
    # the confidences: gclm_pack_fields' bits on the same log-confidences
    ref = pack_fields(torch.zeros(B, 2, h, w, device=dev), torch.zeros(B, 1, h, w, device=dev), ulc.to(dev), llc.to(dev))
    assert torch.equal(bits(got["up_confidence"]), bits(ref["up_confidence"].cpu()))
    assert torch.equal(bits(got["latitude_confidence"]), bits(ref["latitude_confidence"].cpu()))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_outputs_do_not_depend_on_the_path(dev, dtype):
    """The same 6 x 8 data through the 16-byte loads and, 4 bytes off alignment, through one pixel per lane."""
    up_logits, lat_logits, _ = bg.head_logits(2, 73, 180, 6, 8, seed=77, dtype=dtype)
    g = torch.Generator().manual_seed(78)
    ulc, llc = torch.randn(2, 6, 8, generator=g), torch.randn(2, 6, 8, generator=g)
    a, _ = run_both(dev, up_logits, lat_logits, ulc, llc, misaligned=False)
    b, _ = run_both(dev, up_logits, lat_logits, ulc, llc, misaligned=True)
    assert len(a) == 5 and all(torch.equal(bits(a[k]), bits(b[k])) for k in a)


def test_without_confidences_and_sixth_plane_only_the_fields_are_written(dev):
    up_logits, lat_logits, _ = bg.head_logits(2, 73, 180, 6, 8, seed=5)
    got, want = run_both(dev, up_logits, lat_logits, sin_latitude=False)
    assert list(got) == ["up_field", "latitude_field"]
    assert torch.equal(bits(got["up_field"]), bits(want["up_field"])) and torch.equal(bits(got["latitude_field"]), bits(want["latitude_field"]))
    only_lat, _ = run_both(dev, up_logits, lat_logits, None, torch.zeros(2, 6, 8), sin_latitude=False)
    assert list(only_lat) == ["up_field", "latitude_field", "latitude_confidence"] and (only_lat["latitude_confidence"] == 0.5).all()


@pytest.mark.parametrize("h,w", [(6, 8), (5, 7)], ids=["6x8", "5x7"])
def test_a_log_confidence_is_converted_in_place(dev, h, w):
    """The C entry with each confidence output on its log-confidence: the bits of the out-of-place call."""
    B, Ku, Kl = 2, 73, 180
    up_logits, lat_logits, _ = bg.head_logits(B, Ku, Kl, h, w, seed=11, dtype=torch.bfloat16)
    g = torch.Generator().manual_seed(12)
    ulc, llc = 3 * torch.randn(B, h, w, generator=g), 3 * torch.randn(B, h, w, generator=g)
    want = pack_fields_from_logits(up_logits.to(dev), lat_logits.to(dev), ulc.to(dev), llc.to(dev))
    ul, ll, uc, lc = up_logits.to(dev), lat_logits.to(dev), ulc.to(dev), llc.to(dev)
    up, lat = torch.empty(B, 2, h, w, device=dev), torch.empty(B, 1, h, w, device=dev)
    _call.call("gclm_pack_fields_bins", ul.data_ptr(), Ku, ll.data_ptr(), Kl, _lib.LOGIT_DTYPE_IDS["bfloat16"],
               pe.up_bin_table(Ku, dev).data_ptr(), pe.latitude_bin_table(Kl, dev).data_ptr(), uc.data_ptr(), lc.data_ptr(), B, h, w,
               up.data_ptr(), uc.data_ptr(), lat.data_ptr(), lc.data_ptr(), None, _call.raw_stream(dev), device=dev)
    torch.cuda.synchronize()
    for got, key in ((up, "up_field"), (lat, "latitude_field"), (uc, "up_confidence"), (lc, "latitude_confidence")):
        assert torch.equal(bits(got), bits(want[key])), key


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_more_images_than_rows_of_the_grid(dev, dtype):
    """4100 images of 8 x 8: the launch has 4096 rows of workgroups, so the image loop makes a second trip."""
    up_logits, lat_logits, _ = bg.head_logits(4100, 5, 7, 8, 8, seed=3, dtype=dtype)
    got, want = run_both(dev, up_logits, lat_logits, sin_latitude=False)
    assert torch.equal(bits(got["up_field"]), bits(want["up_field"]))
    assert torch.equal(bits(got["latitude_field"]), bits(want["latitude_field"]))


def test_an_image_past_element_2_to_the_31_decodes_like_the_first(dev):
    """80 images of 180 latitude classes at 320 x 480 in bfloat16 are 2.21e9 logits (4.4 GB): the last image starts past
    element 2^31.  All logits are zero but for the first and the last image, which hold the same seeded planes."""
    B, Ku, Kl, h, w = 80, 2, 180, 320, 480
    assert (B - 1) * Kl * h * w > 2 ** 31
    g = torch.Generator().manual_seed(41)
    up_one = torch.randn(1, Ku, h, w, generator=g).bfloat16()
    lat_one = torch.randn(1, Kl, h, w, generator=g).bfloat16()
    want = pack_fields_from_logits(up_one, lat_one)
    up_logits = torch.zeros(B, Ku, h, w, dtype=torch.bfloat16, device=dev)
    lat_logits = torch.zeros(B, Kl, h, w, dtype=torch.bfloat16, device=dev)
    for b in (0, B - 1):
        up_logits[b], lat_logits[b] = up_one[0].to(dev), lat_one[0].to(dev)
    got = pack_fields_from_logits(up_logits, lat_logits)
    torch.cuda.synchronize()
    for b in (0, B - 1):
        assert torch.equal(bits(got["up_field"][b].cpu()), bits(want["up_field"][0])), b
        assert torch.equal(bits(got["latitude_field"][b].cpu()), bits(want["latitude_field"][0])), b
    # every other image: bin 0 of both heads
    assert (got["up_field"][1:B - 1] == pe.up_bin_table(Ku, dev)[0].view(1, 2, 1, 1)).all()
    assert (got["latitude_field"][1:B - 1] == pe.latitude_bin_table(Kl, dev)[0]).all()


@pytest.mark.parametrize("model", ["pinhole", "simple_radial"])
def test_a_solve_with_the_sixth_plane_gives_the_bits_of_a_solve_without_it(dev, model):
    """Ground-truth fields of two pinhole calibrations at 24 x 32 -> bins -> one-hot logits -> the epilogue with the sixth
    plane -> LMOptimizer, 5 steps: camera, gravity and costs equal the solve that reads the radians.  The decoded latitude lies
    within half a class of the rendered one: the quantisation's own bound."""
    from geocalib_amd import Gravity, LMOptimizer, camera_models
    from geocalib_amd import perspective_fields as pf
    B, h, w, Ku, Kl = 2, 24, 32, 73, 180
    cam = camera_models["pinhole"].from_dict({"height": torch.full((B,), float(h)), "width": torch.full((B,), float(w)),
                                              "vfov": torch.tensor([math.radians(50), math.radians(75)])})
    grav = Gravity.from_rp(torch.tensor([0.15, -0.3]), torch.tensor([0.2, -0.1]))
    up, lat = pf.get_perspective_field(cam, grav)                   # CPU: the torch composition
    up_bins = torch.stack([pe.encode_up_bin(up[b], Ku) for b in range(B)])
    lat_bins = pe.encode_bin_latitude(lat[:, 0], Kl)
    one_hot = lambda bins, K: torch.nn.functional.one_hot(bins, K).permute(0, 3, 1, 2).float().contiguous()  # noqa: E731
    data = pack_fields_from_logits(one_hot(up_bins, Ku).to(dev), one_hot(lat_bins, Kl).to(dev), sin_latitude=True)
    torch.cuda.synchronize()
    half_class = math.radians(0.5)
    worst = (data["latitude_field"].cpu() - lat).abs().max().item()
    assert worst <= half_class * (1 + 1e-6) + 2.0 ** -23, worst     # (float32 roundings of the edges, the centre and the field)
    assert torch.equal(data["up_field"].cpu(), pe.decode_up_bin(up_bins, Ku))

    def solve(d):
        out = LMOptimizer({"camera_model": model, "num_steps": 5, "early_stop": False}).eval()(d)
        torch.cuda.synchronize()
        return out
    with_plane = solve(dict(data))
    without = solve({k: v for k, v in data.items() if k != "sin_latitude"})
    for key in ("initial_cost", "final_cost", "initial_latitude_cost", "final_latitude_cost"):
        assert torch.equal(bits(with_plane[key].float()), bits(without[key].float())), key
    assert torch.equal(bits(with_plane["camera"]._data), bits(without["camera"]._data))
    assert torch.equal(bits(with_plane["gravity"]._data), bits(without["gravity"]._data))
    assert torch.isfinite(with_plane["final_cost"]).all()
