"""CPU: the classification-head epilogue without a device -- perspective_encoding against the reference's recorded results
(tests/golden/bins_reference.npz, written by tests/golden/make_golden_bins.py), bit for bit; the round trip of every bin; the
torch composition of fields.pack_fields_from_logits on CPU tensors, planted pixels included; gclm_pack_fields_bins declared,
exported, bound and documented; every invalid argument refused before any HIP call, and the legal neighbours reaching the
launch; the ValueErrors of the Python call."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from geocalib_amd import _lib, perspective_encoding as pe
from geocalib_amd.fields import pack_fields_from_logits
from abi_harness import assert_declared_exported_and_bound
import bins_gate as bg

ARGS = ["const void*", "int", "const void*", "int", "int", "const float*", "const float*", "const float*", "const float*", "int",
        "int", "int", "float*", "float*", "float*", "float*", "float*", "void*"]
CASES = {"": (73, 180), "tiny_": (5, 7)}


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "bins_reference.npz"))
    return {k: z[k] if z[k].dtype.kind == "U" else torch.from_numpy(z[k]) for k in z.files}


def same_bits(a, b):
    return a.dtype == b.dtype == torch.float32 and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------ the definition against the reference
@pytest.mark.parametrize("prefix", CASES, ids=["73-180", "5-7"])
def test_cpu_composition_equals_the_reference_bit_for_bit(golden, prefix):
    Ku, Kl = CASES[prefix]
    up_logits, lat_logits = golden[prefix + "up_logits"], golden[prefix + "lat_logits"]
    assert up_logits.shape == (2, Ku, 5, 7) and lat_logits.shape == (2, Kl, 5, 7)
    out = pack_fields_from_logits(up_logits, lat_logits)
    assert set(out) == {"up_field", "latitude_field"}
    assert same_bits(out["up_field"], golden[prefix + "up_field"])
    assert same_bits(out["latitude_field"], golden[prefix + "latitude"][:, None])
    # the planted pixels are where the fixture says, and hold what the reference gave for the vectors alone
    where = golden[prefix + "planted_at"].tolist()
    assert len(where) == 16 and tuple(golden["kinds"]) == bg.KINDS
    kinds = torch.cat([torch.roll(torch.arange(8), r) for r in range(2)])
    for (b, px), kind in zip(where, kinds.tolist()):
        y, x = divmod(px, 7)
        assert torch.equal(up_logits[b, :, y, x].view(torch.int32), golden[prefix + "planted_up"][kind].view(torch.int32))
        assert same_bits(out["up_field"][b, :, y, x], golden[prefix + "planted_up_field"][kind]), bg.KINDS[kind]
    # ... and every kind alone, both heads
    alone = pack_fields_from_logits(golden[prefix + "planted_up"][:, :, None, None].contiguous(),
                                    golden[prefix + "planted_lat"][:, :, None, None].contiguous())
    assert same_bits(alone["up_field"][:, :, 0, 0], golden[prefix + "planted_up_field"])
    assert same_bits(alone["latitude_field"][:, 0, 0, 0], golden[prefix + "planted_latitude"])


def test_the_planted_pixels_decide_what_they_are_named_for(golden):
    """The argmax rule on the planted vectors, stated on its own: first of the ties, NaN above everything and the first NaN,
    all -inf gives 0 -- and the last up channel is the invalid class, (0, 0)."""
    for K in (73, 180, 7, 5, 2, 1):
        v, p = bg.planted(K, 3), bg.picks(K)
        a, c = p[0], p[-1]
        want = [a, p[0], 0, K - 1, a, p[len(p) // 2] if K >= 3 else a, 0, a]
        assert v.argmax(1).tolist() == want, K
        assert torch.equal(v.bfloat16().float().nan_to_num(7.0), v.nan_to_num(7.0))
        assert torch.equal(v.half().float().nan_to_num(7.0), v.nan_to_num(7.0))
    assert golden["planted_up_field"][3].tolist() == [0.0, 0.0]


@pytest.mark.parametrize("prefix", CASES, ids=["73-180", "5-7"])
def test_decodes_and_encoders_equal_the_reference_exactly(golden, prefix):
    Ku, Kl = CASES[prefix]
    up_logits, lat_logits = golden[prefix + "up_logits"], golden[prefix + "lat_logits"]
    assert same_bits(pe.decode_up_bin(up_logits.argmax(1), Ku), golden[prefix + "up_field"])
    assert same_bits(pe.decode_bin_latitude(lat_logits.argmax(1), Kl), golden[prefix + "latitude"])
    bins = pe.encode_up_bin(golden[prefix + "enc_up_in"], Ku)
    assert bins.dtype == torch.long and torch.equal(bins, golden[prefix + "enc_up_bins"].long())
    assert int(bins.max()) == Ku - 1 and int(bins.min()) == 0
    bins = pe.encode_bin_latitude(golden[prefix + "enc_lat_in"], Kl)
    assert bins.dtype == torch.long and torch.equal(bins, golden[prefix + "enc_lat_bins"].long())
    assert set(bins.tolist()) == set(range(Kl))


@pytest.mark.parametrize("Ku,Kl", [(73, 180), (5, 7)])
def test_round_trip_of_every_bin(Ku, Kl):
    k = torch.arange(Ku)
    up = pe.decode_up_bin(k.view(1, 1, Ku), Ku)                      # (1, 2, 1, Ku)
    assert torch.equal(pe.encode_up_bin(up[0], Ku), k.view(1, Ku))   # the invalid bin included
    assert up[0, :, 0, Ku - 1].tolist() == [0.0, 0.0]
    k = torch.arange(Kl)
    assert torch.equal(pe.encode_bin_latitude(pe.decode_bin_latitude(k, Kl), Kl), k)


def test_tables_are_the_decodes_and_are_cached():
    t = pe.up_bin_table(73)
    assert t.shape == (73, 2) and t.dtype == torch.float32 and pe.up_bin_table(73, "cpu") is t and t[72].tolist() == [0.0, 0.0]
    assert same_bits(t.t().reshape(1, 2, 1, 73).contiguous(), pe.decode_up_bin(torch.arange(73).view(1, 1, 73), 73))
    lt = pe.latitude_bin_table(180)
    assert lt.shape == (180,) and lt.dtype == torch.float32 and pe.latitude_bin_table(180) is lt
    assert lt.abs().max().item() < math.pi / 2 and abs(lt[0].item() + math.radians(89.5)) < 1e-6
    n = next(n for n in range(2, 400) if torch.arange(-90, 90, 180 / n).numel() != n)      # a step that is not exact
    with pytest.raises(ValueError):
        pe.latitude_bin_table(n)
    with pytest.raises(ValueError):
        pe.up_bin_table(1)


# ------------------------------------------------------------------ the entry point
def test_entry_point_is_declared_exported_bound_and_documented():
    args = assert_declared_exported_and_bound("gclm_pack_fields_bins", ARGS)
    assert len(args) == 18 and [a for a in args if a is C.c_int] == [C.c_int] * 6
    header = open(os.path.join(ROOT, "include", "gclm.h")).read()
    assert "gclm_pack_fields_bins added, also within 610" in header[header.index("ABI version:"):header.index("#define GCLM_VERSION")]
    assert "enum gclm_logit_dtype { GCLM_LOGITS_F32 = 0, GCLM_LOGITS_F16 = 1, GCLM_LOGITS_BF16 = 2 }" in header
    assert _lib.LOGIT_DTYPE_IDS == {"float32": 0, "float16": 1, "bfloat16": 2}
    assert f"#define GCLM_MAX_BINS {_lib.MAX_BINS}" in header
    assert "| `gclm_pack_fields_bins` |" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


# fake, never dereferenced device addresses: every call below must be refused before the first HIP call
UPL, LATL, UPT, LATT, ULC, LLC, UP, UPC, LAT, LATC, SLAT = (0x1000000, 0x2000000, 0x3000000, 0x3100000, 0x4000000, 0x4100000,
                                                            0x5000000, 0x5100000, 0x5200000, 0x5300000, 0x5400000)
OK = dict(upl=UPL, Ku=73, latl=LATL, Kl=180, dt=0, upt=UPT, latt=LATT, ulc=ULC, llc=LLC, B=2, H=6, W=8, up=UP, upc=UPC, lat=LAT,
          latc=LATC, slat=SLAT)
PX = 2 * 6 * 8 * 4                       # bytes of a (B, h, w) float plane
BAD = [("NULL up logits", dict(upl=None)), ("NULL latitude logits", dict(latl=None)), ("NULL up table", dict(upt=None)),
       ("NULL latitude table", dict(latt=None)), ("NULL up output", dict(up=None)), ("NULL latitude output", dict(lat=None)),
       ("one up bin", dict(Ku=1)), ("no up bin", dict(Ku=0)), ("2049 up bins", dict(Ku=2049)), ("no latitude bin", dict(Kl=0)),
       ("negative latitude bins", dict(Kl=-5)), ("2049 latitude bins", dict(Kl=2049)), ("dtype 3", dict(dt=3)),
       ("dtype -1", dict(dt=-1)), ("H = 0", dict(H=0)), ("W = 0", dict(W=0)), ("H < 0", dict(H=-6)), ("B < 0", dict(B=-1)),
       ("up log-confidence without its output", dict(upc=None)), ("latitude log-confidence without its output", dict(latc=None)),
       ("up output starts at the up logits' last byte", dict(up=UPL + 73 * PX - 4)),
       ("up output ends one float inside the latitude logits", dict(up=LATL - 2 * PX + 4)),
       ("latitude output on the latitude logits", dict(lat=LATL)),
       ("latitude output starts at the up table's last float", dict(lat=UPT + 73 * 8 - 4)),
       ("up confidence on the latitude table", dict(upc=LATT)),
       ("latitude confidence ends one float inside the up logits", dict(latc=UPL - PX + 4)),
       ("up confidence one float off its log-confidence", dict(upc=ULC + 4)),
       ("latitude confidence on the up log-confidence", dict(latc=ULC)),
       ("up output on the latitude output", dict(up=LAT - PX)),
       ("sin(latitude) on the latitude output", dict(slat=LAT)), ("sin(latitude) on the up output's second plane", dict(slat=UP + PX)),
       ("sin(latitude) on the up log-confidence", dict(slat=ULC)), ("sin(latitude) on the latitude confidence", dict(slat=LATC)),
       ("sin(latitude) ends one float inside the latitude logits", dict(slat=LATL - PX + 4)),
       ("sin(latitude) on the latitude table's last float", dict(slat=LATT + 179 * 4)),
       ("half logits off a 2-byte boundary", dict(dt=1, upl=UPL + 1)), ("float logits off a 4-byte boundary", dict(latl=LATL + 2)),
       ("output off a 4-byte boundary", dict(lat=LAT + 2)), ("table off a 4-byte boundary", dict(upt=UPT + 1))]
NEIGHBOURS = [dict(), dict(dt=1), dict(dt=2), dict(Ku=2, Kl=1), dict(Ku=2048, Kl=2048), dict(H=1, W=1), dict(H=5, W=7),
              dict(ulc=None, upc=None), dict(llc=None, latc=None), dict(ulc=None, llc=None, upc=None, latc=None, slat=None),
              dict(ulc=None), dict(upc=ULC), dict(latc=LLC), dict(upc=ULC, latc=LLC, slat=None),      # in place
              dict(up=UPL + 73 * PX), dict(up=LATL - 2 * PX), dict(lat=UPT + 73 * 8), dict(slat=LATT + 180 * 4),
              dict(dt=2, upl=UPL + 2, latl=LATL + 6), dict(up=UP + 4, slat=SLAT + 12)]


def _call(a):
    return _lib.load().gclm_pack_fields_bins(a["upl"], a["Ku"], a["latl"], a["Kl"], a["dt"], a["upt"], a["latt"], a["ulc"], a["llc"],
                                             a["B"], a["H"], a["W"], a["up"], a["upc"], a["lat"], a["latc"], a["slat"], None)


@pytest.mark.parametrize("what,change", BAD, ids=[b[0] for b in BAD])
def test_refuses_invalid_arguments_before_any_hip_call(what, change):
    assert set(change) <= set(OK) and 1 <= len(change) <= 2
    assert _call({**OK, **change}) == -3, what


def test_an_empty_batch_succeeds_and_launches_nothing():
    assert _call({**OK, "B": 0}) == 0


def test_the_valid_neighbours_reach_the_launch():
    """The neighbours of the refused calls -- ranges that only touch, the extreme bin counts, every dtype, absent confidences, a
    log-confidence converted in place -- are valid and reach the launch, which fails without a device: -10."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: a valid call would launch on fake addresses")
    for change in NEIGHBOURS:
        assert _call({**OK, **change}) == -10, change


# ------------------------------------------------------------------ the Python call
def test_python_call_refuses_what_it_cannot_serve():
    up, lat = torch.zeros(2, 73, 5, 7), torch.zeros(2, 180, 5, 7)
    for bad_up, bad_lat, why in [(up[0], lat, "rank"), (up, lat[0], "rank"), (up, lat[:1], "B"), (up, lat[..., :6], "w"),
                                 (up, lat[:, :, :4], "h"), (up.half(), lat, "mixed dtypes"), (up.double(), lat.double(), "float64"),
                                 (up.long(), lat.long(), "integers"), (up[:, ::2], lat, "non-contiguous up logits"),
                                 (up, lat.transpose(2, 3).contiguous().transpose(2, 3), "non-contiguous latitude logits"),
                                 (up.contiguous(memory_format=torch.channels_last), lat, "channels_last"),
                                 (up[:, :1], lat, "one up bin")]:
        with pytest.raises(ValueError):
            pack_fields_from_logits(bad_up, bad_lat)
            pytest.fail(why)
    with pytest.raises(ValueError):
        pack_fields_from_logits(up, lat, up_log_confidence=torch.zeros(2, 5, 6))
    with pytest.raises(ValueError):
        pack_fields_from_logits(up, lat, lat_log_confidence=torch.zeros(1, 5, 7))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=str)
def test_python_call_on_cpu_tensors_returns_the_dict_of_pack_fields(dtype):
    up_logits, lat_logits, _ = bg.head_logits(2, 73, 180, 5, 7, seed=5, dtype=dtype)
    g = torch.Generator().manual_seed(9)
    ulc, llc = torch.randn(2, 5, 7, generator=g), torch.randn(2, 1, 5, 7, generator=g)
    out = pack_fields_from_logits(up_logits, lat_logits, ulc, llc, sin_latitude=True)
    assert list(out) == ["up_field", "latitude_field", "up_confidence", "latitude_confidence", "sin_latitude"]
    assert all(v.dtype == torch.float32 for v in out.values())
    assert out["up_field"].shape == (2, 2, 5, 7) and out["latitude_field"].shape == out["sin_latitude"].shape == (2, 1, 5, 7)
    assert out["up_confidence"].shape == out["latitude_confidence"].shape == (2, 5, 7)
    # 16-bit logits are compared as the floats they widen to
    wide = pack_fields_from_logits(up_logits.float(), lat_logits.float())
    assert same_bits(out["up_field"], wide["up_field"]) and same_bits(out["latitude_field"], wide["latitude_field"])
    assert torch.equal(out["up_confidence"], torch.sigmoid(ulc)) and torch.equal(out["latitude_confidence"], torch.sigmoid(llc[:, 0]))
    assert torch.equal(out["sin_latitude"], torch.sin(out["latitude_field"]))
