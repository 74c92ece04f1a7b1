"""CPU: gclm_hypothesis_scores without a device -- the entry points are declared, exported and bound, every invalid argument
is refused before any HIP call, the workspace size is monotone, fields.hypothesis_scores hands the C entry the arguments of
include/gclm.h, metrics.rank_calibrations takes the torch path off the device and agrees there with the float64 yardstick,
the gate of tests/hypothesis_gate.py is not vacuous, passes an honest float32 restatement of the kernel and fails its
mutants, and the kernels carry no scratch."""
import ctypes as C
import math
import os

import pytest
import torch

from geocalib_amd import Gravity, _call, _lib, camera_models, fields, metrics
from abi_harness import HEADER, LLVM, assert_declared_exported_and_bound
import field_error_gate as fg
import hypothesis_gate as hg
from test_host_calls import MAX, STREAM, p, rec  # noqa: F401  (the recorder fixture, not edited)

ARGS = ["int", "const float*", "const float*", "int", "int", "int", "int", "const float*", "const float*", "const float*",
        "const float*", "const float*", "float", "float", "float", "float", "void*", "size_t", "float*", "int*", "void*"]


def test_entry_points_are_declared_exported_and_bound():
    args = assert_declared_exported_and_bound("gclm_hypothesis_scores", ARGS)
    for a, t in zip(args, ARGS):
        assert t in ("int", "size_t") or a is (C.c_float if t == "float" else C.c_void_p), (a, t)
    assert assert_declared_exported_and_bound("gclm_hypothesis_scores_workspace", ["int"] * 4, ret="size_t") == [C.c_int] * 4
    header = open(HEADER).read()
    changelog = header[header.index("ABI version:"):header.index("#define GCLM_VERSION")]
    assert "gclm_hypothesis_scores_workspace" in changelog and "gclm_hypothesis_scores " in changelog
    assert f"#define GCLM_HYPOTHESIS_CHUNK {fields.HYPOTHESIS_CHUNK} " in header and fields.HYPOTHESIS_CHUNK == _lib.HYPOTHESIS_CHUNK


# fake, never dereferenced device addresses: every call below must be refused before the first HIP call
CAM, GRAV, UP, LAT, UPC, LATC, MASK = 0x100000, 0x200000, 0x4000000, 0x8000000, 0xC000000, 0x10000000, 0x14000000
WS, SCORES, BEST = 0x20000000, 0x30000000, 0x40000000
PX_BYTES = 2 * 48 * 64 * 4
OK = dict(model=1, cam=CAM, grav=GRAV, B=2, N=7, H=48, W=64, up=UP, lat=LAT, upc=UPC, latc=LATC, mask=MASK, tu=1.0, tl=1.0, wu=1.0,
          wl=1.0, ws=WS, ws_bytes=1 << 24, scores=SCORES, best=BEST)
BAD = [("NULL camera", dict(cam=None)), ("NULL gravity", dict(grav=None)), ("NULL scores", dict(scores=None)),
       ("NULL workspace", dict(ws=None)), ("both fields NULL", dict(up=None, lat=None, upc=None, latc=None)),
       ("up confidence without up", dict(up=None)), ("latitude confidence without latitude", dict(lat=None)),
       ("B = 0", dict(B=0)), ("B > 65535", dict(B=65536, ws_bytes=1 << 62)), ("N = 0", dict(N=0)),
       ("N > 65535", dict(N=65536, ws_bytes=1 << 62)), ("H = 0", dict(H=0)), ("W = 0", dict(W=0)),
       ("H * W > 2^31 - 1", dict(H=65536, W=32768, ws_bytes=1 << 62)),
       ("tile grid over 2^32 threads", dict(H=2 ** 31 - 1, W=1, ws_bytes=1 << 62)),
       ("model -1", dict(model=-1)), ("model 4", dict(model=4)),
       ("NaN up threshold", dict(tu=math.nan)), ("infinite latitude threshold", dict(tl=math.inf)),
       ("infinite up weight", dict(wu=-math.inf)), ("NaN latitude weight", dict(wl=math.nan)),
       ("workspace too small", dict(ws_bytes=1000)),
       ("camera misaligned", dict(cam=CAM + 2)), ("gravity misaligned", dict(grav=GRAV + 1)), ("up misaligned", dict(up=UP + 1)),
       ("latitude misaligned", dict(lat=LAT + 2)), ("up confidence misaligned", dict(upc=UPC + 3)),
       ("latitude confidence misaligned", dict(latc=LATC + 2)), ("mask misaligned", dict(mask=MASK + 2)),
       ("scores misaligned", dict(scores=SCORES + 2)), ("best misaligned", dict(best=BEST + 1)), ("workspace misaligned", dict(ws=WS + 1)),
       ("scores overlap the cameras", dict(scores=CAM + 2 * 7 * 32 - 4)), ("scores overlap the gravities", dict(scores=GRAV - 8)),
       ("scores overlap up", dict(scores=UP + 2 * PX_BYTES - 4)), ("scores overlap the mask", dict(scores=MASK)),
       ("best overlaps the latitude confidence", dict(best=LATC + PX_BYTES - 4)), ("best overlaps scores", dict(best=SCORES + 2 * 7 * 12 - 4)),
       ("workspace overlaps the up confidence", dict(ws=UPC + PX_BYTES - 4)), ("workspace overlaps scores", dict(ws=SCORES - 4)),
       ("workspace overlaps best", dict(best=WS + 8)), ("workspace overlaps latitude", dict(ws=LAT - 4))]


def _call_abi(a):
    f = C.c_float
    return _lib.load().gclm_hypothesis_scores(a["model"], a["cam"], a["grav"], a["B"], a["N"], a["H"], a["W"], a["up"], a["lat"],
                                              a["upc"], a["latc"], a["mask"], f(a["tu"]), f(a["tl"]), f(a["wu"]), f(a["wl"]), a["ws"],
                                              a["ws_bytes"], a["scores"], a["best"], None)


@pytest.mark.parametrize("what,change", BAD, ids=[b[0] for b in BAD])
def test_invalid_arguments_are_refused_before_any_hip_call(what, change):
    assert _call_abi({**OK, **change}) == -3, what


def test_workspace_size_is_monotone_and_zero_for_invalid_sizes():
    ws = _lib.load().gclm_hypothesis_scores_workspace
    K = fields.HYPOTHESIS_CHUNK
    assert 0 < ws(2, 7, 48, 64) <= OK["ws_bytes"]
    assert ws(1, 1, 1, 1) == 2 * K * 4 and ws(2, K + 1, 48, 64) == 2 * 2 * 12 * 2 * K * 4     # (B, chunks, tiles of one pixel per lane, 2 K floats)
    for grow in ((3, 7, 48, 64), (2, K + 1, 48, 64), (2, 7, 49, 64), (2, 7, 48, 65)):
        assert ws(*grow) > ws(2, 7, 48, 64), grow
    for B, N, H, W in ((1, 1, 1, 1), (7, 33, 479, 641), (16, 2000, 320, 320)):
        assert ws(B, N, H, W) <= ws(B + 1, N, H, W) and ws(B, N, H, W) <= ws(B, N + 1, H, W) <= ws(B, N + K, H, W)
        assert ws(B, N, H, W) <= ws(B, N, H + 1, W) <= ws(B, N, H + 1, W + 1)
    assert ws(16, 2000, 320, 320) < 512 << 20
    for bad in ((0, 7, 48, 64), (65536, 7, 48, 64), (2, 0, 48, 64), (2, 65536, 48, 64), (2, 7, 0, 64), (2, 7, 48, 0),
                (2, 7, 65536, 32768), (2, 7, 2 ** 31 - 1, 1), (-1, 7, 48, 64), (2, -1, 48, 64)):
        assert ws(*bad) == 0, bad


# ------------------------------------------------------------------ the call path (the recorder of test_host_calls.py)
def _inputs(B, N, H=2, W=2):
    g = torch.Generator().manual_seed(0)
    cam = torch.tensor([float(W), float(H), 1.5, 1.5, W / 2, H / 2, 0.05, 0.0]).repeat(B, N, 1)
    grav = torch.tensor([0.0, 1.0, 0.0]).repeat(B, N, 1)
    return cam, grav, torch.randn(B, 2, H, W, generator=g), torch.rand(B, 1, H, W, generator=g), torch.rand(B, H, W, generator=g), \
        torch.rand(B, H, W, generator=g), torch.ones(B, H, W)


def test_hypothesis_scores_hands_over_the_arguments_of_the_header(rec):  # noqa: F811
    cam, grav, up, lat, upc, latc, mask = _inputs(2, 5)
    scores, best = fields.hypothesis_scores("radial", cam, grav, up, lat, upc, latc, mask, 3.0, 0.5, 2.0, 0.25)
    assert scores.shape == (2, 5, 3) and best.shape == (2,) and best.dtype == torch.int32 and scores.dtype == torch.float32
    (n0, a0), (n1, a1) = rec.calls
    assert (n0, a0) == ("gclm_hypothesis_scores_workspace", (2, 5, 2, 2)) and n1 == "gclm_hypothesis_scores"
    ws = a1[16]
    assert a1 == (2, p(cam), p(grav), 2, 5, 2, 2, p(up), p(lat), p(upc), p(latc), p(mask), 3.0, 0.5, 2.0, 0.25, ws, 0, p(scores),
                  p(best), STREAM)
    assert isinstance(ws, int) and ws not in (p(scores), p(best)) and not rec.entered
    assert len(a1) == len(ARGS)


def test_hypothesis_scores_passes_null_for_absent_planes(rec):  # noqa: F811
    cam, grav, up, lat, upc, latc, mask = _inputs(2, 3)
    fields.hypothesis_scores("pinhole", cam, grav, None, lat)
    a = rec.calls[1][1]
    assert a[:16] == (0, p(cam), p(grav), 2, 3, 2, 2, None, p(lat), None, None, None, 1.0, 1.0, 1.0, 1.0)
    del rec.calls[:]
    fields.hypothesis_scores("pinhole", cam, grav, up, None, upc, None, mask)
    assert rec.calls[1][1][7:12] == (p(up), None, p(upc), None, p(mask))
    with pytest.raises(ValueError):
        fields.hypothesis_scores("pinhole", cam, grav)
    with pytest.raises(ValueError):
        fields.hypothesis_scores("pinhole", cam, grav, None, lat, upc)
    with pytest.raises(ValueError):
        fields.hypothesis_scores("pinhole", cam[:, 0], grav[:, 0], up, lat)          # (B, 8): no hypothesis dimension
    with pytest.raises(ValueError):
        fields.hypothesis_scores("pinhole", cam, grav[:, :2], up, lat)


def test_hypothesis_scores_slices_and_advances_every_pointer(rec):  # noqa: F811
    B, N = MAX + 3, 2
    cam, grav, up, lat, upc, latc, mask = _inputs(B, N, 1, 1)
    scores, best = fields.hypothesis_scores("pinhole", cam, grav, up, lat, upc, latc, mask)
    (_, w), (_, first), (_, second) = rec.calls
    assert w == (MAX, N, 1, 1)                   # one workspace, sized for the largest call
    ws = first[16]
    assert first == (0, p(cam), p(grav), MAX, N, 1, 1, p(up), p(lat), p(upc), p(latc), p(mask), 1.0, 1.0, 1.0, 1.0, ws, 0, p(scores),
                     p(best), STREAM)
    assert second == (0, p(cam) + MAX * N * 32, p(grav) + MAX * N * 12, 3, N, 1, 1, p(up) + MAX * 8, p(lat) + MAX * 4,
                      p(upc) + MAX * 4, p(latc) + MAX * 4, p(mask) + MAX * 4, 1.0, 1.0, 1.0, 1.0, ws, 0, p(scores) + MAX * N * 12,
                      p(best) + MAX * 4, STREAM)
    assert _call.MAX_CALL == MAX


# ------------------------------------------------------------------ the GPU test's gate, checked here
def _named(model, B, H, W, kind="random", off=False):
    case = (model, B, H, W, kind, off)
    assert case in fg.CASES + fg.EXTREMES, case
    return case


SELF = [_named("pinhole", 3, 37, 53), _named("simple_divisional", 3, 37, 53, off=True), _named("simple_divisional", 2, 30, 200),
        _named("simple_divisional", 2, 30, 44, "pitch+")]
WEIGHTS = (2.0, 0.5)                             # up_weight != lat_weight: the swapped-weights mutant has something to swap
_cache = {}


def _case(case):
    """(cams, gravs, data, hypotheses, mask, yardstick with the mask and WEIGHTS, plain yardstick) of a case at N = 7, computed
    once and left unchanged."""
    if case not in _cache:
        cams, gravs, data = fg.make_case(case)
        hc, hgv = hg.hypotheses(cams, gravs, 7)
        mask = hg.make_mask(case)
        _cache[case] = (cams, gravs, data, hc, hgv, mask, hg.yardstick(case, hc, hgv, data, weights=WEIGHTS, mask=mask),
                        hg.yardstick(case, hc, hgv, data))
    return _cache[case]


def test_the_identical_pair_is_identical():
    cams, gravs, _ = fg.make_case(SELF[0])
    hc, hgv = hg.hypotheses(cams, gravs, 2 * fields.HYPOTHESIS_CHUNK + 3)
    i, j = hg.PAIR
    assert torch.equal(hc[:, i], hc[:, j]) and torch.equal(hgv[:, i], hgv[:, j])
    flat = torch.cat([hc, hgv], -1)[0]
    assert len({tuple(r.tolist()) for r in flat}) == flat.shape[0] - 1          # ... and the only repeated row


@pytest.mark.parametrize("case", SELF, ids=fg.case_id)
def test_gate_is_not_vacuous(case):
    """Every interval is narrower than 1 % of the field's sum of weights, and at least one image's admissible set is one
    index or the identical pair alone."""
    *_, masked, y = _case(case)
    slack = (2 * y["ks"] * hg.K_ROUND * hg.U)
    assert masked["width"].max().item() + slack < 0.01
    print(f"{fg.case_id(case)}: worst width {y['width'].max().item():.3%} of sum c, kappa_s {y['ks']:.2f}, admissible "
          f"{[r.nonzero().flatten().tolist() for r in y['admissible']]}")
    assert y["width"].max().item() + slack < 0.01
    assert hg.decisive(y)


@pytest.mark.parametrize("case", SELF, ids=fg.case_id)
def test_gate_passes_an_honest_float32_restatement(case):
    cams, gravs, data, hc, hgv, mask, y, plain = _case(case)
    v = hg.verdict(y, hg.restate(case, hc, hgv, data, weights=WEIGHTS, mask=mask))
    print(f"{fg.case_id(case)}: honest float32 {v}")
    assert hg.passes(v), v
    assert hg.passes(hg.verdict(plain, hg.restate(case, hc, hgv, data)))
    for which in ("noconf", "up", "lat"):                 # ... and the other three ways a shape is scored, without a mask
        d = fg.subset(data, which)
        v = hg.verdict(hg.yardstick(case, hc, hgv, d), hg.restate(case, hc, hgv, d))
        assert hg.passes(v), (which, v)


# (mutant, what it must push out)
MUTANTS = [("nomask", "up"), ("radians", "up"), ("radians", "lat"), ("swapconf", "up"), ("swapconf", "lat"), ("dropmask", "up"),
           ("dropmask", "lat"), ("swapweights", "total"), ("transposed", "total"), ("lasttie", "best_a")]


@pytest.mark.parametrize("case", [SELF[0], SELF[2]], ids=fg.case_id)
@pytest.mark.parametrize("mutant,what", MUTANTS, ids=[f"{m}-{w}" for m, w in MUTANTS])
def test_gate_fails_each_mutant(case, mutant, what):
    cams, gravs, data, hc, hgv, mask, y, plain = _case(case)
    v = hg.verdict(y, hg.restate(case, hc, hgv, data, weights=WEIGHTS, mask=mask, mutant=mutant))
    print(f"{mutant} on {fg.case_id(case)}: {v}")
    assert not hg.passes(v) and v[what] > 0, (mutant, v)


@pytest.mark.parametrize("case", [SELF[0], SELF[1]], ids=fg.case_id)
def test_gate_fails_le_for_lt(case):
    """<= for <: told apart where an error EQUALS the threshold.  At an up threshold of 0 the pixels under the decoders' mask
    (error exactly 0, gate 0: image 0 holds eleven) are hits of the mutant alone."""
    cams, gravs, data, hc, hgv, mask, _, _ = _case(case)
    y = hg.yardstick(case, hc, hgv, data, thresholds=(0.0, 1.0), weights=WEIGHTS, mask=None)
    assert hg.passes(hg.verdict(y, hg.restate(case, hc, hgv, data, (0.0, 1.0), WEIGHTS)))
    v = hg.verdict(y, hg.restate(case, hc, hgv, data, (0.0, 1.0), WEIGHTS, mutant="le"))
    print(f"le on {fg.case_id(case)}: {v}")
    assert v["up"] > 0 and v["total"] > 0, v


def test_first_argmax_takes_nan_as_the_maximum():
    t = torch.tensor([[1.0, 3.0, 3.0, 2.0], [1.0, math.nan, 5.0, math.nan], [-math.inf, -math.inf, -math.inf, -math.inf]])
    assert hg.first_argmax(t).tolist() == [1, 1, 0] == torch.argmax(t, 1).tolist()


# ------------------------------------------------------------------ rank_calibrations off the device
def _wrappers(model, hc, hgv, dtype, flat):
    B, N = hc.shape[:2]
    c, g = hc.to(dtype), hgv.to(dtype)
    if flat:
        c, g = c.reshape(B * N, 8), g.reshape(B * N, 3)
    cam, grav = camera_models[model](c), Gravity(g)
    grav._data = g                               # as stored: the yardstick does not renormalise either
    return cam, grav


@pytest.mark.parametrize("flat", [False, True], ids=["B,N", "flat"])
def test_rank_calibrations_takes_the_torch_path_off_the_device(flat, monkeypatch):
    """CPU tensors never reach the library.  In float64 the composition is the yardstick's own arithmetic up to the last
    bits of acos, so it is held to the gate's intervals; in float32 it quantises up errors at 0.02 degrees and is held to
    the float64 result within 2 % of the weights only."""
    case = SELF[0]
    cams, gravs, data, hc, hgv, mask, y, plain = _case(case)
    monkeypatch.setattr(fields, "hypothesis_scores", lambda *a, **k: pytest.fail("the library was called"))
    monkeypatch.setattr(metrics, "_RANK_CHUNK_PIXELS", case[1] * case[2] * case[3] * 3)        # three hypotheses per chunk
    cam, grav = _wrappers(case[0], hc, hgv, torch.float64, flat)
    out = metrics.rank_calibrations({k: v.double() for k, v in data.items()}, cam, grav, up_weight=WEIGHTS[0],
                                    latitude_weight=WEIGHTS[1], mask=mask.double())
    assert sorted(out) == ["best", "camera", "gravity", "latitude_scores", "scores", "up_scores"]
    assert out["scores"].shape == (case[1], 7) and out["best"].dtype == torch.int64 and out["best"].shape == (case[1],)
    scores = torch.stack([out["up_scores"], out["latitude_scores"], out["scores"]], -1)
    v = hg.verdict(y, {"scores": scores, "best": out["best"]})
    print(f"torch float64: {v}")
    assert hg.passes(v), v
    rows = torch.arange(case[1])
    assert torch.equal(out["camera"]._data, hc.double()[rows, out["best"]]) and type(out["camera"]) is camera_models[case[0]]
    assert torch.equal(out["gravity"]._data, hgv.double()[rows, out["best"]]) and out["camera"].shape == (case[1],)
    cam32, grav32 = _wrappers(case[0], hc, hgv, torch.float32, flat)
    out32 = metrics.rank_calibrations(data, cam32, grav32, up_weight=WEIGHTS[0], latitude_weight=WEIGHTS[1], mask=mask)
    assert out32["scores"].dtype == torch.float32
    assert ((out32["scores"].double() - out["scores"]).abs() <= 0.02 * (WEIGHTS[0] * y["csum"][:, :1] + WEIGHTS[1] * y["csum"][:, 1:])).all()
    only_lat = metrics.rank_calibrations({"latitude_field": data["latitude_field"]}, cam32, grav32)
    assert (only_lat["up_scores"] == 0).all() and torch.equal(only_lat["scores"], only_lat["latitude_scores"])
    with pytest.raises(ValueError):
        metrics.rank_calibrations({}, cam32, grav32)
    with pytest.raises(ValueError):
        metrics.rank_calibrations(data, cam32[:5] if flat else cam32[:, :5], grav32)


# ------------------------------------------------------------------ code objects
VGPR_MAX, LDS_MAX, FINISH_VGPR_MAX, FINISH_LDS_MAX = 82, 512, 38, 16512        # the figures DESIGN 3.10 reports


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="LLVM tools missing")
def test_hypothesis_kernels_carry_no_scratch(tmp_path):
    from test_kernel_audit import kernel_metadata
    k = {n: v for n, v in kernel_metadata(tmp_path).items() if "hypothesis" in n}
    for m in range(4):
        for px in (1, 2, 4):
            assert any(f"hypothesis_kernelILi{m}ELi{px}E" in n for n in k), (m, px, sorted(k))
    finish = [v for n, v in k.items() if "hypothesis_finish_kernel" in n]
    assert len(finish) == 1 and len(k) == 13
    print({n: v for n, v in k.items()})
    assert all(v["scratch"] == 0 for v in k.values()), k
    assert all(v["vgpr"] <= VGPR_MAX and v["lds"] <= LDS_MAX for n, v in k.items() if "finish" not in n), k
    assert finish[0]["vgpr"] <= FINISH_VGPR_MAX and finish[0]["lds"] <= FINISH_LDS_MAX, finish


# ------------------------------------------------------------------ the caller's workspace
def _device_call(case, dev):
    cams, gravs, data = fg.make_case(case)
    hc, hgv = (t.to(dev) for t in hg.hypotheses(cams, gravs, 7))
    planes = [data[k].to(dev) for k in ("up_field", "latitude_field", "up_confidence", "latitude_confidence")]
    return lambda: fields.hypothesis_scores(case[0], hc, hgv, *planes, up_weight=WEIGHTS[0], lat_weight=WEIGHTS[1])


@pytest.mark.gpu
def test_results_do_not_depend_on_what_the_workspace_held(monkeypatch):
    """gclm_hypothesis_scores at 30 x 200, seven hypotheses (tile columns and rows both ragged) with the wrapper's torch.empty
    workspace holding 0x00 bytes, 0xFF bytes, and the records of a call at 3 x 37 x 53: the same scores and the same winner."""
    from workspace_fill import same_bits_whatever_the_memory_held
    dev = torch.device("cuda:0")
    same_bits_whatever_the_memory_held(monkeypatch, dev, _device_call(SELF[2], dev), _device_call(SELF[0], dev))
