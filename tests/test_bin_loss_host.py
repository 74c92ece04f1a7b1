"""CPU: the classification heads' loss without a device -- losses.bin_loss against F.cross_entropy and the weighting in
float64; the keys, the single heads and the refusals of losses.perspective_bin_loss on its torch path; the gate module on
itself (a float32 restatement passes, a wrong bin and a wrong weighting do not); gclm_bin_loss, gclm_bin_loss_grad and
gclm_bin_loss_workspace declared, exported, bound and in the changelog; every invalid argument refused before any HIP call and
the legal neighbours reaching the launch; the workspace size; the kernels' resource usage (no scratch)."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

import bin_loss_gate as bg
import perspective_gate as pg
from abi_harness import HEADER, assert_declared_exported_and_bound
from conftest import ROOT
from geocalib_amd import Gravity, _lib, losses, perspective_encoding as pe
from geocalib_amd.camera import camera_models


# ------------------------------------------------------------------ the definition
def calibration(model="simple_radial", B=2, H=6, W=8, dtype=torch.float64):
    cams, gravs = bg.calibration(model, H, W, 12)
    camera, gravity = camera_models[model](cams[:B].to(dtype)), Gravity(gravs[:B].to(dtype))
    gravity._data = gravs[:B].to(dtype)
    return camera, gravity


@pytest.mark.parametrize("weighted", [False, True], ids=["mean", "confidence"])
def test_bin_loss_is_cross_entropy_plus_the_weighting_in_float64(weighted):
    g = torch.Generator().manual_seed(4)
    z = torch.randn(3, 9, 5, 7, generator=g, dtype=torch.float64, requires_grad=True)
    t = torch.randint(0, 9, (3, 5, 7), generator=g)
    conf = torch.rand(3, 1, 5, 7, generator=g, dtype=torch.float64).requires_grad_(True) if weighted else None
    ce = F.cross_entropy(z, t, reduction="none")
    want = (ce * conf[:, 0].detach() / conf[:, 0].detach().sum((1, 2), keepdim=True)).sum((1, 2)) if weighted else ce.mean((1, 2))
    got = losses.bin_loss(z, t, conf)
    assert got.dtype == torch.float64 and torch.allclose(got, want, rtol=1e-13, atol=0)
    (g1,) = torch.autograd.grad(got.sum(), z, retain_graph=True)
    (g2,) = torch.autograd.grad(want.sum(), z)
    assert torch.allclose(g1, g2, rtol=1e-12, atol=1e-15)
    if weighted:
        assert conf.grad is None and torch.allclose(losses.bin_loss(z, t, conf, use_uncertainty_loss=False), ce.mean((1, 2)), rtol=1e-13)
        assert losses.bin_loss(z, t, torch.zeros(3, 5, 7, dtype=torch.float64)).isnan().all()
    # 16-bit logits are the floats they widen to; accuracy is torch.argmax's
    for dt in (torch.float16, torch.bfloat16):
        assert torch.equal(losses.bin_loss(z.detach().to(dt), t), losses.bin_loss(z.detach().to(dt).float(), t))
    assert torch.equal(losses.bin_accuracy(z, t), (z.argmax(1) == t).double().mean((1, 2)))
    with pytest.raises(ValueError):
        losses.bin_loss(z, t[:, :4])


def test_keys_single_heads_weights_and_float64():
    camera, gravity = calibration()
    g = torch.Generator().manual_seed(5)
    up = torch.randn(2, 73, 6, 8, generator=g, dtype=torch.float64, requires_grad=True)
    lat = torch.randn(2, 180, 6, 8, generator=g, dtype=torch.float64, requires_grad=True)
    conf = torch.rand(2, 6, 8, generator=g, dtype=torch.float64)
    pred = {"up_logits": up, "latitude_logits": lat, "up_confidence": conf[:, None], "latitude_confidence": conf}
    out = losses.perspective_bin_loss(pred, camera, gravity, up_loss_weight=0.5, latitude_loss_weight=3.0)
    assert list(out) == ["up-classification-loss", "up_total", "up_bin_accuracy", "latitude-classification-loss", "latitude_total",
                         "latitude_bin_accuracy", "perspective_total"]
    assert all(v.shape == (2,) and v.dtype == torch.float64 for v in out.values())
    assert not out["up_bin_accuracy"].requires_grad and not out["latitude_bin_accuracy"].requires_grad
    t_up, t_lat = losses.perspective_target_bins(camera, gravity, 73, 180)
    fields = pg.fields("simple_radial", camera._data, gravity._data, 6, 8)
    want = bg.targets_of_fields(fields, 73, 180)
    assert torch.equal(t_up, want["up"][0]) and torch.equal(t_lat, want["latitude"][0])
    assert torch.allclose(out["up_total"], 0.5 * losses.bin_loss(up, t_up, conf), rtol=1e-14)
    assert torch.allclose(out["latitude_total"], 3.0 * losses.bin_loss(lat, t_lat, conf), rtol=1e-14)
    assert torch.equal(out["perspective_total"], out["up_total"] + out["latitude_total"])
    assert torch.equal(out["up_bin_accuracy"], losses.bin_accuracy(up, t_up))
    out["perspective_total"].sum().backward()
    assert up.grad is not None and lat.grad is not None
    for name in ("up", "latitude"):
        alone = losses.perspective_bin_loss({k: v for k, v in pred.items() if k.startswith(name)}, camera, gravity, up_loss_weight=0.5,
                                            latitude_loss_weight=3.0)
        assert set(alone) == {f"{name}-classification-loss", f"{name}_total", f"{name}_bin_accuracy", "perspective_total"}
        assert torch.equal(alone[f"{name}_total"], out[f"{name}_total"]) and torch.equal(alone["perspective_total"], out[f"{name}_total"])
    plain = losses.perspective_bin_loss(pred, camera, gravity, use_uncertainty_loss=False)
    assert torch.allclose(plain["up_total"], F.cross_entropy(up, t_up, reduction="none").mean((1, 2)), rtol=1e-14)
    # float32 on the CPU, an unbatched calibration, a confidence for an absent head
    cam1, grav1 = calibration(B=1, dtype=torch.float32)
    one = losses.perspective_bin_loss({"up_logits": up[:1].float(), "latitude_confidence": conf[:1]}, cam1[0], grav1[0])
    assert one["up_total"].shape == (1,) and one["up_total"].dtype == torch.float32


def test_refusals_raise_before_the_library_is_loaded(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    camera, gravity = calibration()
    up, lat = torch.zeros(2, 73, 6, 8), torch.zeros(2, 180, 6, 8)
    n = next(n for n in range(2, 400) if torch.arange(-90, 90, 180 / n).numel() != n)      # a latitude count without a table
    with pytest.raises(ValueError):
        pe._latitude_edges(n)
    bad = [({}, "neither head"), ({"up_confidence": torch.ones(2, 6, 8)}, "a confidence alone"),
           ({"up_logits": up[0]}, "rank"), ({"up_logits": up, "latitude_logits": lat[:1]}, "B"),
           ({"up_logits": up, "latitude_logits": lat[..., :7]}, "W"), ({"up_logits": up[:, :1]}, "one up bin"),
           ({"latitude_logits": torch.zeros(2, n, 6, 8)}, "a latitude count without classes"),
           ({"latitude_logits": lat[:, :0]}, "no latitude bin"),
           ({"up_logits": up, "up_confidence": torch.ones(2, 6, 7)}, "a confidence of another size"),
           ({"up_logits": torch.zeros(2, 73, 5, 8)}, "logits of another size than the camera's (torch path)")]
    for pred, why in bad:
        with pytest.raises(ValueError):
            losses.perspective_bin_loss(pred, camera, gravity)
            pytest.fail(why)


def test_the_gate_passes_a_float32_restatement_and_catches_mutants():
    """bin_loss_gate on itself: the bins of the float32 fields and the float32 composition pass every gate of every case; a bin
    off by one at a decided pixel, a plain mean where a confidence is given, and a gradient that lacks the one-hot do not."""
    for case in bg.CASES:
        inp = bg.inputs(case)
        model, H, W = case[:3]
        f32 = pg.fields(model, inp["cams"], inp["gravs"], H, W, torch.float32)
        t32 = bg.targets_of_fields(f32, inp["counts"]["up"], inp["counts"]["latitude"])
        bins = {n: t32[n][0] for n in bg.heads_of(case)}
        y64, u = bg.units(case, bins)
        y32 = bg.composition(case, bins, torch.float32)
        for n in bg.heads_of(case):
            wrong, undecided = bg.bins_verdict(case, n, bins[n])
            assert wrong == 0 and undecided <= 0.01, (bg.case_id(case), n, wrong, undecided)
            assert bg.passes(bg.verdict(case, y64, u, n, y32["loss"][n], y32["grad"][n].to(case[5]))), (bg.case_id(case), n)
            assert torch.equal(y32["hits"][n], y64["hits"][n])
    case = bg.CASES[1]
    inp = bg.inputs(case)
    t, _, _, und = inp["targets"]["up"]
    off = t.clone()
    b, y, x = (~und).nonzero()[0].tolist()
    off[b, y, x] = (off[b, y, x] + 1) % 72
    assert bg.bins_verdict(case, "up", off)[0] == 1
    bins = {n: inp["targets"][n][0] for n in bg.heads_of(case)}
    y64, u = bg.units(case, bins)
    z = inp["pred"]["up_logits"].clone().requires_grad_(True)
    plain = losses.bin_loss(z, bins["up"]) * bg.WEIGHTS["up"]
    (torch.tensor(bg.GOUT) * plain).sum().backward()
    assert bg.verdict(case, y64, u, "up", plain.detach(), z.grad)["loss"] > bg.GATE
    good = bg.composition(case, bins, torch.float32)
    no_onehot = good["grad"]["up"] + torch.zeros_like(z).scatter_(1, bins["up"][:, None], 1e-4)
    assert bg.verdict(case, y64, u, "up", good["loss"]["up"], no_onehot)["grad"] > bg.GATE


# ------------------------------------------------------------------ the entry points
P, I, F32P = "const void*", "int", "const float*"
FORWARD = [I, F32P, F32P, I, I, I, P, I, P, I, I, F32P, F32P, "void*", "size_t", "float*", "float*", "int16_t*", "void*"]
GRAD = [P, I, P, I, I, F32P, F32P, I, I, I, F32P, "const int16_t*", F32P, "void*", "void*", "void*"]


def test_entry_points_are_declared_exported_bound_and_documented():
    args = assert_declared_exported_and_bound("gclm_bin_loss", FORWARD)
    assert len(args) == 19 and [a for a in args if a is C.c_int] == [C.c_int] * 7 and args[14] is C.c_size_t
    args = assert_declared_exported_and_bound("gclm_bin_loss_grad", GRAD)
    assert len(args) == 16 and [a for a in args if a is C.c_int] == [C.c_int] * 6
    assert_declared_exported_and_bound("gclm_bin_loss_workspace", [I, I, I], ret="size_t")
    header = open(HEADER).read()
    log = header[header.index("ABI version:"):header.index("#define GCLM_VERSION")]
    assert "gclm_bin_loss, gclm_bin_loss_grad and gclm_bin_loss_workspace added, also within 610" in log
    assert "#define GCLM_VERSION 610" in header
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "| `gclm_bin_loss` |" in integration and "perspective_bin_loss" in integration
    assert "gclm_bin_loss.hip" in open(os.path.join(ROOT, "README.md")).read()
    assert re.search(r"^#+ 3\.23", open(os.path.join(ROOT, "DESIGN.md")).read(), flags=re.M)


# fake, never dereferenced device addresses: every call below must be refused before the first HIP call
CAM, GRAV, UPL, LATL, UPC, LATC, WS, OUT, LSE, BINS, SCALE, GUP, GLAT = (0x100000, 0x110000, 0x1000000, 0x2000000, 0x3000000, 0x3100000,
                                                                         0x4000000, 0x4100000, 0x5000000, 0x5100000, 0x5200000,
                                                                         0x6000000, 0x7000000)
Bn, Hn, Wn = 2, 6, 8
PX = Bn * Hn * Wn * 4                    # bytes of a (B, H, W) float plane
WS_BYTES = 1 << 16
OK = dict(model=1, cam=CAM, grav=GRAV, B=Bn, H=Hn, W=Wn, upl=UPL, Ku=73, latl=LATL, Kl=180, dt=0, upc=UPC, latc=LATC, ws=WS,
          ws_bytes=WS_BYTES, out=OUT, lse=LSE, bins=BINS, scale=SCALE, gup=GUP, glat=GLAT)
SHARED_BAD = [("both logit tensors NULL", dict(upl=None, latl=None, upc=None, latc=None, gup=None, glat=None)),
              ("an up confidence without its logits", dict(upl=None, gup=None)), ("a latitude confidence without its logits", dict(latl=None, glat=None)),
              ("one up bin", dict(Ku=1)), ("no up bin", dict(Ku=0)), ("2049 up bins", dict(Ku=2049)), ("no latitude bin", dict(Kl=0)),
              ("negative latitude bins", dict(Kl=-5)), ("2049 latitude bins", dict(Kl=2049)), ("dtype 3", dict(dt=3)), ("dtype -1", dict(dt=-1)),
              ("H = 0", dict(H=0)), ("W = 0", dict(W=0)), ("H < 0", dict(H=-6)), ("B < 0", dict(B=-1)), ("B = 65536", dict(B=65536)),
              ("H W over 2^31", dict(H=65536, W=32768)),
              ("half logits off a 2-byte boundary", dict(dt=1, upl=UPL + 1)), ("float logits off a 4-byte boundary", dict(latl=LATL + 2)),
              ("a confidence off a 4-byte boundary", dict(upc=UPC + 2)), ("lse off a 4-byte boundary", dict(lse=LSE + 2)),
              ("bins off a 2-byte boundary", dict(bins=BINS + 1)), ("NULL lse", dict(lse=None)), ("NULL bins", dict(bins=None))]
FORWARD_BAD = SHARED_BAD + [
    ("NULL camera", dict(cam=None)), ("NULL gravity", dict(grav=None)), ("NULL workspace", dict(ws=None)), ("NULL out", dict(out=None)),
    ("model 4", dict(model=4)), ("model -1", dict(model=-1)), ("a workspace one byte short", dict(ws_bytes="short")),
    ("out off a 4-byte boundary", dict(out=OUT + 2)), ("workspace off a 4-byte boundary", dict(ws=WS + 2)),
    ("lse starts at the up logits' last float", dict(lse=UPL + 73 * PX - 4)), ("lse ends one float inside the latitude logits", dict(lse=LATL - 2 * PX + 4)),
    ("bins on the latitude logits", dict(bins=LATL)), ("bins on the up confidence's last float", dict(bins=UPC + PX - 4)),
    ("out on the camera rows", dict(out=CAM)), ("out on the gravity's last float", dict(out=GRAV + Bn * 12 - 4)),
    ("the workspace on the latitude confidence", dict(ws=LATC)), ("lse on bins", dict(lse=BINS)), ("bins inside lse", dict(bins=LSE + PX)),
    ("out inside the workspace", dict(out=WS + 64)), ("the workspace's end on out", dict(ws=OUT - 96 + 4))]
GRAD_BAD = SHARED_BAD + [
    ("NULL scale", dict(scale=None)), ("both gradients NULL", dict(gup=None, glat=None)),
    ("an up gradient off a 4-byte boundary", dict(gup=GUP + 2)), ("a half gradient off a 2-byte boundary", dict(dt=2, glat=GLAT + 1)),
    ("the up gradient on the up logits", dict(gup=UPL)), ("the up gradient ends one float inside the latitude logits", dict(gup=LATL - 73 * PX + 4)),
    ("the latitude gradient on the up confidence", dict(glat=UPC)), ("the latitude gradient on lse's last float", dict(glat=LSE + 2 * PX - 4)),
    ("the up gradient on bins", dict(gup=BINS)), ("the latitude gradient on the scales", dict(glat=SCALE)),
    ("the gradients on each other", dict(glat=GUP + 72 * PX))]
FORWARD_OK = [dict(), dict(dt=1), dict(dt=2), dict(Ku=2, Kl=1), dict(Ku=2048, Kl=2048), dict(H=1, W=1), dict(H=5, W=7), dict(model=0), dict(model=3),
              dict(upc=None), dict(latc=None, upc=None), dict(upl=None, upc=None, Ku=0), dict(latl=None, latc=None, Kl=-1),
              dict(lse=UPL + 73 * PX), dict(bins=UPC + PX), dict(out=GRAV + Bn * 12), dict(dt=2, upl=UPL + 2, latl=LATL + 6), dict(bins=BINS + 2),
              dict(ws_bytes="exact")]
GRAD_OK = [dict(), dict(dt=1), dict(dt=2), dict(Ku=2, Kl=1), dict(gup=None), dict(glat=None), dict(upl=None, upc=None, gup=None, Ku=0),
           dict(latl=None, latc=None, glat=None, Kl=0), dict(gup=UPL + 73 * PX), dict(glat=LSE + 2 * PX), dict(upc=None, latc=None)]


def _forward(a):
    need = _lib.load().gclm_bin_loss_workspace(a["B"], a["H"], a["W"])
    ws_bytes = {"short": need - 1, "exact": need}.get(a["ws_bytes"], a["ws_bytes"])
    return _lib.load().gclm_bin_loss(a["model"], a["cam"], a["grav"], a["B"], a["H"], a["W"], a["upl"], a["Ku"], a["latl"], a["Kl"], a["dt"],
                                     a["upc"], a["latc"], a["ws"], ws_bytes, a["out"], a["lse"], a["bins"], None)


def _grad(a):
    return _lib.load().gclm_bin_loss_grad(a["upl"], a["Ku"], a["latl"], a["Kl"], a["dt"], a["upc"], a["latc"], a["B"], a["H"], a["W"],
                                          a["lse"], a["bins"], a["scale"], a["gup"], a["glat"], None)


@pytest.mark.parametrize("what,change", FORWARD_BAD, ids=[b[0] for b in FORWARD_BAD])
def test_forward_refuses_invalid_arguments_before_any_hip_call(what, change):
    assert set(change) <= set(OK)
    assert _forward({**OK, **change}) == -3, what


@pytest.mark.parametrize("what,change", GRAD_BAD, ids=[b[0] for b in GRAD_BAD])
def test_gradient_refuses_invalid_arguments_before_any_hip_call(what, change):
    assert set(change) <= set(OK)
    assert _grad({**OK, **change}) == -3, what


def test_an_empty_batch_succeeds_and_launches_nothing():
    assert _forward({**OK, "B": 0}) == 0 and _grad({**OK, "B": 0}) == 0


def test_the_valid_neighbours_reach_the_launch():
    """The neighbours of the refused calls -- ranges that only touch, the extreme bin counts, every dtype and model, absent
    confidences, each head alone (its count then not looked at) -- are valid and reach the launch, which fails without a
    device: -10."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: a valid call would launch on fake addresses")
    for change in FORWARD_OK:
        assert _forward({**OK, **change}) == -10, change
    for change in GRAD_OK:
        assert _grad({**OK, **change}) == -10, change


def test_workspace_size_is_monotone_and_zero_for_invalid_sizes():
    ws = _lib.load().gclm_bin_loss_workspace
    assert 0 < ws(Bn, Hn, Wn) <= WS_BYTES
    for B, H, W in ((1, 1, 1), (7, 479, 641), (64, 320, 480)):
        assert ws(B, H, W) <= ws(B + 1, H, W) and ws(B, H, W) <= ws(B, H + 1, W) <= ws(B, H + 1, W + 1)
    assert ws(64, 320, 480) < 1 << 20 and ws(1, 4, 64) == 6 * 4 and ws(1, 5, 65) == 4 * 6 * 4
    for bad in ((0, 48, 64), (65536, 48, 64), (2, 0, 64), (2, 48, 0), (2, 65536, 32768), (2, 2 ** 31 - 1, 1)):
        assert ws(*bad) == 0, bad


def test_kernels_carry_no_scratch(tmp_path):
    """Read from the code objects inside the built library, as tests/test_kernel_audit.py reads the sweeps': the flags are
    the build's own.  Forward: four models x three logit types x two widths; gradient: three types x two widths; the finish."""
    from test_kernel_audit import LLVM, SO, kernel_metadata
    if not (os.path.exists(SO) and os.path.exists(f"{LLVM}/llvm-readelf")):
        pytest.skip("library or LLVM tools missing")
    k = {n: v for n, v in kernel_metadata(tmp_path).items() if "bin_loss_" in n}
    assert len([n for n in k if "bin_loss_kernelILi" in n]) == 24, sorted(k)
    assert len([n for n in k if "bin_loss_grad_kernelILi" in n]) == 6 and len([n for n in k if "bin_loss_finish_kernel" in n]) == 1, sorted(k)
    assert not any(v["scratch"] for v in k.values()), k
    assert all(v["lds"] <= 4 * 8 * 6 * 4 for v in k.values()), k
