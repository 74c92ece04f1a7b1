"""gclm_field_loss_param_grad / gclm_perspective_fields_backward through the C ABI (tests/field_calib_grad_gate.py has the
fixture and the gate).

CPU: the entry points are declared, exported and bound; every invalid argument is refused before any HIP call; the workspace
size is monotone and 0 for sizes out of range; the keyword `calibration_grad` defaults to False everywhere; on the call
recorder, the wrappers hand the C entries the arguments of include/gclm.h and both autograd Functions call what is asked for,
nothing more, and return each gradient to its input; the committed
fixture meets the conditions its generator asserts -- per field and image at least 4 residuals on either side of Huber's
delta, no residual exactly 0, every pixel at least 1e-3 inside the latitude clamp, |q| >= 1e-3, fx != fy, the principal point
off the pixel grid, gravities with c of either sign, and for simple_divisional tau >= 1e-2 and k1 r2 != 0 everywhere (k1 = 0
exactly in the one extra case).

GPU: per image and entry |hip - ref64| <= 4 max(|ref32 - ref64|, 2^-23 A) for every recorded case of both entries, also with
the planes 4 bytes off their alignment (one pixel per lane); image i of a batch gets the bits it gets alone, gravity alone
gets the same gravity bits, two runs give equal bits; nothing outside (B, 8), (B, 3) and the told workspace size is written;
a refused call leaves its outputs untouched.

Measured on an MI355X (profiles/field_calib_grad_tests.log): worst ratio 1.000 (the k1 entry of the k1 = 0 up-only plane case:
the kernel gives 0, the unit is the reference's own 2.6e-23 of rounding), loss cases worst 0.63, median 0.011 over 3840
non-zero ratios; each case's worst and median ratio is printed before the assertion."""
import ctypes as C
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

from geocalib_amd import _call, _lib, fields, losses, perspective_fields as pf
from abi_harness import HEADER, assert_declared_exported_and_bound
from conftest import GOLDEN, ROOT
import field_calib_grad_gate as gate
from geocalib_amd import Gravity, camera_models
from test_host_calls import STREAM, p, rec  # noqa: F401  (the recorder fixture, not edited)

SHARED = ["int", "const float*", "const float*", "int", "int", "int"]
LOSS_ARGS = SHARED + ["const float*"] * 4 + ["int", "int", "const float*", "void*", "size_t", "float*", "float*", "void*"]
PLANES_ARGS = SHARED + ["int", "const float*", "const float*", "void*", "size_t", "float*", "float*", "void*"]


def test_entry_points_are_declared_exported_and_bound():
    for name, args in (("gclm_field_loss_param_grad", LOSS_ARGS), ("gclm_perspective_fields_backward", PLANES_ARGS)):
        for a, t in zip(assert_declared_exported_and_bound(name, args), args):
            assert t in ("int", "size_t") or a is C.c_void_p, (name, a, t)
    assert assert_declared_exported_and_bound("gclm_field_param_grad_workspace", ["int"] * 3, ret="size_t") == [C.c_int] * 3
    header = open(HEADER).read()
    changelog = header[header.index("ABI version:"):header.index("#define GCLM_VERSION")]
    assert all(n in changelog for n in ("gclm_field_loss_param_grad", "gclm_perspective_fields_backward", "gclm_field_param_grad_workspace"))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "| `gclm_field_loss_param_grad`, `gclm_perspective_fields_backward` (+ `gclm_field_param_grad_workspace`) |" in doc


def test_keyword_defaults():
    for fn in (losses.perspective_field_loss, pf.get_perspective_field, pf.get_up_field, pf.get_latitude_field):
        assert inspect.signature(fn).parameters["calibration_grad"].default is False, fn
    assert "calibration_grad" not in inspect.signature(losses.perspective_decoder_loss).parameters      # (passed through **loss_options)
    assert inspect.signature(pf._on_hip).parameters["calibration_grad"].default is False


def test_fixture_meets_its_conditions():
    spec = importlib.util.spec_from_file_location("make_golden_field_calib_grad", os.path.join(GOLDEN, "make_golden_field_calib_grad.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    z = gate.golden()
    assert (gen.B, gen.Q, gen.SHAPES, gen.MODELS) == (gate.B, gate.Q, gate.SHAPES, gate.MODELS)
    found = gate.sets()
    assert sorted(found) == sorted([(m, m, H, W) for m in gate.MODELS for H, W in gate.SHAPES] +
                                   [("simple_divisional_k0", "simple_divisional", *gate.SHAPES[0])])
    for tag, model, H, W in found:
        gen.check_conditions(model, {k: z[f"{tag}/{H}x{W}/{k}"] for k in gate.INPUTS}, k1_zero=tag.endswith("_k0"))
        names = [c[4] for c in gate.cases() if c[0] == tag and (c[2], c[3]) == (H, W)]
        want = [c[0] for c in gen.case_list((H, W))]
        assert set(names) <= set(want) and (tag.endswith("_k0") or sorted(names) == sorted(want)), (tag, names)
    # every loss type of either field, with and without confidences, each field alone, the planes with normalize on and off
    parsed = [gate.parse(c[4]) for c in gate.cases() if c[0] == "radial" and (c[2], c[3]) == gate.SHAPES[0]]
    assert {p[1] for p in parsed if p[0] == "loss"} >= {"l1", "l2", "dot", "cauchy", "huber", None}
    assert {p[2] for p in parsed if p[0] == "loss"} >= {"l1", "l2", "cauchy", "huber", None}
    assert {p[3] for p in parsed if p[0] == "loss"} == {True, False} and {p[4] for p in parsed if p[0] == "planes"} == {True, False}
    # the k1 = 0 case: the up field's share of the k1 entry is 0 in the reference, to the rounding its reverse mode leaves (its own
    # gradient is the yardstick there too)
    r64, r32, A = gate.reference(("simple_divisional_k0", "simple_divisional", *gate.SHAPES[0], "planes-up"))
    assert np.abs(r64[:, 6]).max() < 1e-12 and np.abs(r32[:, 6]).max() < 1e-12 and np.all(A[:, 6] == 0)
    assert os.path.getsize(gate.PATH) < 1 << 20


# ------------------------------------------------------------------ refusals
# fake, never dereferenced device addresses on the CPU; the GPU test below runs the same table on real buffers
FAKE = dict(cam=0x100000, grav=0x200000, up=0x4000000, lat=0x8000000, upc=0xC000000, latc=0x10000000, ws=0x20000000,
            gcam=0x30000000, ggrav=0x34000000, scale=0x38000000, gup=0x40000000, glat=0x50000000)
SIZES = dict(model=1, B=2, H=48, W=64, ul=0, ll=4, nrm=1, ws_bytes=1 << 24)
PX_BYTES = 2 * 48 * 64 * 4
BOTH = [("NULL camera", lambda a: dict(cam=None)), ("NULL gravity", lambda a: dict(grav=None)),
        ("both outputs NULL", lambda a: dict(gcam=None, ggrav=None)), ("NULL workspace", lambda a: dict(ws=None)),
        ("workspace too small", lambda a: dict(ws_bytes=2 * 12 * 9 * 8 - 1)),
        ("B = 0", lambda a: dict(B=0)), ("B > 65535", lambda a: dict(B=65536)), ("H = 0", lambda a: dict(H=0)), ("W = 0", lambda a: dict(W=0)),
        ("H * W > 2^31 - 1", lambda a: dict(H=65536, W=32768, ws_bytes=1 << 62)),
        ("tile grid over 2^32 threads", lambda a: dict(H=2 ** 31 - 1, W=1, ws_bytes=1 << 62)),
        ("model -1", lambda a: dict(model=-1)), ("model 4", lambda a: dict(model=4)),
        ("camera misaligned", lambda a: dict(cam=a["cam"] + 2)), ("gravity misaligned", lambda a: dict(grav=a["grav"] + 1)),
        ("camera gradient misaligned", lambda a: dict(gcam=a["gcam"] + 2)), ("gravity gradient misaligned", lambda a: dict(ggrav=a["ggrav"] + 1)),
        ("workspace not 8-byte aligned", lambda a: dict(ws=a["ws"] + 4)),
        ("camera gradient is the camera", lambda a: dict(gcam=a["cam"])), ("camera gradient overlaps the camera", lambda a: dict(gcam=a["cam"] + 60)),
        ("gravity gradient overlaps the gravity", lambda a: dict(ggrav=a["grav"] - 20)),
        ("camera gradient overlaps the gravity", lambda a: dict(gcam=a["grav"] + 20)),
        ("workspace overlaps the camera gradient", lambda a: dict(ws=a["gcam"] + 56)),
        ("workspace overlaps the camera", lambda a: dict(ws=a["cam"] - 2 * 12 * 9 * 8 + 8)),
        ("the gradients overlap", lambda a: dict(ggrav=a["gcam"] + 60))]
LOSS = [("both fields NULL", lambda a: dict(up=None, lat=None, upc=None, latc=None)), ("up confidence without up", lambda a: dict(up=None)),
        ("latitude confidence without latitude", lambda a: dict(lat=None)), ("up loss -1", lambda a: dict(ul=-1)), ("up loss 5", lambda a: dict(ul=5)),
        ("latitude loss -1", lambda a: dict(ll=-1)), ("latitude loss 5", lambda a: dict(ll=5)), ("dot for latitude", lambda a: dict(ll=2)),
        ("NULL scale", lambda a: dict(scale=None)), ("scale misaligned", lambda a: dict(scale=a["scale"] + 2)),
        ("up misaligned", lambda a: dict(up=a["up"] + 1)), ("latitude misaligned", lambda a: dict(lat=a["lat"] + 2)),
        ("up confidence misaligned", lambda a: dict(upc=a["upc"] + 3)), ("latitude confidence misaligned", lambda a: dict(latc=a["latc"] + 2)),
        ("camera gradient overlaps up", lambda a: dict(gcam=a["up"] + 2 * PX_BYTES - 4)),
        ("gravity gradient overlaps the scale", lambda a: dict(ggrav=a["scale"] + 12)),
        ("workspace overlaps the latitude confidence", lambda a: dict(ws=a["latc"] + PX_BYTES - 8)),
        ("workspace overlaps latitude", lambda a: dict(ws=a["lat"] - 8))]
PLANES = [("both cotangent planes NULL", lambda a: dict(gup=None, glat=None)), ("normalize 2", lambda a: dict(nrm=2)),
          ("normalize -1", lambda a: dict(nrm=-1)), ("up cotangent not 8-byte aligned", lambda a: dict(gup=a["gup"] + 4)),
          ("latitude cotangent misaligned", lambda a: dict(glat=a["glat"] + 2)),
          ("camera gradient overlaps the up cotangent", lambda a: dict(gcam=a["gup"] + 2 * PX_BYTES - 4)),
          ("gravity gradient overlaps the latitude cotangent", lambda a: dict(ggrav=a["glat"])),
          ("workspace overlaps the up cotangent", lambda a: dict(ws=a["gup"] - 8))]


def _loss_call(a):
    return _lib.load().gclm_field_loss_param_grad(a["model"], a["cam"], a["grav"], a["B"], a["H"], a["W"], a["up"], a["lat"], a["upc"],
                                                  a["latc"], a["ul"], a["ll"], a["scale"], a["ws"], a["ws_bytes"], a["gcam"], a["ggrav"], None)


def _planes_call(a):
    return _lib.load().gclm_perspective_fields_backward(a["model"], a["cam"], a["grav"], a["B"], a["H"], a["W"], a["nrm"], a["gup"],
                                                        a["glat"], a["ws"], a["ws_bytes"], a["gcam"], a["ggrav"], None)


@pytest.mark.parametrize("what,change", BOTH + LOSS, ids=[b[0] for b in BOTH + LOSS])
def test_invalid_arguments_of_the_loss_form_are_refused_before_any_hip_call(what, change):
    base = {**FAKE, **SIZES}
    assert _loss_call({**base, **change(base)}) == -3, what


@pytest.mark.parametrize("what,change", BOTH + PLANES, ids=[b[0] for b in BOTH + PLANES])
def test_invalid_arguments_of_the_planes_form_are_refused_before_any_hip_call(what, change):
    base = {**FAKE, **SIZES}
    assert _planes_call({**base, **change(base)}) == -3, what


def test_workspace_size_is_monotone_and_zero_for_invalid_sizes():
    ws = _lib.load().gclm_field_param_grad_workspace
    assert ws(2, 48, 64) == 2 * 12 * 9 * 8                      # images x tiles at one pixel per lane x nine float64 sums
    for grow in ((3, 48, 64), (2, 49, 64), (2, 48, 65)):
        assert ws(*grow) > ws(2, 48, 64), grow
    for B, H, W in ((1, 1, 1), (7, 479, 641), (1024, 480, 640)):
        assert ws(B, H, W) <= ws(B + 1, H, W) and ws(B, H, W) <= ws(B, H + 1, W) <= ws(B, H + 1, W + 1)
    assert ws(1024, 480, 640) < 128 << 20
    for bad in ((0, 48, 64), (65536, 48, 64), (2, 0, 64), (2, 48, 0), (2, 65536, 32768), (2, 2 ** 31 - 1, 1)):
        assert ws(*bad) == 0, bad


# ------------------------------------------------------------------ the host side, on the recorder (no device)
def _host_inputs(B=2, H=2, W=2):
    g = torch.Generator().manual_seed(3)
    cam = torch.tensor([[float(W), float(H), 1.5, 1.6, W / 2 + 0.3, H / 2 - 0.2, 0.05, 0.01]]).repeat(B, 1)
    grav = torch.tensor([[0.1, -0.9, 0.4]]).repeat(B, 1)
    return (cam, grav, torch.rand(B, 2, H, W, generator=g), torch.rand(B, 1, H, W, generator=g), torch.rand(B, H, W, generator=g),
            torch.rand(B, H, W, generator=g))


def test_wrappers_hand_over_the_arguments_of_the_header(rec):  # noqa: F811
    cam, grav, up, lat, upc, latc = _host_inputs()
    scale = torch.rand(2, 2)
    gc, gg = fields.field_loss_param_grad("radial", cam, grav, scale, up, lat, upc, latc, "dot", "huber")
    assert gc.shape == (2, 8) and gg.shape == (2, 3)
    (n0, a0), (n1, a1) = rec.calls
    assert (n0, a0) == ("gclm_field_param_grad_workspace", (2, 2, 2)) and n1 == "gclm_field_loss_param_grad"
    ws = a1[13]
    assert a1 == (2, p(cam), p(grav), 2, 2, 2, p(up), p(lat), p(upc), p(latc), 2, 4, p(scale), ws, 0, p(gc), p(gg), STREAM)
    assert isinstance(ws, int) and ws % 8 == 0 and not rec.entered
    del rec.calls[:]
    gc, gg = fields.field_loss_param_grad("pinhole", cam, grav, scale, None, lat, None, None, want_cam=False)
    assert gc is None and rec.calls[1][1][6:12] == (None, p(lat), None, None, 0, 0) and rec.calls[1][1][15:] == (None, p(gg), STREAM)
    del rec.calls[:]
    g_up, g_lat = torch.rand(2, 2, 2, 2), torch.rand(2, 2, 2, 1)            # (B, H, W, 2), (B, H, W, 1): the renderer's outputs
    gc, gg = fields.perspective_fields_backward("simple_divisional", cam, grav, g_up, g_lat, normalize=False)
    (n0, a0), (n1, a1) = rec.calls
    assert (n0, a0) == ("gclm_field_param_grad_workspace", (2, 2, 2)) and n1 == "gclm_perspective_fields_backward"
    assert a1 == (3, p(cam), p(grav), 2, 2, 2, 0, p(g_up), p(g_lat), a1[9], 0, p(gc), p(gg), STREAM)
    del rec.calls[:]
    gc, gg = fields.perspective_fields_backward("pinhole", cam, grav, None, g_lat[..., 0], want_grav=False)
    assert gg is None and rec.calls[1][1][6:9] == (1, None, p(g_lat)) and rec.calls[1][1][11:] == (p(gc), None, STREAM)
    for bad in (lambda: fields.perspective_fields_backward("pinhole", cam, grav),
                lambda: fields.perspective_fields_backward("pinhole", cam, grav, g_up, g_lat, want_cam=False, want_grav=False),
                lambda: fields.perspective_fields_backward("pinhole", cam, grav, g_up[:1], g_lat),
                lambda: fields.perspective_fields_backward("pinhole", cam, grav, g_up, g_lat[:, :1]),
                lambda: fields.field_loss_param_grad("pinhole", cam, grav, torch.rand(3, 2), up, lat),
                lambda: fields.field_loss_param_grad("pinhole", cam, grav, scale, up, lat, lat_loss="dot")):
        with pytest.raises(ValueError):
            bad()


def test_autograd_hands_the_calibration_its_gradients(rec, monkeypatch):  # noqa: F811
    """The plumbing of both Functions on the recorder (the values are whatever the untouched buffers hold): which entries
    are called, what backward returns to which input, and that nothing is called for what nobody asks."""
    monkeypatch.setattr(losses, "_hip_path", lambda tensors, c, g: not (c.requires_grad or g.requires_grad))
    monkeypatch.setattr(pf, "_on_hip", lambda camera, gravity, calibration_grad=False:
                        calibration_grad or not (camera._data.requires_grad or gravity._data.requires_grad))
    cam_data, grav_data, up, lat, upc, latc = _host_inputs()
    pred = dict(up_field=up, latitude_field=lat, up_confidence=upc, latitude_confidence=latc)
    launches = lambda: [(n, a) for n, a in rec.calls if not n.endswith("_workspace")]  # noqa: E731
    names = lambda: [n for n, _ in launches()]  # noqa: E731

    def calibration(cam_grad=True, grav_grad=True):
        cam_leaf, grav_leaf = cam_data.clone().requires_grad_(cam_grad), grav_data.clone().requires_grad_(grav_grad)
        cam, grav = camera_models["radial"](cam_leaf), Gravity(grav_data)
        cam._data, grav._data = cam_leaf, grav_leaf
        return cam, grav, cam_leaf, grav_leaf

    cam, grav, cam_leaf, grav_leaf = calibration()
    out = losses.perspective_field_loss(pred, cam, grav, "l2", "huber", calibration_grad=True)
    assert out["perspective_total"].requires_grad and names() == ["gclm_field_loss"]
    out["perspective_total"].sum().backward()
    assert names() == ["gclm_field_loss", "gclm_field_loss_param_grad"]
    assert cam_leaf.grad.shape == (2, 8) and grav_leaf.grad.shape == (2, 3)
    del rec.calls[:]
    cam, grav, cam_leaf, grav_leaf = calibration(cam_grad=False)             # gravity alone, and a field that asks
    leaf = up.clone().requires_grad_(True)
    losses.perspective_field_loss({**pred, "up_field": leaf}, cam, grav, calibration_grad=True)["perspective_total"].sum().backward()
    assert names() == ["gclm_field_loss", "gclm_field_loss_grad", "gclm_field_loss_param_grad"]
    grad_call, param_call = launches()[1][1], launches()[2][1]
    assert grad_call[6:10] == (p(leaf), None, p(upc), None) and param_call[6:10] == (p(leaf), p(lat), p(upc), p(latc))
    assert param_call[15] is None and param_call[16] is not None and cam_leaf.grad is None and grav_leaf.grad.shape == (2, 3)
    assert leaf.grad.shape == up.shape
    del rec.calls[:]
    cam, grav, _, _ = calibration(False, False)                              # nobody asks: the flag adds no launch
    losses.perspective_field_loss({**pred, "up_field": leaf}, cam, grav, calibration_grad=True)["perspective_total"].sum().backward()
    assert names() == ["gclm_field_loss", "gclm_field_loss_grad"]
    del rec.calls[:]
    cam, grav, cam_leaf, grav_leaf = calibration()                           # the rendered fields
    up_f, lat_f = pf.get_perspective_field(cam, grav, calibration_grad=True)
    assert up_f.shape == (2, 2, 2, 2) and lat_f.shape == (2, 1, 2, 2) and up_f.requires_grad and lat_f.requires_grad
    (up_f.sum() + 2 * lat_f.sum()).backward()
    assert names() == ["gclm_perspective_fields", "gclm_perspective_fields_backward"]
    back = rec.calls[-1][1]
    assert back[:7] == (2, p(cam_leaf), p(grav_leaf), 2, 2, 2, 1) and back[7] is not None and back[8] is not None
    assert cam_leaf.grad.shape == (2, 8) and grav_leaf.grad.shape == (2, 3)
    del rec.calls[:]
    cam, grav, cam_leaf, grav_leaf = calibration()
    pf.get_up_field(cam, grav, normalize=False, calibration_grad=True).sum().backward()
    assert names() == ["gclm_perspective_fields", "gclm_perspective_fields_backward"] and rec.calls[-1][1][6:9:2] == (0, None)
    del rec.calls[:]
    pf.get_latitude_field(*calibration()[:2], calibration_grad=True).sum().backward()
    assert rec.calls[-1][1][7] is None and rec.calls[-1][1][8] is not None
    del rec.calls[:]
    with torch.no_grad():                                                    # no graph asked for: the plain render
        assert not pf.get_up_field(*calibration()[:2], calibration_grad=True).requires_grad
    assert names() == ["gclm_perspective_fields"]


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def shifted(t, floats, dev):
    """`t` on the device, in a buffer that starts `floats` floats past an aligned address."""
    flat = torch.empty(t.numel() + floats, dtype=t.dtype, device=dev)
    flat[floats:].copy_(t.reshape(-1))
    return flat[floats:].view(t.shape)


def run_case(c, dev, shift=False, want_cam=True, want_grav=True, images=slice(None)):
    """(grad_cam, grad_grav) of a recorded case from the C entries, through their one-to-one wrappers in fields.py; `shift`
    puts every plane 4 bytes (the interleaved up cotangent 8 bytes) past its alignment: one pixel per lane."""
    tag, model, H, W, name = c
    kind, ul, ll, conf, normalize = gate.parse(name)
    d = gate.inputs(tag, H, W)
    d = {k: shifted(v[images], (2 if k == "gup" else 1) if shift and k not in ("cam", "grav") else 0, dev) for k, v in d.items()}
    if kind == "planes":
        return fields.perspective_fields_backward(model, d["cam"], d["grav"], None if ul is None else d["gup"],
                                                  None if ll is None else d["glat"], normalize, want_cam, want_grav)
    planes = (None if ul is None else d["up"], None if ll is None else d["lat"], d["upc"] if conf and ul is not None else None,
              d["latc"] if conf and ll is not None else None)
    types = (ul or "l1", ll or "l1")
    den = fields.field_loss(model, d["cam"], d["grav"], *planes, *types)[:, 2:]
    scale = gate.grad_output(dev)[images, None] / den          # as _FieldLossFunction.backward forms it (weights 1)
    return fields.field_loss_param_grad(model, d["cam"], d["grav"], scale, *planes, *types, want_cam, want_grav)


def check_case(c, g_cam, g_grav):
    r = gate.ratios(c, g_cam, g_grav)
    gate.report(c, r)
    assert torch.all(g_cam[:, gate.unread_columns(c[1])] == 0), "an entry the formulas never read must be 0"
    assert np.nanmax(r) <= gate.G and not np.isnan(r).any(), r


@pytest.mark.gpu
@pytest.mark.parametrize("c", gate.cases(), ids=gate.case_id)
def test_accuracy_through_the_c_abi(dev, c):
    check_case(c, *run_case(c, dev))


@pytest.mark.gpu
@pytest.mark.parametrize("c", [c for c in gate.cases() if (c[2], c[3]) in (gate.SHAPES[0], gate.SHAPES[2], gate.SHAPES[4]) and
                               c[4] in ("huber-huber-conf", "planes-norm", "l2-l2-conf")], ids=gate.case_id)
def test_accuracy_with_one_pixel_per_lane(dev, c):
    """The planes off their alignment: 5 x 130 walks three tile columns, 6 x 260 five."""
    check_case(c, *run_case(c, dev, shift=True))


BITS = [c for c in gate.cases() if c[4] in ("huber-huber-conf", "cauchy-huber-conf", "planes-norm", "planes-raw") and c[0] in ("pinhole", "simple_divisional")]


@pytest.mark.gpu
@pytest.mark.parametrize("c", BITS, ids=gate.case_id)
def test_bits_are_repeatable_and_independent_of_batch_and_outputs(dev, c):
    g_cam, g_grav = run_case(c, dev)
    again = run_case(c, dev)
    assert torch.equal(g_cam, again[0]) and torch.equal(g_grav, again[1])
    only_cam, none = run_case(c, dev, want_grav=False)
    none2, only_grav = run_case(c, dev, want_cam=False)
    assert none is None and none2 is None and torch.equal(only_cam, g_cam) and torch.equal(only_grav, g_grav)
    for i in range(gate.B):
        one = run_case(c, dev, images=slice(i, i + 1))
        assert torch.equal(one[0][0], g_cam[i]) and torch.equal(one[1][0], g_grav[i]), i


def _device_args(dev, canary):
    """Real buffers for the table of refusals and the canary test: B = 2 images of 48 x 64, outputs and workspace inside
    canary-filled buffers with 64 words either side."""
    B, H, W = SIZES["B"], SIZES["H"], SIZES["W"]
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.rand(*s, generator=g).to(dev)  # noqa: E731
    cam = torch.tensor([[W, H, 60.0, 63.0, 31.4, 23.7, 0.05, 0.0]] * B, device=dev)
    grav = torch.nn.functional.normalize(torch.tensor([[0.1, -0.9, 0.3], [-0.2, -0.9, -0.2]]), dim=-1).to(dev)
    t = dict(cam=cam, grav=grav, up=rnd(B, 2, H, W) - 0.5, lat=rnd(B, 1, H, W) - 0.5, upc=rnd(B, H, W), latc=rnd(B, H, W),
             scale=rnd(B, 2), gup=rnd(B, H, W, 2) - 0.5, glat=rnd(B, H, W) - 0.5)
    ws_bytes = int(_lib.load().gclm_field_param_grad_workspace(B, H, W))
    pad = 64
    guard = {k: torch.full((n + 2 * pad,), canary, dtype=torch.float32, device=dev) for k, n in
             (("gcam", B * 8), ("ggrav", B * 3), ("ws", ws_bytes // 4))}
    a = {k: v.data_ptr() for k, v in t.items()}
    a.update({k: v[pad:].data_ptr() for k, v in guard.items()})
    return {**SIZES, **a, "ws_bytes": ws_bytes}, t, guard, pad


@pytest.mark.gpu
def test_nothing_outside_the_outputs_and_the_told_workspace_is_written(dev):
    canary = -7.25
    for call, drop in ((_loss_call, ()), (_planes_call, ()), (_loss_call, ("gcam",)), (_planes_call, ("ggrav",))):
        a, keep, guard, pad = _device_args(dev, canary)
        for k in drop:
            a[k] = None
        assert a["ws"] % 8 == 0
        assert call(a) == 0
        torch.cuda.synchronize()
        for k, n in (("gcam", a["B"] * 8), ("ggrav", a["B"] * 3), ("ws", a["ws_bytes"] // 4)):
            buf = guard[k]
            assert torch.all(buf[:pad] == canary) and torch.all(buf[pad + n:] == canary), k
            if k in drop:
                assert torch.all(buf == canary), k
            elif k != "ws":
                assert torch.isfinite(buf[pad:pad + n]).all() and not torch.any(buf[pad:pad + n] == canary), k


@pytest.mark.gpu
def test_refused_calls_leave_their_outputs_untouched(dev):
    canary = 3.5
    a, keep, guard, pad = _device_args(dev, canary)
    for call, table in ((_loss_call, BOTH + LOSS), (_planes_call, BOTH + PLANES)):
        for what, change in table:
            assert call({**a, **change(a)}) == -3, what
    torch.cuda.synchronize()
    for k, buf in guard.items():
        assert torch.all(buf == canary), k
    assert _loss_call(a) == 0 and _planes_call(a) == 0          # ... and the unchanged arguments are accepted
    torch.cuda.synchronize()


def _wrapper_call(which, H, W, dev):
    t = gate.inputs("simple_radial", H, W, device=dev)
    if which == "loss":
        scale = torch.tensor([[0.25, -1.5]], device=dev).repeat(gate.B, 1)
        return lambda: fields.field_loss_param_grad("simple_radial", t["cam"], t["grav"], scale, t["up"], t["lat"], t["upc"], t["latc"],
                                                    "l1", "huber")
    return lambda: fields.perspective_fields_backward("simple_radial", t["cam"], t["grav"], t["gup"], t["glat"])


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["loss", "planes"])
def test_results_do_not_depend_on_what_the_workspace_held(monkeypatch, dev, which):
    """gclm_field_loss_param_grad / gclm_perspective_fields_backward on the fixture's 6 x 260 set (five tile columns, the last
    four pixels wide; two tile rows, the last of two rows) with the wrapper's torch.empty workspace holding 0x00 bytes, 0xFF
    bytes, and the records of a call at 67 x 65: the same bits."""
    from workspace_fill import same_bits_whatever_the_memory_held
    same_bits_whatever_the_memory_held(monkeypatch, dev, _wrapper_call(which, 6, 260, dev), _wrapper_call(which, 67, 65, dev))
