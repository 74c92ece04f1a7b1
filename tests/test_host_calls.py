"""CPU: the one call path from the Python package to the C ABI (geocalib_amd/_call.py).  The library is replaced by a
recorder and the one device check by a no-op, so no kernel runs: every stateless wrapper hands its C entry the arguments of
include/gclm.h in order (stream last), batches beyond one call are sliced with the pointers advanced, the HIP device is
switched only for a stateless entry on another device, and a failure's text carries a handle's message and never a stale one."""
import ctypes as C

import pytest
import torch

from geocalib_amd import _call, _lib, fields, lm_optimizer, perspective_fields, synth
from geocalib_amd.camera import camera_models
from geocalib_amd.gravity import Gravity
from geocalib_amd.lm_optimizer import LMOptimizer

STREAM = 0x5EED
MAX = 65535


class _Rec:
    """Stands in for the loaded library: records every gclm_* call (ctypes arrays as lists) and returns `rc`."""

    def __init__(self):
        self.calls, self.rc = [], 0

    def __getattr__(self, name):
        if name == "gclm_last_error":
            return lambda h: b"text of the handle"
        if name == "gclm_comm_last_error":
            return lambda c: b"text of the communicator"
        if not name.startswith("gclm_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, tuple(list(a) if isinstance(a, C.Array) else a for a in args)))
            return self.rc
        return fn


@pytest.fixture
def rec(monkeypatch):
    r = _Rec()
    r.entered = []

    class Device:
        def __init__(self, device):
            self.device = device

        def __enter__(self):
            r.entered.append(self.device)

        def __exit__(self, *exc):
            return False

    monkeypatch.setattr(_lib, "load", lambda: r)
    monkeypatch.setattr(_call, "require_device", lambda t, name: None)
    monkeypatch.setattr(_call, "raw_stream", lambda device: STREAM)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "device", Device)
    return r


def _cameras(B, size=2.0):
    cam = torch.tensor([[size, size, 1.5, 1.5, size / 2, size / 2, 0.05, 0.0]]).repeat(B, 1)
    grav = torch.tensor([[0.0, 1.0, 0.0]]).repeat(B, 1)
    return cam, grav


def _data(B=2, H=2, W=2):
    g = torch.Generator().manual_seed(0)
    return {"up_field": torch.randn(B, 2, H, W, generator=g), "latitude_field": torch.rand(B, 1, H, W, generator=g) - 0.5,
            "up_confidence": torch.rand(B, H, W, generator=g), "latitude_confidence": torch.rand(B, H, W, generator=g)}


def p(t):
    return t.data_ptr()


# ------------------------------------------------------------------ arguments, in the order of include/gclm.h

@pytest.mark.parametrize("sin_latitude", [False, True])
def test_pack_fields(rec, sin_latitude):
    up_raw, lat_raw, ulc, llc = torch.randn(2, 2, 2, 2), torch.randn(2, 1, 2, 2), torch.randn(2, 2, 2), torch.randn(2, 1, 2, 2)
    out = fields.pack_fields(up_raw, lat_raw, ulc, llc, sin_latitude=sin_latitude)
    assert ("sin_latitude" in out) == sin_latitude
    assert rec.calls == [("gclm_pack_fields_ex", (
        p(up_raw), p(ulc), p(lat_raw), p(llc), 2, 2, 2, p(out["up_field"]), p(out["up_confidence"]), p(out["latitude_field"]),
        p(out["latitude_confidence"]), p(out["sin_latitude"]) if sin_latitude else None, STREAM))]
    assert not rec.entered


def test_pack_fields_without_confidences_passes_null(rec):
    up_raw, lat_raw = torch.randn(2, 2, 2, 2), torch.randn(2, 1, 2, 2)
    out = fields.pack_fields(up_raw, lat_raw)
    assert rec.calls == [("gclm_pack_fields_ex", (p(up_raw), None, p(lat_raw), None, 2, 2, 2, p(out["up_field"]), None,
                                                  p(out["latitude_field"]), None, None, STREAM))]


def test_upsample_fields(rec):
    src = torch.randn(2, 2, 2, 2)
    dst = fields.upsample_fields(src, (4, 4))
    assert dst.shape == (2, 2, 4, 4)
    assert rec.calls == [("gclm_upsample_fields", (p(src), 4, 2, 2, 4, 4, p(dst), STREAM))]


def test_upsample_fields_multi(rec):
    a, b = torch.randn(2, 2, 2, 2), torch.randn(2, 1, 2, 2)
    oa, ob = fields.upsample_fields_multi([a, b], (4, 4))
    assert oa.shape == (2, 2, 4, 4) and ob.shape == (2, 1, 4, 4)
    assert rec.calls == [("gclm_upsample_fields_multi", ([p(a), p(b)], [p(oa), p(ob)], [4, 2], 2, 2, 2, 4, 4, STREAM))]


def test_undistort_image(rec):
    cam, _ = _cameras(2)
    img = torch.rand(2, 1, 2, 2)
    dst = fields.undistort_image("radial", cam, img, (2, 2))
    assert rec.calls == [("gclm_undistort_image", (2, p(cam), 2, p(img), 2, 1, 2, 2, 2, 2, p(dst), STREAM))]


def _byte_images():
    """(image, layout flag): a contiguous uint8 image and a channels_last one of C = 3, which the wrappers read as it lies."""
    planar = torch.randint(0, 256, (2, 3, 2, 2), dtype=torch.uint8)
    return [(planar, 0), (planar.contiguous(memory_format=torch.channels_last), 1)]


def test_undistort_image_picks_the_byte_entry_and_its_layout_flag(rec):
    cam, _ = _cameras(2)
    for img, interleaved in _byte_images():
        del rec.calls[:]
        dst = fields.undistort_image("radial", cam, img, (2, 2))
        assert rec.calls == [("gclm_undistort_image_u8", (2, p(cam), 2, p(img), 2, 3, 2, 2, 2, 2, interleaved, p(dst), STREAM))]
        assert dst.dtype == torch.uint8 and dst.shape == (2, 3, 2, 2) and dst.stride() == img.stride()
    with pytest.raises(RuntimeError):
        fields.undistort_image("radial", cam, torch.zeros(2, 3, 2, 2, dtype=torch.float64), (2, 2))


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
def test_undistort_image_hands_over_the_camera_rows_it_has_for_the_entry_to_refuse(rec, dtype):
    """A camera batch that is neither 1 nor B reaches the entry as the number of rows behind the pointer, never as the image
    count: the entry refuses cam_batch != 1, B (tests/test_undistort_abi.py, test_u8_image_abi.py), and the refusal surfaces."""
    cam, _ = _cameras(2)
    img = torch.zeros(4, 1, 2, 2, dtype=dtype)
    rec.rc = -3
    with pytest.raises(_lib.GclmError, match=r"gclm_undistort_image\w* failed \(-3\)"):
        fields.undistort_image("radial", cam, img, (2, 2))
    (_, args), = rec.calls
    assert args[:5] == (2, p(cam), 2, p(img), 4)


def test_reproject_image_picks_the_entry_of_the_dtype_and_its_layout_flag(rec):
    cam, _ = _cameras(2)
    rot = torch.eye(3).repeat(2, 1, 1)
    img = torch.rand(2, 3, 2, 2)
    dst, valid = fields.reproject_image("radial", cam, "pinhole", cam[:, :], rot[:1], img, (2, 2), (2, 2), return_valid=True)
    (name, args), = rec.calls
    assert name == "gclm_reproject_image" and args[:7] == (2, p(cam), 0, p(cam), 2, p(rot), 1)
    assert args[7:] == (p(img), 2, 3, 2, 2, 2, 2, 2, 2, p(dst), args[-2], STREAM) and valid.dtype == torch.bool
    for img, interleaved in _byte_images():
        del rec.calls[:]
        dst = fields.reproject_image("radial", cam[:1], "pinhole", cam[:1], None, img, (2, 2), (2, 2))
        assert rec.calls == [("gclm_reproject_image_u8", (2, p(cam), 0, p(cam), 1, None, 1, p(img), 2, 3, 2, 2, 2, 2, 2, 2,
                                                          interleaved, p(dst), None, STREAM))]
        assert dst.dtype == torch.uint8 and dst.stride() == img.stride()
    with pytest.raises(RuntimeError):
        fields.reproject_image("radial", cam, "pinhole", cam, None, torch.zeros(2, 3, 2, 2, dtype=torch.int16), (2, 2), (2, 2))
    with pytest.raises(ValueError, match="camera batches 2 and 1 must be equal and, as the rotation batch None, 1 or 2"):
        fields.reproject_image("radial", cam, "pinhole", cam[:1], None, img, (2, 2), (2, 2))


def test_render_from_pano(rec):
    cam, _ = _cameras(2)
    rot, pano = torch.eye(3).repeat(2, 1, 1), torch.rand(1, 2, 2)
    dst = fields.render_from_pano("pinhole", cam, rot, [pano, pano], (2, 2))
    assert rec.calls == [("gclm_render_from_pano", (0, p(cam), 2, p(rot), [p(pano)] * 2, [2, 2, 2, 2], 2, 1, 2, 2, p(dst),
                                                    STREAM))]


def test_perspective_fields(rec):
    cam, grav = _cameras(2)
    up, lat = fields.perspective_fields("simple_radial", cam, grav, (2, 2))
    assert rec.calls == [("gclm_perspective_fields", (1, p(cam), p(grav), 2, 2, 2, 1, p(up), p(lat), STREAM))]
    only_lat = fields.perspective_fields("simple_radial", cam, grav, (2, 2), up=False, normalize=False)
    assert only_lat[0] is None
    assert rec.calls[1] == ("gclm_perspective_fields", (1, p(cam), p(grav), 2, 2, 2, 0, None, p(only_lat[1]), STREAM))


def test_jacobian_fields(rec):
    cam, grav = _cameras(2)
    camera, gravity = camera_models["simple_radial"](cam), Gravity(grav)
    J_up, J_lat = perspective_fields._jacobian_fields(camera, gravity, True, False, True, True)
    assert J_up.shape == (2, 2, 2, 2, 4) and J_lat.shape == (2, 2, 2, 1, 4)
    assert rec.calls == [("gclm_jacobian_fields", (1, p(camera._data), p(gravity._data), 2, 2, 2, 1, 0, p(J_up), p(J_lat),
                                                   STREAM))]
    none, J_lat = perspective_fields._jacobian_fields(camera, gravity, False, True, False, True)
    assert none is None
    assert rec.calls[1][1] == (1, p(camera._data), p(gravity._data), 2, 2, 2, 0, 1, None, p(J_lat), STREAM)


def test_synth_fields(rec):
    d, gt_cam, gt_grav = synth.synth_fields("pinhole", 2, 2, 2, "cpu", seed=3, first_index=5, noise=0.5, group_size=2, run=1,
                                            run_stride=4)
    assert rec.calls == [("gclm_synth_fields_grouped", (
        0, 3, 5, 2, 2, 2, 0.5, 2, 1, 4, p(d["up_field"]), p(d["latitude_field"]), p(d["up_confidence"]),
        p(d["latitude_confidence"]), p(gt_cam), p(gt_grav), STREAM))]
    d, gt_cam, gt_grav = synth.synth_fields("radial", 2, 2, 2, "cpu", confidences=False)
    assert rec.calls[1][1] == (2, 0, 0, 2, 2, 2, 0.02, 1, 0, 0, p(d["up_field"]), p(d["latitude_field"]), None, None, p(gt_cam),
                               p(gt_grav), STREAM)


def test_huber_loss(rec):
    x = torch.rand(5)
    loss, d1, d2 = lm_optimizer.huber_loss(x)
    assert rec.calls == [("gclm_huber_costs", (p(x), 5, 0, 1.0, None, p(loss), p(d1), p(d2), STREAM))]


def test_optimizer_step(rec):
    G, H, lam = torch.rand(2, 3), torch.rand(2, 3, 3), torch.rand(2)
    delta = lm_optimizer.optimizer_step(G, H, lam)
    assert delta.shape == G.shape
    assert rec.calls == [("gclm_optimizer_step", (p(G), p(H), p(lam), 0, 1e-6, 2, 3, p(delta), None, STREAM))]


def test_calculate_residuals_costs_and_gradient(rec):
    cam, grav = _cameras(2)
    camera, gravity = camera_models["pinhole"](cam), Gravity(grav)
    data = _data()
    opt = LMOptimizer({"camera_model": "pinhole"})
    res = opt.calculate_residuals(camera, gravity, data)
    assert res["up_residual"].shape == (2, 4, 2) and res["latitude_residual"].shape == (2, 4, 1)
    assert rec.calls == [("gclm_residual_fields", (
        0, p(data["up_field"]), p(data["latitude_field"]), p(camera._data), p(gravity._data), 2, 2, 2, p(res["up_residual"]),
        p(res["latitude_residual"]), STREAM))]
    del rec.calls[:]
    costs, weights = opt.calculate_costs(res, data)
    assert rec.calls == [
        ("gclm_huber_costs", (p(res["up_residual"]), 8, 2, 1e-2, p(data["up_confidence"]), p(costs["up_cost"]),
                              p(weights["up_weights"]), None, STREAM)),
        ("gclm_huber_costs", (p(res["latitude_residual"]), 8, 1, 1e-2, p(data["latitude_confidence"]),
                              p(costs["latitude_cost"]), p(weights["latitude_weights"]), None, STREAM))]
    del rec.calls[:]
    J = torch.rand(2, 4, 2, 3)
    Grad, Hess = opt.calculate_gradient_and_hessian(J, res["up_residual"], weights["up_weights"])
    (name, args), = rec.calls
    # the Jacobian goes in as a gathered copy of its free columns: a pointer of its own, not the caller's tensor
    assert isinstance(args[0], int) and args[0] != p(J)
    assert (name, args[1:]) == ("gclm_gradient_hessian", (p(res["up_residual"]), p(weights["up_weights"]), 2, 4, 2, 3, 0, p(Grad),
                                                          p(Hess), STREAM))
    assert not rec.entered


# ------------------------------------------------------------------ slicing at the per-call image limit

def test_the_limit_has_one_definition():
    assert _call.MAX_CALL == LMOptimizer._MAX_CALL == MAX
    assert list(_call.slices(MAX + 3)) == [(0, MAX), (MAX, 3)]
    assert list(_call.slices(MAX)) == [(0, MAX)] and list(_call.slices(0)) == []


def test_perspective_fields_slices_and_advances_every_pointer(rec):
    cam, grav = _cameras(MAX + 3, size=1.0)
    up, lat = fields.perspective_fields("pinhole", cam, grav, (1, 1))
    first, second = (a for _, a in rec.calls)
    assert first == (0, p(cam), p(grav), MAX, 1, 1, 1, p(up), p(lat), STREAM)
    assert second == (0, p(cam) + MAX * 8 * 4, p(grav) + MAX * 3 * 4, 3, 1, 1, 1, p(up) + MAX * 2 * 4, p(lat) + MAX * 4, STREAM)


def test_undistort_image_slices_per_image_and_shared_cameras(rec):
    cam, _ = _cameras(MAX + 3)
    img = torch.zeros(MAX + 3, 1, 2, 2)
    dst = fields.undistort_image("radial", cam, img, (2, 2))
    step = MAX * 4 * 4
    assert [a for _, a in rec.calls] == [(2, p(cam), MAX, p(img), MAX, 1, 2, 2, 2, 2, p(dst), STREAM),
                                         (2, p(cam) + MAX * 8 * 4, 3, p(img) + step, 3, 1, 2, 2, 2, 2, p(dst) + step, STREAM)]
    del rec.calls[:]
    dst = fields.undistort_image("radial", cam[:1], img, (2, 2))
    assert [a for _, a in rec.calls] == [(2, p(cam), 1, p(img), MAX, 1, 2, 2, 2, 2, p(dst), STREAM),
                                         (2, p(cam), 1, p(img) + step, 3, 1, 2, 2, 2, 2, p(dst) + step, STREAM)]


def test_render_from_pano_slices_the_pointer_and_size_arrays(rec):
    n = MAX + 3
    cam, _ = _cameras(1)
    rot, pano = torch.eye(3).repeat(n, 1, 1), torch.zeros(1, 2, 2)
    dst = fields.render_from_pano("pinhole", cam, rot, [pano] * n, (2, 2))
    first, second = (a for _, a in rec.calls)
    assert first == (0, p(cam), 1, p(rot), [p(pano)] * MAX, [2] * (2 * MAX), MAX, 1, 2, 2, p(dst), STREAM)
    assert second == (0, p(cam), 1, p(rot) + MAX * 9 * 4, [p(pano)] * 3, [2] * 6, 3, 1, 2, 2, p(dst) + MAX * 4 * 4, STREAM)


# ------------------------------------------------------------------ which HIP device the launch goes to

def test_a_stateless_call_switches_only_to_another_device(rec):
    _call.call("gclm_upsample_fields", 1, 2, device=torch.device("cuda", 0))
    assert rec.entered == []
    _call.call("gclm_upsample_fields", 1, 2, device=torch.device("cuda", 1))
    assert rec.entered == [torch.device("cuda", 1)]
    assert rec.calls == [("gclm_upsample_fields", (1, 2))] * 2


def test_a_handle_or_communicator_call_never_switches(rec):
    h = C.c_void_p(1)
    for index in (0, 1):
        _call.call("gclm_shared_finish", h, 2, 3, handle=h, device=torch.device("cuda", index))
        _call.call("gclm_comm_all_reduce_sum", h, 2, 3, 4, comm=h, device=torch.device("cuda", index))
    assert rec.entered == [] and len(rec.calls) == 4


# ------------------------------------------------------------------ how a non-zero return becomes an exception

def test_a_failure_names_the_function_and_the_code_and_only_a_handle_adds_text(rec):
    rec.rc = -3
    with pytest.raises(_lib.GclmError) as e:
        _call.call("gclm_upsample_fields", 1, 2, device=torch.device("cuda", 0))
    assert str(e.value) == "gclm_upsample_fields failed (-3)"
    h = C.c_void_p(1)
    with pytest.raises(_lib.GclmError) as e:
        _call.call("gclm_shared_finish", h, 2, 3, handle=h)
    assert str(e.value) == "gclm_shared_finish failed (-3): text of the handle"
    with pytest.raises(_lib.GclmError) as e:
        _call.call("gclm_comm_all_reduce_sum", h, 2, 3, 4, comm=h)
    assert str(e.value) == "gclm_comm_all_reduce_sum failed (-3): text of the communicator"
    with pytest.raises(_lib.GclmError, match=r"gclm_huber_costs failed \(-3\)$"):      # ... and through a wrapper
        lm_optimizer.huber_loss(torch.rand(3))


def test_a_stateless_failure_does_not_quote_the_last_failed_create(monkeypatch):
    """The real library: without a handle gclm_last_error returns the thread's last failed gclm_create."""
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    cfg = _lib.GclmConfig.default(0)
    cfg.camera_model = 99
    h = C.c_void_p()
    with pytest.raises(_lib.GclmError) as e:
        _call.call("gclm_create", C.byref(h), C.byref(cfg))
    stale = _lib.last_error(None)
    assert stale.startswith("gclm_create") and str(e.value) == f"gclm_create failed (-2): {stale}"      # its own message
    # B = 0 is refused before any HIP call; the addresses are never dereferenced
    with pytest.raises(_lib.GclmError) as e:
        _call.call("gclm_undistort_image", 1, 0x100000, 1, 0x200000, 0, 3, 48, 64, 48, 64, 0x4000000, None,
                   device=torch.device("cuda", 0))
    assert str(e.value) == "gclm_undistort_image failed (-3)" and stale not in str(e.value)


def test_the_device_check_names_the_tensor():
    with pytest.raises(RuntimeError, match="`up_raw` must live on a HIP device .* no CPU fallback"):
        fields.pack_fields(torch.zeros(1, 2, 2, 2), torch.zeros(1, 1, 2, 2))
    assert _call.ptr(None) is None
