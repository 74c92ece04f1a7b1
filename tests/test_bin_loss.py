"""GPU: gclm_bin_loss / gclm_bin_loss_grad behind losses.perspective_bin_loss against the float64 definition on the CPU
(tests/bin_loss_gate.py: inputs, yardstick, units and gates).

1. Targets: the bins the kernel used equal the float64 encode, a neighbouring bin accepted only at the undecided pixels (within
   1e-3 degrees of a boundary), which are at most 1 % of an image per head.
2. Loss and gradients against float64 evaluated with the kernel's own bins, within 4 units (float32), 16-bit gradients within
   one ulp of the dtype on top; the hit counts exact.
3. Structure: an image's bits do not depend on its batch; the 16-byte and the one-pixel path agree bit for bit; canary-filled
   outputs and workspace are untouched outside what was passed; an absent head has no gradient; nothing of the logits' size is
   allocated beside the gradients.

Measured on an MI355X, over the sixteen cases and their heads (MEASURED below; the test prints every figure with -s): the loss
within 0.54 units (median 0.21; gate 4), float32 gradients within 0.54 units (median 0.41; gate 4), 16-bit gradients within 0.50
of their bound (median 0.50: the rounding's half ulp; bound 1).  The units are the float32 CPU composition's own errors or
their floors: 2.0e-7 .. 7.8e-7 of the loss, 9.2e-7 .. 3.7e-6 of the gradient's max-norm.  No case has a wrong bin; at most 0.52 % of an
image's pixels are undecided."""
import pytest
import torch

import bin_loss_gate as bg
from geocalib_amd import Gravity, _call, _lib, fields, losses
from geocalib_amd.camera import camera_models

pytestmark = pytest.mark.gpu

# (worst, median) ratio to the unit over the sixteen cases, as test_loss_and_gradients_within_the_gate prints them (-s)
MEASURED = {"loss": (0.54, 0.21), "grad": (0.54, 0.41), "grad_ulp": (0.50, 0.50)}


def device():
    return torch.device("cuda", torch.cuda.current_device())


def on_device(case, offset_bytes=0):
    """The case's inputs on the device: (cam (B, 8), grav (B, 3), {head: logits}, {head: confidence or None}).  `offset_bytes`
    places every logit tensor that far behind a 16-byte boundary."""
    inp, dev = bg.inputs(case), device()
    logits, confs = {}, {}
    for n in bg.heads_of(case):
        z = inp["pred"][f"{n}_logits"]
        k = offset_bytes // z.element_size()
        buf = torch.empty(z.numel() + 16, dtype=z.dtype, device=dev)
        assert buf.data_ptr() % 16 == 0
        logits[n] = buf[k:k + z.numel()].view(z.shape).copy_(z)
        c = inp["pred"].get(f"{n}_confidence")
        confs[n] = None if c is None else c.to(dev)
    return inp["cams"].to(dev), inp["gravs"].to(dev), logits, confs


def forward(case, offset_bytes=0):
    cam, grav, logits, confs = on_device(case, offset_bytes)
    out, lse, bins = fields.bin_loss(case[0], cam, grav, logits.get("up"), logits.get("latitude"), confs.get("up"), confs.get("latitude"))
    return out, lse, bins, logits, confs


def public(case, batch=slice(None), offset_bytes=0):
    """losses.perspective_bin_loss on the device inputs of images `batch`, and the gradients of sum_b GOUT[b] perspective_total."""
    cam, grav, logits, confs = on_device(case, offset_bytes)
    camera, gravity = camera_models[case[0]](cam[batch]), Gravity(grav[batch])
    gravity._data = grav[batch]
    pred = {f"{n}_logits": z[batch].detach().requires_grad_(True) for n, z in logits.items()}
    pred.update({f"{n}_confidence": c[batch] for n, c in confs.items() if c is not None})
    out = losses.perspective_bin_loss(pred, camera, gravity, up_loss_weight=bg.WEIGHTS["up"], latitude_loss_weight=bg.WEIGHTS["latitude"])
    gout = torch.tensor(bg.GOUT, device=cam.device)[batch]
    (gout * out["perspective_total"]).sum().backward()
    return out, {n: pred[f"{n}_logits"].grad for n in logits}


@pytest.mark.parametrize("case", bg.CASES, ids=bg.case_id)
def test_target_bins_equal_the_float64_encode_off_the_undecided_pixels(case):
    out, lse, bins, _, _ = forward(case)
    for i, n in enumerate(bg.HEADS):
        if n not in bg.heads_of(case):
            assert out[:, 3 * i:3 * i + 3].isnan().all()
            continue
        wrong, undecided = bg.bins_verdict(case, n, bins[:, i])
        print(bg.case_id(case), n, "wrong", wrong, "undecided share", undecided)
        assert undecided <= 0.01, (n, undecided)
        assert wrong == 0, (n, wrong)


RATIOS = {"loss": [], "grad": [], "grad_ulp": []}


@pytest.mark.parametrize("case", bg.CASES, ids=bg.case_id)
def test_loss_and_gradients_within_the_gate(case):
    raw, lse, bins, _, _ = forward(case)
    out, grads = public(case)
    heads = bg.heads_of(case)
    assert set(out) == {"perspective_total"} | {k.format(n) for n in heads for k in ("{}-classification-loss", "{}_total", "{}_bin_accuracy")}
    kernel_bins = {n: bins[:, bg.HEADS.index(n)].cpu() for n in heads}
    y64, u = bg.units(case, kernel_bins)
    H, W = case[1:3]
    for n in heads:
        i = bg.HEADS.index(n)
        v = bg.verdict(case, y64, u, n, out[f"{n}_total"], grads[n])
        gmax = y64["grad"][n].abs().flatten(1).max(1).values.clamp(min=1e-300)
        rel = {"loss": (u["loss"][n] / y64["loss"][n].abs().clamp(min=1e-300)).max().item(), "grad": (u["grad"][n] / gmax).max().item()}
        print(bg.case_id(case), n, {k: f"{x:.3f}" for k, x in v.items()}, "relative units", {k: f"{x:.2e}" for k, x in rel.items()})
        RATIOS["loss"].append(v["loss"])
        RATIOS["grad" if case[5] == torch.float32 else "grad_ulp"].append(v["grad"] if case[5] == torch.float32 else v["grad_ulp"])
        assert bg.passes(v), (n, v)
        assert grads[n].dtype == case[5] and grads[n].shape == bg.inputs(case)["pred"][f"{n}_logits"].shape
        # the public loss is the kernel's numerator over its denominator, times the weight; the hits are exact
        assert torch.equal(out[f"{n}_total"], raw[:, 3 * i] / raw[:, 3 * i + 1] * bg.WEIGHTS[n])
        assert torch.equal(raw[:, 3 * i + 2].cpu().long(), y64["hits"][n])
        assert torch.equal(out[f"{n}_bin_accuracy"], raw[:, 3 * i + 2] / (H * W)) and not out[f"{n}_bin_accuracy"].requires_grad
        # lse is the float64 one to float32 rounding and the exp's ulp
        assert ((lse[:, i].double().cpu() - y64["lse"][n]).abs() <= 2.0 ** -21 * y64["lse"][n].abs().clamp(min=1)).all()
    if case == bg.CASES[-1]:
        import statistics
        print({k: (f"worst {max(x):.2f}", f"median {statistics.median(x):.2f}") for k, x in RATIOS.items() if x})


@pytest.mark.parametrize("case", [bg.CASES[1], bg.CASES[4], bg.CASES[2]], ids=bg.case_id)
def test_an_image_gets_the_bits_it_gets_alone(case):
    out, grads = public(case)
    for b in range(bg.B):
        one, g1 = public(case, slice(b, b + 1))
        for k in out:
            assert torch.equal(out[k][b:b + 1], one[k]), (b, k)
        for n in grads:
            assert torch.equal(grads[n][b:b + 1].view(torch.uint8), g1[n].view(torch.uint8)), (b, n)


@pytest.mark.parametrize("case", [bg.CASES[1], bg.CASES[6], bg.CASES[11]], ids=bg.case_id)
def test_vector_and_scalar_paths_agree_bit_for_bit(case):
    """24 x 40 admits 4 and 8 pixels per lane; logits 4 bytes behind a 16-byte boundary take one pixel per lane."""
    raw, lse, bins, logits, _ = forward(case)
    raw1, lse1, bins1, logits1, _ = forward(case, offset_bytes=4)
    assert all(z.data_ptr() % 16 == 0 for z in logits.values()) and all(z.data_ptr() % 16 == 4 for z in logits1.values())
    assert torch.equal(raw.view(torch.int32), raw1.view(torch.int32))
    assert torch.equal(lse.view(torch.int32), lse1.view(torch.int32)) and torch.equal(bins, bins1)
    (out, grads), (out1, grads1) = public(case), public(case, offset_bytes=4)
    for k in out:
        assert torch.equal(out[k], out1[k]), k
    for n in grads:
        assert torch.equal(grads[n].view(torch.uint8), grads1[n].view(torch.uint8)), n


CANARY = 0x5A


@pytest.mark.parametrize("case,heads", [(bg.CASES[0], "both"), (bg.CASES[1], "up"), (bg.CASES[6], "latitude"), (bg.CASES[4], "both")],
                         ids=lambda v: v if isinstance(v, str) else bg.case_id(v))
def test_canaries_outside_what_was_passed_stay(case, heads):
    """Both calls over the C ABI with caller-made buffers: d_out, d_lse, d_bins, the workspace and the gradients each lie in a
    canary-filled buffer with a margin either side, the workspace longer than the call is told.  With one head alone the other
    head's planes of d_lse and d_bins, and its gradient buffer, keep their canaries too."""
    cam, grav, logits, confs = on_device(case)
    model, H, W, Ku, Kl, dtype = case[:6]
    dev, B = cam.device, bg.B
    use = bg.HEADS if heads == "both" else (heads,)
    z = {n: logits[n] if n in use else None for n in bg.HEADS}
    c = {n: confs.get(n) if n in use else None for n in bg.HEADS}
    ws_bytes = int(_lib.load().gclm_bin_loss_workspace(B, H, W))
    margin = 256

    def canaried(nbytes):
        buf = torch.full((nbytes + 2 * margin,), CANARY, dtype=torch.uint8, device=dev)
        return buf, buf[margin:margin + nbytes]

    esize = logits[bg.heads_of(case)[0]].element_size()
    bufs = {"out": canaried(B * 6 * 4), "lse": canaried(B * 2 * H * W * 4), "bins": canaried(B * 2 * H * W * 2), "ws": canaried(ws_bytes + 512),
            "g_up": canaried(B * Ku * H * W * esize), "g_latitude": canaried(B * Kl * H * W * esize), "scale": canaried(B * 2 * 4)}
    p = {k: v[1].data_ptr() for k, v in bufs.items()}
    bufs["scale"][1].view(torch.float32).copy_(torch.tensor([[0.5, -0.25]] * B).flatten())
    dt = _lib.LOGIT_DTYPE_IDS[str(dtype).split(".")[-1]]
    stream = _call.raw_stream(dev)
    _call.call("gclm_bin_loss", _lib.CAMERA_MODEL_IDS[model], cam.data_ptr(), grav.data_ptr(), B, H, W, _call.ptr(z["up"]), Ku,
               _call.ptr(z["latitude"]), Kl, dt, _call.ptr(c["up"]), _call.ptr(c["latitude"]), p["ws"], ws_bytes, p["out"], p["lse"],
               p["bins"], stream, device=dev)
    _call.call("gclm_bin_loss_grad", _call.ptr(z["up"]), Ku, _call.ptr(z["latitude"]), Kl, dt, _call.ptr(c["up"]), _call.ptr(c["latitude"]),
               B, H, W, p["lse"], p["bins"], p["scale"], p["g_up"] if "up" in use else None, p["g_latitude"] if "latitude" in use else None,
               stream, device=dev)
    torch.cuda.synchronize()
    for k, (buf, inner) in bufs.items():
        assert (buf[:margin] == CANARY).all() and (buf[margin + inner.numel():] == CANARY).all(), k
    assert (bufs["ws"][1][ws_bytes:] == CANARY).all()
    lse, bins = bufs["lse"][1].view(B, 2, H * W * 4), bufs["bins"][1].view(B, 2, H * W * 2)
    for i, n in enumerate(bg.HEADS):
        if n not in use:
            assert (lse[:, i] == CANARY).all() and (bins[:, i] == CANARY).all() and (bufs[f"g_{n}"][1] == CANARY).all(), n
            assert bufs["out"][1].view(torch.float32).view(B, 6)[:, 3 * i:3 * i + 3].isnan().all()
        else:
            assert not (bufs[f"g_{n}"][1].view(-1, 4)[:, :] == CANARY).all(1).any(), n     # every gradient word was written
    # what was written is what the package's call writes
    out, lse_ref, bins_ref = fields.bin_loss(model, cam, grav, z["up"], z["latitude"], c["up"], c["latitude"])
    assert torch.equal(bufs["out"][1].view(torch.int32), out.view(torch.int32).flatten())
    for i, n in enumerate(bg.HEADS):
        if n in use:
            assert torch.equal(lse[:, i].contiguous().view(torch.int32), lse_ref[:, i].contiguous().view(torch.int32).view(B, -1))


def test_an_absent_head_has_no_gradient_and_the_camera_may_require_grad():
    case = bg.CASES[1]
    cam, grav, logits, confs = on_device(case)
    camera, gravity = camera_models[case[0]](cam.clone().requires_grad_(True)), Gravity(grav)
    gravity._data = grav.clone().requires_grad_(True)
    up = logits["up"].detach().requires_grad_(True)
    lat = logits["latitude"].detach().requires_grad_(True)
    out = losses.perspective_bin_loss({"up_logits": up, "latitude_logits": lat.detach()}, camera, gravity)
    assert out["up_total"].requires_grad
    out["perspective_total"].sum().backward()
    assert up.grad is not None and lat.grad is None and camera._data.grad is None and gravity._data.grad is None
    # the same gradient as with both heads asking
    both = losses.perspective_bin_loss({"up_logits": up.detach().requires_grad_(True), "latitude_logits": lat}, camera, gravity)
    assert torch.equal(both["up_total"], out["up_total"]) and torch.equal(both["latitude_total"], out["latitude_total"])
    # one head alone: the other head's keys are absent
    alone = losses.perspective_bin_loss({"latitude_logits": lat}, camera, gravity)
    assert set(alone) == {"latitude-classification-loss", "latitude_total", "latitude_bin_accuracy", "perspective_total"}
    assert torch.equal(alone["latitude_total"], out["latitude_total"])
    assert fields.bin_loss_grad(torch.ones(bg.B, 2, device=cam.device), *fields.bin_loss(case[0], cam, grav, up.detach(), lat.detach())[1:],
                                None, lat.detach())[0] is None


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_nothing_of_the_logits_size_is_allocated(dtype):
    """Peak memory of forward + backward stays below inputs + gradients + 12 B per pixel (lse, bins) + workspace + 10 % of the
    logits' bytes."""
    dev, (B, Ku, Kl, H, W) = device(), (4, 73, 180, 96, 128)
    cams, gravs = bg.calibration("simple_radial", H, W, 12)
    cam, grav = cams.repeat(2, 1)[:B].to(dev), gravs.repeat(2, 1)[:B].to(dev)
    g = torch.Generator(device="cpu").manual_seed(3)
    up = torch.randn(B, Ku, H, W, generator=g).to(dev, dtype).requires_grad_(True)
    lat = torch.randn(B, Kl, H, W, generator=g).to(dev, dtype).requires_grad_(True)
    conf = torch.rand(B, H, W, generator=g).to(dev)
    camera, gravity = camera_models["simple_radial"](cam), Gravity(grav)
    gravity._data = grav
    pred = {"up_logits": up, "latitude_logits": lat, "up_confidence": conf, "latitude_confidence": conf}
    losses.perspective_bin_loss(pred, camera, gravity)["perspective_total"].sum().backward()      # (warm: tables, the library)
    up.grad = lat.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    losses.perspective_bin_loss(pred, camera, gravity)["perspective_total"].sum().backward()
    torch.cuda.synchronize()
    logit_bytes = up.numel() * up.element_size() + lat.numel() * lat.element_size()
    ws_bytes = int(_lib.load().gclm_bin_loss_workspace(B, H, W))
    extra = torch.cuda.max_memory_allocated() - before
    bound = logit_bytes + 12 * B * H * W + ws_bytes + 0.1 * logit_bytes       # (the inputs are in `before`)
    print("extra", extra, "bound", bound, "gradients", logit_bytes)
    assert up.grad is not None and lat.grad is not None and extra <= bound, (extra, bound)
