"""Writes tests/golden/field_calib_grad_reference.npz: the gradients of the decoders' losses, and of linear functions of the
rendered fields, with respect to the camera data and the gravity vector, as the reference gets them from autograd through its
own get_perspective_field / get_up_field / get_latitude_field and UpDecoder / LatitudeDecoder.calculate_losses.  Data only.

Per (camera model, shape) one set of inputs, B = 3 images: cameras (fx != fy, the principal point off the pixel grid) and
gravities (c of either sign) as float32; predictions = the float64 fields of a perturbed calibration (field_error_gate's
perturbation, a quarter of it) plus uniform noise of +-0.02, rounded to multiples of 2^-12 and stored as those integers
(exact in float32; the residuals straddle Huber's delta = 1 degree); confidences k / 8, k = 1..7, stored as k; cotangent
planes k / 4, k = -4..4, stored as k.  Per case (a pair of loss types with or without confidences, one field alone, or
the plane-cotangent form with normalize on or off), for the sum over images of GOUT[b] x loss[b] (planes: sum of
cotangent x field):
one float64 array (3, 3, 11): per image, three rows over the 8 entries of the camera data and the 3 of the gravity vector --
    row 0   the gradients in float64 autograd of the reference
    row 1   the same in float32
    row 2   A: per entry, the sum over pixels of |that pixel's contribution| in float64 (the pixel's target cotangent times the
            forward-mode derivative of the reference's fields)
The gravity vector is the reference Gravity's data as stored (its constructor's normalisation is bypassed: the HIP kernels use
gravity as stored).  The conditions the inputs must meet are asserted here (check_conditions) and again, on the committed
file, by tests/test_field_calib_grad_abi.py.

Runs where a checkout of the reference is available (oracle/ref_import.py says where).

    python tests/golden/make_golden_field_calib_grad.py
"""
import importlib.util
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import ref_import  # noqa: E402
import perspective_gate as pg  # noqa: E402

B = 3
GOUT = (0.5, -2.0, 1.25)
MODELS = ("pinhole", "simple_radial", "radial", "simple_divisional")
SHAPES = ((13, 19), (67, 65), (5, 130), (7, 130), (6, 260))        # (H, W)
DELTA = math.pi / 180
Q = 4096.0                                                         # predictions are multiples of 1 / Q
K1 = {"simple_radial": (-0.12, 0.08, 0.15), "radial": (-0.12, 0.08, 0.15), "simple_divisional": (-0.15, 0.1, 0.2)}
K2 = (0.03, -0.02, 0.05)
PITCH, ROLL = (0.3, -0.4, 0.15), (0.2, -0.3, 0.1)


def case_list(shape):
    """(name, kind, up_loss, lat_loss, conf, normalize): up_loss / lat_loss None = that field absent."""
    if shape == SHAPES[0]:
        return [("l1-l1-conf", "loss", "l1", "l1", True, True), ("l2-l2-conf", "loss", "l2", "l2", True, True),
                ("dot-cauchy-conf", "loss", "dot", "cauchy", True, True), ("cauchy-huber-conf", "loss", "cauchy", "huber", True, True),
                ("huber-l1-noconf", "loss", "huber", "l1", False, True), ("up-huber-conf", "loss", "huber", None, True, True),
                ("lat-huber-noconf", "loss", None, "huber", False, True),
                ("planes-norm", "planes", "", "", False, True), ("planes-raw", "planes", "", "", False, False),
                ("planes-up", "planes", "", None, False, True), ("planes-lat", "planes", None, "", False, True)]
    return [("huber-huber-conf", "loss", "huber", "huber", True, True), ("planes-norm", "planes", "", "", False, True)]


def calibration(model, H, W, k1_zero=False):
    cams = torch.zeros(B, 8, dtype=torch.float64)
    for b in range(B):
        fx = 0.9 * max(H, W) * (1 + 0.1 * b)
        cams[b, :6] = torch.tensor([W, H, fx, fx * 1.07, W / 2 + 0.37 + 0.5 * b, H / 2 - 0.21 + 0.3 * b])
        if model in K1 and not k1_zero:
            cams[b, 6] = K1[model][b]
        if model == "radial":
            cams[b, 7] = K2[b]
    p, r = torch.tensor(PITCH, dtype=torch.float64), torch.tensor(ROLL, dtype=torch.float64)
    h = -torch.cos(p)
    gravs = torch.stack([torch.sin(r) * h, torch.cos(r) * h, torch.sin(p)], -1)
    return cams.float(), gravs.float()


def perturbed(cams, gravs, scale=0.25):
    """field_error_gate._perturbed: the calibration moved by scale x (roll 3 deg, pitch 3 deg, focal 3 %)."""
    g = gravs.double()
    pitch, roll = torch.asin(g[:, 2].clamp(-1, 1)), torch.atan2(-g[:, 0], -g[:, 1])
    pitch, roll = pitch - scale * math.radians(3), roll + scale * math.radians(3)
    h = -torch.cos(pitch)
    c = cams.clone().double()
    c[:, 2:4] *= 1 + 0.03 * scale
    return c.float(), torch.stack([torch.sin(roll) * h, torch.cos(roll) * h, torch.sin(pitch)], -1).float()


def make_inputs(model, H, W, seed, k1_zero=False):
    g = torch.Generator().manual_seed(seed)
    cams, gravs = calibration(model, H, W, k1_zero)
    f = pg.fields(model, *perturbed(cams, gravs), H, W)
    noise = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) - 0.5) * 0.04  # noqa: E731
    up = f["up"].permute(0, 3, 1, 2) + noise(B, 2, H, W)
    lat = f["lat"][:, None] + noise(B, 1, H, W)
    return {"cam": cams.numpy(), "grav": gravs.numpy(),
            "up_q": torch.round(up * Q).to(torch.int16).numpy(), "lat_q": torch.round(lat * Q).to(torch.int16).numpy(),
            "upc_k": torch.randint(1, 8, (B, H, W), generator=g).to(torch.uint8).numpy(),
            "latc_k": torch.randint(1, 8, (B, H, W), generator=g).to(torch.uint8).numpy(),
            "gup_k": torch.randint(-4, 5, (B, H, W, 2), generator=g).to(torch.int8).numpy(),
            "glat_k": torch.randint(-4, 5, (B, H, W), generator=g).to(torch.int8).numpy()}


def decode(inp, dtype=torch.float32):
    """The tensors a stored input set stands for."""
    t = lambda k, div: torch.from_numpy(inp[k].astype(np.float64) / div).to(dtype)  # noqa: E731
    return {"cam": torch.from_numpy(inp["cam"]).to(dtype), "grav": torch.from_numpy(inp["grav"]).to(dtype),
            "up": t("up_q", Q), "lat": t("lat_q", Q), "upc": t("upc_k", 8.0), "latc": t("latc_k", 8.0),
            "gup": t("gup_k", 4.0), "glat": t("glat_k", 4.0)}


def check_conditions(model, inp, k1_zero=False):
    """The conditions of the inputs (module docstring of tests/test_field_calib_grad_abi.py lists them)."""
    d = decode(inp, torch.float64)
    H, W = d["lat"].shape[-2:]
    f = pg.fields(model, d["cam"].float(), d["grav"].float(), H, W)
    cam = d["cam"]
    assert (cam[:, 2] != cam[:, 3]).all() and ((cam[:, 4:6] % 1) != 0).all()
    assert (d["grav"][:, 2] > 0).any() and (d["grav"][:, 2] < 0).any()
    res = {"up": d["up"] - f["up"].permute(0, 3, 1, 2), "lat": d["lat"] - f["lat"][:, None]}
    for name, r in res.items():
        assert (r != 0).all(), name
        a = r.abs().reshape(B, -1)
        assert ((a < DELTA).sum(1) >= 4).all() and ((a > DELTA).sum(1) >= 4).all(), (name, (a < DELTA).sum(1), (a > DELTA).sum(1))
    assert (f["sin"].abs() <= pg.LAT_HI32 - 1e-3).all()
    assert (f["qnorm"] >= 1e-3).all()
    if model == "simple_divisional":
        k1 = cam[:, 6, None, None]
        x, y = torch.arange(W, dtype=torch.float64)[None, None, :], torch.arange(H, dtype=torch.float64)[None, :, None]
        r2 = ((x - cam[:, 4, None, None]) / cam[:, 2, None, None]) ** 2 + ((y - cam[:, 5, None, None]) / cam[:, 3, None, None]) ** 2
        if k1_zero:
            assert (k1 == 0).all()
        else:
            assert (1 - 4 * k1 * r2 >= 1e-2).all() and (k1 * r2 != 0).all()


class _KeepDouble(torch.Tensor):
    """Float64 predictions through calculate_losses' `predictions.float()` (nn.HuberLoss takes one dtype only)."""

    def float(self):
        return self.as_subclass(torch.Tensor)


def reference():
    spec = importlib.util.spec_from_file_location("make_golden_field_loss", os.path.join(HERE, "make_golden_field_loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fns = mod.reference_decoders()
    return ref_import.load(), fns


def record_case(ns, fns, model, d64, case):
    """The (3, 3, 11) array of one case."""
    name, kind, up_loss, lat_loss, conf, normalize = case
    pf = ns.perspective_fields
    cam_cls = ns.camera.camera_models[model]
    gout = torch.tensor(GOUT, dtype=torch.float64)

    def wrap(cam, grav):
        c, g = cam_cls(cam.detach()), ns.gravity.Gravity(grav.detach())
        c._data, g._data = cam, grav                 # the leaves themselves: no normalisation of the gravity in between
        return c, g

    def targets(cam, grav):
        c, g = wrap(cam, grav)
        B_, (H, W) = cam.shape[0], d64["lat"].shape[-2:]
        up = pf.get_up_field(c, g, normalize=normalize).reshape(B_, H, W, 2) if up_loss is not None else None
        lat = pf.get_latitude_field(c, g).reshape(B_, H, W) if lat_loss is not None else None
        return up, lat

    def total(up_t, lat_t, d):
        dt = d["lat"].dtype
        t = 0
        if kind == "planes":
            if up_t is not None:
                t = t + (d["gup"] * up_t).sum()
            if lat_t is not None:
                t = t + (d["glat"] * lat_t).sum()
            return t
        for field, tgt, kind_, pred, cf in (("up", None if up_t is None else up_t.permute(0, 3, 1, 2), up_loss, d["up"], d["upc"]),
                                            ("latitude", None if lat_t is None else lat_t[:, None], lat_loss, d["lat"], d["latc"])):
            if tgt is None:
                continue
            self = types.SimpleNamespace(loss_type=kind_, use_uncertainty_loss=conf, loss_weight=1.0,
                                         conf=types.SimpleNamespace(loss_type=kind_))
            if dt == torch.float64:               # the reference's predictions.float() would round the float64 run: keep it double
                pred = pred.as_subclass(_KeepDouble)
            loss = fns[field](self, pred, tgt, cf if conf else None)[f"{field}-{kind_}-loss"]
            t = t + (gout.to(loss.dtype) * loss).sum()
        return t

    out = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        d = {k: v.to(dt) for k, v in d64.items()}
        cam, grav = d["cam"].clone().requires_grad_(True), d["grav"].clone().requires_grad_(True)
        t = total(*targets(cam, grav), d)
        assert t.dtype == dt, (t.dtype, dt)
        gc, gg = torch.autograd.grad(t, [cam, grav])
        out[tag] = torch.cat([gc, gg], 1).double().numpy()
    # per pixel, in float64: the cotangent of the targets times the forward-mode derivative of the fields
    d = d64
    with torch.no_grad():
        up0, lat0 = targets(d["cam"], d["grav"])
    leaves = [t.clone().requires_grad_(True) for t in (up0, lat0) if t is not None]
    it = iter(leaves)
    t = total(next(it) if up0 is not None else None, next(it) if lat0 is not None else None, d)
    cot = list(torch.autograd.grad(t, leaves))
    A = torch.zeros(B, 11, dtype=torch.float64)
    S = torch.zeros(B, 11, dtype=torch.float64)
    for j in range(11):
        tc, tg = torch.zeros_like(d["cam"]), torch.zeros_like(d["grav"])
        (tc if j < 8 else tg)[:, j if j < 8 else j - 8] = 1.0
        fn = lambda c, g: tuple(x for x in targets(c, g) if x is not None)  # noqa: E731
        _, tangents = torch.autograd.functional.jvp(fn, (d["cam"], d["grav"]), (tc, tg))
        contrib = 0
        for g_, dt_ in zip(cot, tangents):
            c_ = g_ * dt_
            contrib = contrib + (c_.sum(-1) if c_.dim() == 4 else c_)
        A[:, j], S[:, j] = contrib.abs().sum((1, 2)), contrib.sum((1, 2))
    full = out["64"]
    # (the pixels' contributions add up to the gradient; 1e-12: the k1 = 0 case, where reverse mode leaves rounding and forward mode 0)
    assert np.all(np.abs(S.numpy() - full) <= 1e-9 * A.numpy() + 1e-12), (name, np.abs(S.numpy() - full).max())
    return np.stack([out["64"], out["32"], A.numpy()], 1)


def main():
    ns, fns = reference()
    rec = {"grad_output": np.array(GOUT, np.float32)}
    sets = [(m, m, s, False) for m in MODELS for s in SHAPES] + [("simple_divisional_k0", "simple_divisional", SHAPES[0], True)]
    for i, (tag, model, (H, W), k1_zero) in enumerate(sets):
        inp = make_inputs(model, H, W, 100 + i, k1_zero)
        check_conditions(model, inp, k1_zero)
        base = f"{tag}/{H}x{W}"
        for k, v in inp.items():
            rec[f"{base}/{k}"] = v
        d64 = decode(inp, torch.float64)
        cases = case_list((H, W))
        if k1_zero:
            cases = [c for c in cases if c[0] in ("l2-l2-conf", "planes-norm", "planes-up", "planes-lat")]
        for case in cases:
            rec[f"{base}/{case[0]}"] = record_case(ns, fns, model, d64, case)
        print(base, len(cases), "cases", flush=True)
    out = os.path.join(HERE, "field_calib_grad_reference.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes,", len(rec), "arrays")


if __name__ == "__main__":
    main()
