"""The fixture and the gate of the calibration gradients (gclm_field_loss_param_grad, gclm_perspective_fields_backward),
shared by tests/test_field_calib_grad_abi.py (CPU checks, the C ABI on the GPU) and tests/test_field_calib_grad.py (autograd).

Fixture: tests/golden/field_calib_grad_reference.npz, written by tests/golden/make_golden_field_calib_grad.py from the
reference's own get_perspective_field and calculate_losses -- per case the gradients to the camera data and the gravity
vector in float64 autograd (ref64), the same in float32 (ref32), and per entry A = sum over pixels of |that pixel's
contribution| in float64.

Gate, per image and entry:   |hip - ref64| <= G max(|ref32 - ref64|, 2^-23 A),   G = 4 (the project's stage-gate figure).
The unit is the larger of the reference's own float32 error at that entry and half a float32 ulp of every pixel's
contribution: a float32 evaluation cannot be held below the second, and the first is what the reference itself delivers.
Entries the formulas never read (w, h; k2 of the one-parameter models; k1, k2 of pinhole) are 0 on both sides, exactly."""
import math
import os

import numpy as np
import torch

from conftest import GOLDEN

PATH = os.path.join(GOLDEN, "field_calib_grad_reference.npz")
G = 4.0
B = 3
MODELS = ("pinhole", "simple_radial", "radial", "simple_divisional")
SHAPES = ((13, 19), (67, 65), (5, 130), (7, 130), (6, 260))        # (H, W)
Q = 4096.0
DELTA = math.pi / 180
INPUTS = ("cam", "grav", "up_q", "lat_q", "upc_k", "latc_k", "gup_k", "glat_k")
_cache = {}


def golden():
    if "z" not in _cache:
        with np.load(PATH) as z:
            _cache["z"] = {k: z[k] for k in z.files}
    return _cache["z"]


def sets():
    """(tag, model, H, W) of every input set of the fixture."""
    out = []
    for k in golden():
        if k.endswith("/cam"):
            tag, shape = k.split("/")[:2]
            H, W = (int(v) for v in shape.split("x"))
            out.append((tag, "simple_divisional" if tag == "simple_divisional_k0" else tag, H, W))
    return out


def cases():
    """(tag, model, H, W, case name) of every recorded case."""
    z = golden()
    return [(tag, model, H, W, k.split("/")[2]) for tag, model, H, W in sets() for k in z
            if k.startswith(f"{tag}/{H}x{W}/") and k.split("/")[2] not in INPUTS]


def case_id(c):
    return f"{c[0]}-{c[2]}x{c[3]}-{c[4]}"


def parse(name):
    """(kind, up_loss, lat_loss, conf, normalize) of a case name; a loss of None = that field absent."""
    if name.startswith("planes"):
        what = name.split("-")[1]
        return "planes", None if what == "lat" else "", None if what == "up" else "", False, what != "raw"
    parts = name.split("-")
    conf = parts[-1] == "conf"
    if parts[0] == "up":
        return "loss", parts[1], None, conf, True
    if parts[0] == "lat":
        return "loss", None, parts[1], conf, True
    return "loss", parts[0], parts[1], conf, True


def inputs(tag, H, W, dtype=torch.float32, device="cpu"):
    """The tensors an input set stands for: cam (3, 8), grav (3, 3), up (3, 2, H, W), lat (3, 1, H, W), upc / latc (3, H, W),
    gup (3, H, W, 2), glat (3, H, W); all exact in float32."""
    z, base = golden(), f"{tag}/{H}x{W}/"
    t = lambda k, div: torch.from_numpy(z[base + k].astype(np.float64) / div).to(dtype).to(device)  # noqa: E731
    return {"cam": torch.from_numpy(z[base + "cam"]).to(dtype).to(device), "grav": torch.from_numpy(z[base + "grav"]).to(dtype).to(device),
            "up": t("up_q", Q), "lat": t("lat_q", Q), "upc": t("upc_k", 8.0), "latc": t("latc_k", 8.0),
            "gup": t("gup_k", 4.0), "glat": t("glat_k", 4.0)}


def grad_output(device="cpu"):
    return torch.from_numpy(golden()["grad_output"]).to(device)


def reference(c):
    """(ref64, ref32, A), each (3, 11) float64: columns 0..7 the camera data, 8..10 the gravity vector."""
    a = golden()[f"{c[0]}/{c[2]}x{c[3]}/{c[4]}"]
    return a[:, 0], a[:, 1], a[:, 2]


def unread_columns(model):
    """The columns of the camera gradient that are 0 on both sides."""
    return [0, 1] + {"pinhole": [6, 7], "radial": []}.get(model, [7])


def ratios(c, g_cam, g_grav):
    """|hip - ref64| / max(|ref32 - ref64|, 2^-23 A) per image and entry, (3, 11); 0 where both sides are 0 exactly, inf where
    the unit is 0 and the sides differ."""
    r64, r32, A = reference(c)
    hip = np.concatenate([g_cam.detach().double().cpu().numpy(), g_grav.detach().double().cpu().numpy()], 1)
    unit = np.maximum(np.abs(r32 - r64), 2.0 ** -23 * A)
    err = np.abs(hip - r64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / unit)


def report(c, r, log=None):
    line = f"{case_id(c):48s} worst {np.nanmax(r):7.3f}  median {np.median(r[r > 0]) if (r > 0).any() else 0.0:6.3f}"
    print(line)
    if log is not None:
        log.append(line)
    return line
