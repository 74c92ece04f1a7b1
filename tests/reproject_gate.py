"""Float64 yardstick and per-pixel gate of Camera.reproject_image / upright_image (gclm_reproject_image), shared by the CPU
self-check (test_reproject_abi.py) and the GPU parity test (test_reproject_image.py).  Built on tests/undistort_gate.py: its
images, cameras, float64 grid_sample, honest float32 bilinear sum and the bound L * delta + 4 ulp(A).

Yardstick: the definition of include/gclm.h (gclm_reproject_image) in float64 from the float32 cameras and rotations --
coordinates, the visible and inside_model tests -- and F.grid_sample(bilinear, zeros, align_corners=True) of the float64
source; 0 where a test fails.  Gate per pixel and channel:
    |out - ref| <= L * delta + 4 ulp(A)
L the largest difference between neighbouring source pixels (zero padding included) in the 4 x 4 window around the float64
floor, A the largest magnitude there, delta DERIVED per case from a float32 restatement of the kernel's evaluation order
against float64 (coordinate_bound).  A pixel whose float64 coordinate is more than delta outside [-1, Win] x [-1, Hin], or
that is invisible or folded, has bound 0: the output must be exactly 0.

The definition is discontinuous where q_z crosses 1e-3 and where s + 2 r2s s' crosses 0; there float32 and float64 may
legitimately decide differently, so the pixels with
    |q_z - 1e-3| < 1e-5 |q|    or    |s + 2 r2s s'| < 1e-4
are excluded from the value gate, and for the mask also the pixels whose coordinate lies within delta of the in-image
edge.  Excluded pixels are at most CAP = 2 % of any image: a condition on the cases (asserted on CPU for every case), not a
measurement."""
import math

import torch

from geocalib_amd.utils import rad2rotmat
import undistort_gate as ug

EPS = 1e-3                      # BaseCamera.eps
CAP = 0.02
B, C = 3, 3
HS, WS = 30, 44                 # nominal size of the source camera
HIN, WIN = 41, 59               # size the source image is stored at: exercises (Win - 1) / (Ws - 1)


def _t(model, k1, k2, r2):
    """Undistort scale, the forms of csrc/gclm_render.h (any dtype)."""
    if model == "pinhole":
        return torch.ones_like(r2)
    if model == "simple_radial":
        return 1 - k1 * r2
    if model == "radial":
        return 1 - k1 * r2 + (3 * k1 * k1 - k2) * (r2 * r2)
    den = 1 + k1 * r2
    return 1 / torch.where(den == 0, torch.full_like(den, 1e6), den)


def _s(model, k1, k2, r2):
    """Distort scale and ds/dr2, the non-cancelling forms of csrc/gclm_render.h in its order (any dtype)."""
    one, zero = torch.ones_like(r2), torch.zeros_like(r2)
    if model == "pinhole":
        return one, zero
    if model == "simple_radial":
        return 1 + k1 * r2, k1 + zero
    if model == "radial":
        return 1 + (k1 + k2 * r2) * r2, k1 + 2 * k2 * r2
    kr = k1 * r2
    tau = 1 - 4 * kr
    rt = torch.sqrt(tau.clamp(min=0))
    d = 1 + rt
    s = torch.where(tau > 0, 2 / d, 1 / torch.where(kr == 0, one, 2 * kr))
    tt = torch.sqrt(torch.tensor(1e-6, dtype=r2.dtype, device=r2.device))
    den = 2 * k1 * (r2 * r2) * tt
    hi = tau >= 1e-6
    sp = torch.where(hi, 4 * k1 / torch.where(hi, rt * d * d, one), (2 * k1 * r2 - (1 - tt) * tt) / torch.where(den == 0, 1e6 * one, den))
    return torch.where(kr == 0, one, s), torch.where(kr == 0, zero, sp)


def coordinates(src_model, src_cams, tgt_model, tgt_cams, rot, H, W, Hs, Ws, Hin, Win, dtype=torch.float64, device="cpu"):
    """The definition for every output pixel, in `dtype`: float64 is the yardstick; float32 restates the kernel's evaluation
    order (1 / f and 1 / q_z once, then products; the scale (Win - 1) / (Ws - 1) correctly rounded).  Cameras (n, 8), `rot`
    (nr, 3, 3) or None.  Returns a dict of (max(n, nr), H, W) tensors: ix, iy (as computed, possibly non-finite where not ok),
    ok = visible & inside_model, visible, r2s, and the two quantities the discontinuities hang on: zgap = |q_z - eps| / |q|,
    mono = s + 2 r2s s'."""
    cs, ct = src_cams.to(device=device, dtype=dtype), tgt_cams.to(device=device, dtype=dtype)
    fxs, fys, cxs, cys, k1s, k2s = (cs[:, i, None, None] for i in range(2, 8))
    fxt, fyt, cxt, cyt, k1t, k2t = (ct[:, i, None, None] for i in range(2, 8))
    x = torch.arange(W, device=device, dtype=dtype)[None, None, :]
    y = torch.arange(H, device=device, dtype=dtype)[None, :, None]
    if dtype == torch.float64:
        u, v = (x - cxt) / fxt, (y - cyt) / fyt
        sx, sy = (Win - 1) / (Ws - 1), (Hin - 1) / (Hs - 1)
    else:
        u, v = (x - cxt) * (1 / fxt), (y - cyt) * (1 / fyt)
        sx = torch.tensor((Win - 1) / (Ws - 1), dtype=dtype, device=device)
        sy = torch.tensor((Hin - 1) / (Hs - 1), dtype=dtype, device=device)
    t = _t(tgt_model, k1t, k2t, u * u + v * v)
    bu, bv = u * t, v * t
    if rot is None:
        qx, qy, qz = bu, bv, torch.ones_like(bu)
    else:
        M = rot.to(device=device, dtype=dtype)[:, :, :, None, None]
        qx, qy, qz = (bu * M[:, 0, j] + bv * M[:, 1, j] + M[:, 2, j] for j in range(3))
    visible = (qz > EPS) & torch.isfinite(qz)
    iz = 1 / qz
    px, py = qx * iz, qy * iz
    r2s = px * px + py * py
    s, sp = _s(src_model, k1s, k2s, r2s)
    mono = s + 2 * r2s * sp
    inside = mono > 0 if src_model != "pinhole" else torch.ones_like(visible)
    ix, iy = (px * s * fxs + cxs) * sx, (py * s * fys + cys) * sy
    zgap = (qz - EPS).abs() / torch.sqrt(qx * qx + qy * qy + qz * qz)
    n = max(ix.shape[0], qz.shape[0])
    e = lambda a: a.expand(n, H, W)  # noqa: E731
    return {"ix": e(ix), "iy": e(iy), "ok": e(visible & inside), "zgap": e(zgap), "mono": e(mono), "visible": e(visible),
            "r2s": e(r2s)}


def excluded(c64, src_model):
    """Pixels at a discontinuity of the definition (module docstring), from the float64 yardstick."""
    ex = c64["zgap"] < 1e-5
    if src_model != "pinhole":
        ex = ex | (c64["visible"] & (c64["mono"].abs() < 1e-4))
    return ex


def in_image(c, Hin, Win):
    return c["ok"] & (c["ix"] >= 0) & (c["ix"] <= Win - 1) & (c["iy"] >= 0) & (c["iy"] <= Hin - 1)


def edge_band(c64, Hin, Win, delta):
    """Pixels whose float64 coordinate lies within delta of the in-image edge: the mask may go either way."""
    ix, iy = c64["ix"], c64["iy"]
    return (ix.abs() < delta) | ((ix - (Win - 1)).abs() < delta) | (iy.abs() < delta) | ((iy - (Hin - 1)).abs() < delta)


def sample_at(c):
    """(ix, iy) with the pixels that are not ok, or not finite, moved to where no tap lies inside the source."""
    seen = c["ok"] & torch.isfinite(c["ix"]) & torch.isfinite(c["iy"])
    out = torch.full_like(c["ix"], -2.0)
    return torch.where(seen, c["ix"], out), torch.where(seen, c["iy"], out)


def coordinate_bound(c64, c32, ex, Hin, Win):
    """delta: 4 x the largest |dix| + |diy| of the float32 restatement against float64 over the pixels that both decide ok,
    that are not excluded and whose float64 coordinate lies within a pixel of the source, plus 2 ulp of the largest such
    coordinate (what the kernel's contracted multiply-adds may differ from the restatement by)."""
    ix, iy = c64["ix"], c64["iy"]
    near = c64["ok"] & c32["ok"] & ~ex & (ix >= -1) & (ix <= Win) & (iy >= -1) & (iy <= Hin)
    err = ((c32["ix"].double() - ix).abs() + (c32["iy"].double() - iy).abs())[near]
    worst = err.max().item() if err.numel() else 0.0
    return 4 * worst + 2 * max(Win, Hin) * 2.0 ** -23


def reference(src64, c64, ex, delta):
    """(ref, bound), (B, C, H, W) float64: the yardstick image and its per-pixel gate, inf on the excluded pixels."""
    gx, gy = sample_at(c64)
    ref = ug.grid_sample64(src64, gx, gy)
    bound = ug.gate(src64, gx, gy, delta)
    ex = ex.expand(src64.shape[0], -1, -1)[:, None].expand_as(bound)
    return ref, torch.where(ex, torch.full_like(bound, math.inf), bound)


def worst_ratio(out, ref, bound):
    """ug.worst_ratio over the pixels whose bound is finite (the others are excluded)."""
    keep = torch.isfinite(bound)
    return ug.worst_ratio(out[keep], ref[keep], bound[keep]) if keep.any() else 0.0


# ------------------------------------------------------------------ rotations
def upright_rotation(roll_deg, pitch_deg, level_pitch):
    """M = R_t @ R_s^T of upright_image for a camera rolled and pitched by the given degrees (float64)."""
    r, p = (torch.tensor(math.radians(a), dtype=torch.float64) for a in (roll_deg, pitch_deg))
    zero = torch.zeros_like(r)
    return rad2rotmat(zero, zero if level_pitch else p) @ rad2rotmat(r, p).transpose(-1, -2)


def make_rotations(kind, nr):
    """(nr, 3, 3) float32, or None: "none", "eye", "roll25" (a 25 deg roll removed), "level" ((-40, 30) deg levelled) and
    "yaw100" (a 100 deg yaw: nearly every pixel looks away from the source).  Image i of a batch differs by i degrees."""
    if kind == "none":
        return None
    mats = []
    for i in range(nr):
        if kind == "eye":
            mats.append(torch.eye(3, dtype=torch.float64))
        elif kind == "roll25":
            mats.append(upright_rotation(25.0 + i, 0.0, False))
        elif kind == "level":
            mats.append(upright_rotation(-40.0 + i, 30.0 - i, True))
        else:
            z = torch.zeros((), dtype=torch.float64)
            mats.append(rad2rotmat(z, z, z + math.radians(100.0 + i)))
    return torch.stack(mats).to(torch.float32)


# Cases: (source model, k1, k2, f / W or None, target model, k1, k2, rotation, camera batch, rotation batch, H, W, images).
# k None: drawn across the model's dist_range per camera; f None: drawn in 0.5 .. 1.2 W.  B = 3, C = 3, the source stored
# at 41 x 59 for a nominal 30 x 44 camera.  Outputs 30 x 44, 37 x 53 and 9 x 130 (two tiles per row, a ragged tail).
# simple_radial k1 = -0.3 and simple_divisional k1 = +-2 at f = 0.5 W put the fold radius / the tau = 0 clamp inside the image.
CASES = [
    ("pinhole", None, None, None, "pinhole", None, None, "none", 1, 1, 30, 44, "noise"),
    ("pinhole", None, None, None, "simple_radial", 0.2, None, "roll25", 3, 3, 37, 53, "smooth"),
    ("simple_radial", None, None, None, "pinhole", None, None, "eye", 3, 1, 9, 130, "noise"),
    ("simple_radial", None, None, None, "radial", -0.1, 0.05, "level", 1, 3, 30, 44, "noise"),
    ("simple_radial", -0.3, None, 0.5, "pinhole", None, None, "none", 1, 1, 37, 53, "noise"),
    ("simple_radial", -0.3, None, 0.5, "simple_divisional", -0.3, None, "roll25", 3, 1, 30, 44, "smooth"),
    ("simple_radial", 0.7, None, None, "pinhole", None, None, "roll25", 1, 1, 9, 130, "smooth"),
    ("radial", None, None, None, "pinhole", None, None, "roll25", 3, 3, 30, 44, "noise"),
    ("radial", None, None, None, "simple_radial", 0.2, None, "none", 3, 1, 37, 53, "noise"),
    ("radial", -0.7, 0.3, None, "pinhole", None, None, "level", 1, 1, 37, 53, "smooth"),
    ("radial", 0.7, 0.7, None, "radial", -0.1, 0.05, "eye", 1, 3, 9, 130, "noise"),
    ("simple_divisional", None, None, None, "pinhole", None, None, "none", 3, 1, 30, 44, "noise"),
    ("simple_divisional", None, None, None, "simple_divisional", -0.3, None, "level", 3, 3, 37, 53, "smooth"),
    ("simple_divisional", 2.0, None, 0.5, "pinhole", None, None, "level", 1, 1, 30, 44, "noise"),
    ("simple_divisional", 2.0, None, 0.5, "simple_radial", 0.2, None, "none", 1, 1, 37, 53, "noise"),
    ("simple_divisional", -2.0, None, 0.5, "pinhole", None, None, "level", 1, 3, 9, 130, "noise"),
    ("simple_divisional", -2.0, None, 0.5, "radial", -0.1, 0.05, "eye", 3, 1, 30, 44, "smooth"),
    ("pinhole", None, None, None, "pinhole", None, None, "yaw100", 1, 1, 30, 44, "noise"),
    ("radial", None, None, None, "simple_divisional", -0.3, None, "yaw100", 3, 3, 37, 53, "noise"),
]


def case_id(case):
    sm, k1, k2, f, tm, tk1, tk2, rot, nb, nr, H, W, kind = case
    return f"{sm}[{k1},{k2},{f}]-to-{tm}-{rot}-nb{nb}-nr{nr}-{H}x{W}-{kind}"


def case_inputs(case, seed=0):
    """(source cameras (nb, 8), target cameras (nb, 8), rotations (nr, 3, 3) or None, image (B, C, HIN, WIN)), float32."""
    sm, k1, k2, f, tm, tk1, tk2, rot, nb, nr, H, W, kind = case
    src = ug.make_cameras(sm, nb, HS, WS, k1, k2, seed)
    if f is not None:
        src[:, 2] = src[:, 3] = f * WS
    tgt = ug.make_cameras(tm, nb, H, W, tk1, tk2, seed + 1)
    return src, tgt, make_rotations(rot, nr), ug.make_images(kind, B, C, HIN, WIN, seed)


def case_parts(case, device="cpu"):
    """Everything the gate of one case needs, on `device`: the inputs, the float64 yardstick and its float32 restatement
    (always derived on the CPU: delta must not depend on the device under test), delta, ref, bound and the mask parts."""
    sm, tm, H, W = case[0], case[4], case[10], case[11]
    src, tgt, rot, img = case_inputs(case)
    geo = (sm, src, tm, tgt, rot, H, W, HS, WS, HIN, WIN)
    c64, c32 = coordinates(*geo), coordinates(*geo, dtype=torch.float32)
    ex = excluded(c64, sm)
    delta = coordinate_bound(c64, c32, ex, HIN, WIN)
    if torch.device(device).type != "cpu":
        c64 = coordinates(*geo, device=device)
        ex = excluded(c64, sm)
    src64 = img.to(device=device, dtype=torch.float64)
    ref, bound = reference(src64, c64, ex, delta)
    return {"src": src, "tgt": tgt, "rot": rot, "img": img, "c64": c64, "c32": c32, "ex": ex, "delta": delta, "ref": ref,
            "bound": bound, "valid": in_image(c64, HIN, WIN).expand(B, -1, -1),
            "mask_free": (ex | edge_band(c64, HIN, WIN, delta)).expand(B, -1, -1)}
