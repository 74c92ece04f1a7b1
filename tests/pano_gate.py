"""Float64 yardstick and per-pixel gate of Camera.get_img_from_pano (gclm_render_from_pano), shared by the CPU self-check
(test_pano_abi.py) and the GPU parity test (test_pano_image.py).

Reference: F.grid_sample(bilinear, zeros, align_corners=True) of the float64 panorama at float64 coordinates (ix, iy)
computed from the float32 camera and the float32 rotation R_i.  The kernel's float32 result differs from it in two ways:
  - its coordinate carries float32 rounding.  That rounding is conditioned by atan2: a relative error u = 2^-24 of the
    rotated bearing b' moves lon by about u / rho and lat by about u, rho = hypot(b'x, b'z), so per pixel
        delta_p = kappa u ((Ws - 1) / (2 pi rho_p) + (Hs - 1) / pi) + 4 ulp(max(Ws, Hs)),
    with kappa DERIVED per case: twice the worst ratio of a float32 restatement of the kernel's formula against float64
    (coordinate_kappa).  delta_p grows towards the poles (rho -> 0);
  - its bilinear sum carries float32 rounding of the weights, products and sums.
A coordinate error moves the interpolant by at most L delta_p, L the largest difference between neighbouring panorama
pixels (zero padding included) in a window of radius ceil(delta_p) + 2 around the float64 point (rounded up to a power of
two, capped at the panorama width); the sum's rounding is a few ulp of the largest |value| A in that window.  Gate:
    |out - ref| <= L delta_p + 4 ulp(A).
At the seam (b'z < 0, lon within delta_p of +-pi) float32 may take the other branch of atan2: the pixel passes if it meets
the gate at either branch's coordinate."""
import math

import torch
from torch.nn import functional as F

from geocalib_amd.gravity import Gravity
from geocalib_amd.utils import rad2rotmat
import undistort_gate as ug

MODELS = ug.MODELS
U = 2.0 ** -24


def rotations(roll, pitch, yaws):
    """(n, 3, 3) float32 R_i = Gravity.from_rp(roll, pitch).R @ rad2rotmat(0, 0, yaw), the public method's own ops."""
    g = Gravity.from_rp(torch.as_tensor(roll, dtype=torch.float32), torch.as_tensor(pitch, dtype=torch.float32))
    y = torch.as_tensor(yaws, dtype=torch.float32).reshape(-1)
    return g.R.reshape(-1, 3, 3) @ rad2rotmat(y.new_zeros(y.shape), y.new_zeros(y.shape), y)


def _undistort_scale(model, k1, k2, r2, distort=False):
    if model == "pinhole":
        return torch.ones_like(r2)
    if distort:                                       # a mutant: the distort form where the undistort form belongs
        return 1 + k1 * r2 + (k2 * r2 * r2 if model == "radial" else 0)
    if model == "simple_radial":
        return 1 - k1 * r2
    if model == "radial":
        return 1 - k1 * r2 + (3 * k1 * k1 - k2) * (r2 * r2)
    den = 1 + k1 * r2
    return 1 / torch.where(den == 0, torch.full_like(den, 1e6), den)


def bearings(model, cams, rot, H, W, dtype=torch.float64, device="cpu", half_pixel=False, distort=False):
    """Rotated bearings b' = normalize((p, 1)) @ R_i, (n, H, W, 3) in `dtype` (float32: the kernel's order, unnormalised)."""
    c = cams.to(device=device, dtype=dtype)
    c = c.expand(rot.shape[0], -1) if c.shape[0] == 1 else c
    fx, fy, cx, cy, k1, k2 = (c[:, i, None, None] for i in range(2, 8))
    x = torch.arange(W, device=device, dtype=dtype)[None, None, :] + (0.5 if half_pixel else 0.0)
    y = torch.arange(H, device=device, dtype=dtype)[None, :, None] + (0.5 if half_pixel else 0.0)
    u, v = (x - cx) / fx, (y - cy) / fy
    s = _undistort_scale(model, k1, k2, u * u + v * v, distort)
    p = torch.stack(torch.broadcast_tensors(u * s, v * s, torch.ones_like(u * s)), -1)
    if dtype == torch.float64:
        p = F.normalize(p, dim=-1)
    R = rot.to(device=device, dtype=dtype)
    return torch.einsum("nhwi,nij->nhwj", p, R.expand(p.shape[0], 3, 3))


def coordinates(model, cams, rot, H, W, Hs, Ws, dtype=torch.float64, device="cpu", mutant=None):
    """Panorama coordinates (ix, iy, rho, b'z), each (n, H, W).  float64 is the yardstick; float32 restates the kernel."""
    b = bearings(model, cams, rot, H, W, dtype, device, half_pixel=mutant == "half_pixel", distort=mutant == "distort")
    bx, by, bz = b.unbind(-1)
    rho = torch.hypot(bx, bz)
    lon = torch.atan2(bz, bx) if mutant == "atan2_swap" else torch.atan2(bx, bz)
    lat = torch.atan2(by, rho)
    Ws_, Hs_ = torch.as_tensor(Ws, dtype=dtype, device=device), torch.as_tensor(Hs, dtype=dtype, device=device)
    if Ws_.dim():
        Ws_, Hs_ = Ws_[:, None, None], Hs_[:, None, None]
    wx = Ws_ if mutant in ("Ws", "wrap") else Ws_ - 1
    ix = (lon * (1 / math.pi) + 1) * 0.5 * wx
    iy = (2 * lat * (1 / math.pi) + 1) * 0.5 * (Hs_ - 1)
    return ix, iy, rho, bz


def coordinate_kappa(model, cams, rot, H, W, Hs, Ws):
    """kappa: twice the worst (|dix| + |diy|) / (u ((Ws - 1) / (2 pi rho) + (Hs - 1) / pi)) of the float32 restatement
    against float64 (a seam pixel counts with the nearer branch)."""
    ix, iy, rho, _ = coordinates(model, cams, rot, H, W, Hs, Ws)
    jx, jy, _, _ = coordinates(model, cams, rot, H, W, Hs, Ws, torch.float32)
    dx = (jx.double() - ix).abs()
    dx = torch.minimum(dx, (dx - (Ws - 1)).abs())
    err = dx + (jy.double() - iy).abs()
    scale = U * ((Ws - 1) / (2 * math.pi * rho) + (Hs - 1) / math.pi)
    ok = torch.isfinite(err) & (scale > 0)
    return 2 * (err[ok] / scale[ok]).max().item() if ok.any() else 0.0


def delta_map(kappa, rho, Hs, Ws):
    return kappa * U * ((Ws - 1) / (2 * math.pi * rho) + (Hs - 1) / math.pi) + 4 * max(Ws, Hs) * 2.0 ** -24


def grid_sample64(src64, ix, iy, padding_mode="zeros"):
    """F.grid_sample of (1 or n, C, Hs, Ws) at pixel coordinates (n, H, W), align_corners=True."""
    Hs, Ws = src64.shape[-2:]
    g = torch.stack([2 * ix / (Ws - 1) - 1, 2 * iy / (Hs - 1) - 1], -1)
    src = src64.expand(ix.shape[0], -1, -1, -1)
    return F.grid_sample(src, g.to(src64.dtype), mode="bilinear", padding_mode=padding_mode, align_corners=True)


def wrap_sample(src, ix, iy):
    """A mutant sampler: bilinear with the columns periodic (column Ws is column 0), rows zero-padded."""
    Ws = src.shape[-1]
    ext = torch.cat([src, src[..., :1]], -1)
    g = torch.stack([2 * torch.remainder(ix, Ws) / Ws - 1, 2 * iy / (src.shape[-2] - 1) - 1], -1)
    return F.grid_sample(ext.expand(ix.shape[0], -1, -1, -1), g.to(src.dtype), align_corners=True)


def bilinear32(src32, ix, iy):
    """An honest float32 evaluation of the zero-padded bilinear sum at float32 coordinates (the kernel's order)."""
    return ug.bilinear32(src32.expand(ix.shape[0], -1, -1, -1).contiguous(), ix, iy)


def _window_maps(src64, r):
    """Per panorama pixel: the largest neighbour difference L and the largest |value| A within radius r, zero padding
    included (index (y + 1, x + 1) is panorama pixel (y, x))."""
    P = F.pad(src64, (1, 1, 1, 1))
    dh = F.pad((P[..., :, 1:] - P[..., :, :-1]).abs(), (0, 1))
    dv = F.pad((P[..., 1:, :] - P[..., :-1, :]).abs(), (0, 0, 0, 1))
    base = torch.maximum(dh, dv)
    k = 2 * r + 1
    if r >= P.shape[-1] or r >= P.shape[-2]:
        L = base.amax((-2, -1), keepdim=True).expand_as(base)
        A = P.abs().amax((-2, -1), keepdim=True).expand_as(P)
    else:
        L = F.max_pool2d(base, k, stride=1, padding=r)
        A = F.max_pool2d(P.abs(), k, stride=1, padding=r)
    return L, A


def gate(src64, ix, iy, delta):
    """Per-pixel bound L delta + 4 ulp(A) (module docstring) at the float64 coordinates (n, H, W); src64 (1 or n, C, Hs, Ws)."""
    n = ix.shape[0]
    C, Hs, Ws = src64.shape[-3:]
    src = src64.expand(n, -1, -1, -1)
    radius = torch.ceil(delta.clamp(max=2.0 * Ws)) + 2
    radius = torch.where(torch.isfinite(radius), radius, torch.full_like(radius, 2.0 * Ws))
    cls = torch.ceil(torch.log2(radius)).clamp(min=1)
    out = torch.zeros(n, C, *ix.shape[1:], dtype=torch.float64, device=ix.device)
    xs = (torch.floor(ix.nan_to_num(-1.0)).clamp(-1, Ws) + 1).long()
    ys = (torch.floor(iy.nan_to_num(-1.0)).clamp(-1, Hs) + 1).long()
    for c in torch.unique(cls).tolist():
        r = min(int(2 ** c), Ws)
        L, A = _window_maps(src, r)
        idx = (ys * L.shape[-1] + xs).reshape(n, 1, -1).expand(-1, C, -1)
        Lp = torch.gather(L.reshape(n, C, -1), 2, idx).reshape(out.shape)
        Ap = torch.gather(A.reshape(n, C, -1), 2, idx).reshape(out.shape)
        _, e = torch.frexp(Ap)
        ulp = torch.where(Ap > 0, torch.ldexp(torch.ones_like(Ap), (e - 24).to(Ap.dtype)), torch.zeros_like(Ap))
        out = torch.where((cls == c)[:, None], Lp * delta[:, None] + 4 * ulp, out)
    return out


class Yardstick:
    """Everything the gate needs for one case: float64 reference(s) and bounds, both seam branches."""

    def __init__(self, model, cams, rot, H, W, src64):
        Hs, Ws = src64.shape[-2:]
        self.kappa = coordinate_kappa(model, cams.cpu(), rot.cpu(), H, W, Hs, Ws)
        dev = src64.device
        ix, iy, rho, bz = coordinates(model, cams, rot, H, W, Hs, Ws, device=dev)
        self.ix, self.iy = ix, iy
        self.delta = delta_map(self.kappa, rho, Hs, Ws)
        self.ref = grid_sample64(src64, ix, iy)
        self.bound = gate(src64, ix, iy, self.delta)
        # the other branch of atan2 at the seam: lon -/+ 2 pi
        seam = (bz < 0) & (torch.minimum(ix, (Ws - 1) - ix) <= self.delta)
        self.seam = seam
        if seam.any():
            jx = torch.where(ix > (Ws - 1) / 2, ix - (Ws - 1), ix + (Ws - 1))
            self.ref_alt = grid_sample64(src64, jx, iy)
            self.bound_alt = gate(src64, jx, iy, self.delta)
        else:
            self.ref_alt = None

    def ratio_map(self, out):
        r = _ratio(out, self.ref, self.bound)
        if self.ref_alt is not None:
            alt = _ratio(out, self.ref_alt, self.bound_alt)
            r = torch.where(self.seam[:, None], torch.minimum(r, alt), r)
        return r

    def worst_ratio(self, out):
        return self.ratio_map(out).max().item()


def _ratio(out, ref, bound):
    d = (out.to(ref.device, torch.float64) - ref).abs()
    return torch.where(bound > 0, d / torch.where(bound > 0, bound, torch.ones_like(bound)),
                       torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, math.inf)))


def make_pano(kind, C, Hs, Ws, seed=0, n=1):
    """float32 panoramas (n, C, Hs, Ws): "noise" or "smooth" (undistort_gate's images)."""
    return ug.make_images(kind, n, C, Hs, Ws, seed)


# Cases of the GPU parity test: (model, k1 or None, n, cam_batch, C, H, W, Hs, Ws, kind, roll, pitch, yaw or None).
# yaw None: n yaws spread over [-pi, pi).  Strong distortion, yaw = pi (the seam in view), pitch near +-pi/2 (a pole in
# view), C = 1 / 3 / 4, odd output sizes, camera batch 1 and n, n up to 64.
CASES = [
    ("pinhole", None, 8, 8, 3, 48, 64, 256, 512, "noise", 0.1, 0.2, None),
    ("simple_radial", None, 8, 8, 3, 47, 65, 256, 512, "noise", -0.2, 0.1, None),
    ("radial", None, 8, 1, 4, 48, 64, 256, 512, "smooth", 0.05, -0.3, None),
    ("simple_divisional", None, 8, 8, 1, 48, 64, 256, 512, "noise", 0.0, 0.0, None),
    ("simple_radial", 0.7, 4, 1, 3, 61, 83, 300, 600, "noise", 0.0, 0.0, math.pi),
    ("radial", -0.7, 4, 4, 3, 61, 83, 300, 600, "noise", 0.3, 0.05, math.pi),
    ("simple_divisional", 3.0, 4, 1, 4, 61, 83, 300, 600, "smooth", 0.0, 0.0, math.pi),
    ("pinhole", None, 4, 4, 1, 60, 80, 256, 512, "noise", 0.2, 1.5, 0.3),
    ("simple_radial", None, 4, 4, 3, 60, 80, 256, 512, "noise", -0.1, -1.5, -0.7),
    ("simple_divisional", -3.0, 4, 1, 3, 60, 80, 256, 512, "noise", 0.0, 1.55, 2.0),
    ("radial", None, 64, 64, 3, 33, 45, 128, 256, "noise", 0.1, 0.4, None),
    ("simple_divisional", None, 64, 1, 1, 33, 45, 128, 256, "smooth", -0.3, -0.2, None),
]


def case_inputs(case, seed=0):
    """(cams (cam_batch, 8) float32, rot (n, 3, 3) float32, pano (1, C, Hs, Ws) float32, yaws, rolls, pitches (n,)) of one
    case."""
    model, k1, n, nb, C, H, W, Hs, Ws, kind, roll, pitch, yaw = case
    cams = ug.make_cameras(model, nb, H, W, k1, None, seed)
    yaws = torch.linspace(-math.pi, math.pi, n + 1)[:n] + 0.1 if yaw is None else torch.full((n,), yaw)
    g = torch.Generator().manual_seed(seed + 1)
    rolls = roll + 0.05 * torch.randn(n, generator=g)
    pitches = (pitch + 0.05 * torch.randn(n, generator=g)).clamp(-1.565, 1.565)
    return cams, rotations(rolls, pitches, yaws), make_pano(kind, C, Hs, Ws, seed), yaws, rolls, pitches
