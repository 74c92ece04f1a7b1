"""Float64 yardstick and per-pixel gate of Camera.undistort_image (gclm_undistort_image), shared by the CPU self-check
(test_undistort_abi.py) and the GPU parity test (test_undistort_image.py).

Reference: F.grid_sample(bilinear, zeros, align_corners=True) of the float64 source at float64 coordinates computed from the
float32 camera.  The kernel's float32 result differs from it in two ways:
  - its coordinate (ix, iy) carries float32 rounding: |dix| + |diy| <= delta, where delta is DERIVED per case from a float32
    restatement of the kernel's formula against float64 at that case's shapes and cameras (coordinate_bound);
  - its bilinear sum carries float32 rounding of the weights, products and sums.
A coordinate error moves the interpolant by at most L * (|dix| + |diy|), L the largest difference between neighbouring
source pixels (zero padding included) in the 4 x 4 window around the float64 floor, which holds every tap either
evaluation can touch; the sum's rounding is a few ulp of the largest |value| A in that window.  Gate per pixel:
    |out - ref| <= L * delta + 4 ulp(A).
A pixel whose float64 coordinate is more than delta outside [-1, Win] x [-1, Hin] has no tap in the source for either
evaluation: its gate is 0 and the output must be exactly 0."""
import math

import torch
from torch.nn import functional as F

MODELS = ("pinhole", "simple_radial", "radial", "simple_divisional")
DIST_RANGE = {"pinhole": (0.0, 0.0), "simple_radial": (-0.7, 0.7), "radial": (-0.7, 0.7), "simple_divisional": (-3.0, 3.0)}
PAD = 3


def make_cameras(model, n, H, W, k1=None, k2=None, seed=0):
    """(n, 8) float32 cameras of size (W, H): focal 0.5 .. 1.2 W, principal point off the centre by up to 5 % (not exactly
    representable), k1 / k2 as given (scalars or lists) or drawn across the model's dist_range."""
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64)  # noqa: E731
    f = u(0.5, 1.2) * W
    cx, cy = W / 2 + u(-0.05, 0.05) * W, H / 2 + u(-0.05, 0.05) * H
    lo, hi = DIST_RANGE[model]
    k1 = u(lo, hi) if k1 is None else torch.as_tensor(k1, dtype=torch.float64).expand(n)
    k2 = (u(lo, hi) if model == "radial" else torch.zeros(n, dtype=torch.float64)) if k2 is None else \
        torch.as_tensor(k2, dtype=torch.float64).expand(n)
    if model == "pinhole":
        k1, k2 = k1 * 0, k2 * 0
    if model != "radial":
        k2 = k2 * 0
    wh = torch.tensor([W, H], dtype=torch.float64).expand(n, 2)
    return torch.cat([wh, torch.stack([f, f * u(0.95, 1.05), cx, cy, k1, k2], -1)], -1).to(torch.float32)


def make_images(kind, B, C, H, W, seed=0):
    """float32 test images: "noise" (uniform, every neighbour differs) or "smooth" (a few low-frequency waves)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "noise":
        return torch.rand(B, C, H, W, generator=g)
    y = torch.linspace(0, 1, H, dtype=torch.float64)[:, None]
    x = torch.linspace(0, 1, W, dtype=torch.float64)[None, :]
    ph = torch.rand(B, C, 3, generator=g, dtype=torch.float64) * 6.28
    out = sum(torch.sin(6.28 * (j + 1) * (x * (j % 2 + 1) + y) + ph[..., j, None, None]) for j in range(3)) / 3
    return out.to(torch.float32)


def _scale64(model, k1, k2, r2, cancelling=False):
    if model == "pinhole":
        return torch.ones_like(r2)
    if model == "simple_radial":
        return 1 + k1 * r2
    if model == "radial":
        return 1 + k1 * r2 + k2 * r2 ** 2
    kr = k1 * r2
    if cancelling:       # the reference's form: (1 - sqrt(max(0, 1 - 4 k r2))) / (2 k r2)
        num = 1 - torch.sqrt((1 - 4 * kr).clamp(min=0))
        return torch.where(kr == 0, torch.ones_like(r2), num / torch.where(kr == 0, torch.ones_like(kr), 2 * kr))
    t = 1 - 4 * kr
    s = torch.where(t > 0, 2 / (1 + torch.sqrt(t.clamp(min=0))), 1 / torch.where(kr == 0, torch.ones_like(kr), 2 * kr))
    return torch.where(kr == 0, torch.ones_like(r2), s)


def coordinates(model, cams, H, W, Hin, Win, dtype=torch.float64, cancelling=False, device="cpu"):
    """Source coordinates (n, H, W) of every output pixel, in `dtype`: float64 is the yardstick; float32 restates the
    kernel's evaluation order (1/f once, then products; (x - c) s + c; times (Win - 1) / (W - 1))."""
    c = cams.to(device=device, dtype=dtype)
    fx, fy, cx, cy, k1, k2 = (c[:, i, None, None] for i in range(2, 8))
    x = torch.arange(W, device=device, dtype=dtype)[None, None, :]
    y = torch.arange(H, device=device, dtype=dtype)[None, :, None]
    dx, dy = x - cx, y - cy
    if dtype == torch.float64:
        u, v = dx / fx, dy / fy
        sx, sy = (Win - 1) / (W - 1), (Hin - 1) / (H - 1)
    else:
        u, v = dx * (1 / fx), dy * (1 / fy)
        sx = torch.tensor((Win - 1) / (W - 1), dtype=dtype, device=device)   # correctly rounded, as the kernel's division
        sy = torch.tensor((Hin - 1) / (H - 1), dtype=dtype, device=device)
    s = _scale64(model, k1, k2, u * u + v * v, cancelling)
    return (dx * s + cx) * sx, (dy * s + cy) * sy


def coordinate_bound(model, cams, H, W, Hin, Win):
    """delta: 4 x the largest |dix| + |diy| of the float32 restatement against float64 over the pixels whose float64
    coordinate lies within a pixel of the source, plus 2 ulp of the largest such coordinate (what the kernel's contracted
    multiply-adds may differ from the restatement by where the restatement happens to round exactly)."""
    ix, iy = coordinates(model, cams, H, W, Hin, Win)
    jx, jy = coordinates(model, cams, H, W, Hin, Win, torch.float32)
    near = (ix >= -1) & (ix <= Win) & (iy >= -1) & (iy <= Hin)
    err = ((jx.double() - ix).abs() + (jy.double() - iy).abs())[near]
    worst = err.max().item() if err.numel() else 0.0
    return 4 * worst + 2 * max(Win, Hin) * 2.0 ** -23


def grid_sample64(src64, ix, iy, align_corners=True, padding_mode="zeros"):
    """The yardstick: F.grid_sample on float64 at pixel coordinates (ix, iy) of shape (B or 1, H, W)."""
    Hin, Win = src64.shape[-2:]
    g = torch.stack([2 * ix / (Win - 1) - 1, 2 * iy / (Hin - 1) - 1], -1).expand(src64.shape[0], -1, -1, -1)
    return F.grid_sample(src64, g, mode="bilinear", padding_mode=padding_mode, align_corners=align_corners)


def bilinear32(src32, ix, iy):
    """An honest float32 evaluation of the zero-padded bilinear sum at float32 coordinates (the kernel's order)."""
    B, C, Hin, Win = src32.shape
    ix, iy = ix.expand(B, -1, -1), iy.expand(B, -1, -1)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    ax, ay = ix - x0, iy - y0
    bx, by = 1 - ax, 1 - ay
    out = torch.zeros(B, C, *ix.shape[1:], dtype=torch.float32, device=src32.device)
    flat = src32.reshape(B, C, -1)
    for dyy, dxx, w in ((0, 0, bx * by), (0, 1, ax * by), (1, 0, bx * ay), (1, 1, ax * ay)):
        xi, yi = x0.long() + dxx, y0.long() + dyy
        m = (xi >= 0) & (xi < Win) & (yi >= 0) & (yi < Hin)
        idx = (yi.clamp(0, Hin - 1) * Win + xi.clamp(0, Win - 1)).reshape(B, 1, -1).expand(-1, C, -1)
        v = torch.gather(flat, 2, idx).reshape(out.shape) * m[:, None]
        out = out + v * w[:, None]
    return out


def gate(src64, ix, iy, delta):
    """Per-pixel bound L * delta + 4 ulp(A) (module docstring) for the float64 coordinates (ix, iy), (B or 1, H, W)."""
    B, C, Hin, Win = src64.shape
    P = F.pad(src64, (PAD, PAD, PAD, PAD))
    dh = F.pad((P[..., :, 1:] - P[..., :, :-1]).abs(), (0, 1))
    dv = F.pad((P[..., 1:, :] - P[..., :-1, :]).abs(), (0, 0, 0, 1))
    Lmap = F.max_pool2d(torch.maximum(dh, dv), 4, stride=1)
    Amap = F.max_pool2d(P.abs(), 4, stride=1)
    ix, iy = ix.expand(B, -1, -1), iy.expand(B, -1, -1)
    inside = (ix >= -1 - delta) & (ix <= Win + delta) & (iy >= -1 - delta) & (iy <= Hin + delta)
    xs = (torch.floor(ix).clamp(-2, Win) - 1 + PAD).long().clamp(0, Lmap.shape[-1] - 1)
    ys = (torch.floor(iy).clamp(-2, Hin) - 1 + PAD).long().clamp(0, Lmap.shape[-2] - 1)
    idx = (ys * Lmap.shape[-1] + xs).reshape(B, 1, -1).expand(-1, C, -1)
    L = torch.gather(Lmap.reshape(B, C, -1), 2, idx).reshape(B, C, *ix.shape[1:])
    A = torch.gather(Amap.reshape(B, C, -1), 2, idx).reshape(B, C, *ix.shape[1:])
    _, e = torch.frexp(A)
    ulp = torch.where(A > 0, torch.ldexp(torch.ones_like(A), (e - 24).to(A.dtype)), torch.zeros_like(A))
    return torch.where(inside[:, None], L * delta + 4 * ulp, torch.zeros_like(L))


def worst_ratio(out, ref, bound):
    """max |out - ref| / bound (a pixel of bound 0 counts as 0 if exact, inf otherwise)."""
    d = (out.double() - ref).abs()
    r = torch.where(bound > 0, d / torch.where(bound > 0, bound, torch.ones_like(bound)),
                    torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, math.inf)))
    return r.max().item()


# Cases of the GPU parity test: (model, k1, k2 or None, B, cam_batch, C, H, W, Hin, Win, image kind).  k None: drawn
# across dist_range per camera.  Strong distortion (zero padding active), simple_divisional across the t = 0 clamp
# (k1 = 3) and at |k1| <= 1e-4, odd sizes, Hin != H, camera batch 1 and B.
CASES = [
    ("pinhole", None, None, 7, 7, 3, 479, 641, 479, 641, "noise"),
    ("pinhole", None, None, 1, 1, 1, 480, 640, 600, 800, "smooth"),
    ("simple_radial", None, None, 7, 7, 3, 479, 641, 479, 641, "noise"),
    ("simple_radial", 0.7, None, 7, 1, 4, 479, 641, 479, 641, "smooth"),
    ("simple_radial", -0.7, None, 1, 1, 1, 479, 641, 311, 415, "noise"),
    ("radial", None, None, 7, 7, 3, 479, 641, 479, 641, "noise"),
    ("radial", 0.7, 0.7, 7, 1, 1, 479, 641, 521, 700, "smooth"),
    ("radial", -0.7, 0.3, 7, 7, 4, 479, 641, 479, 641, "noise"),
    ("simple_divisional", None, None, 7, 7, 3, 479, 641, 479, 641, "noise"),
    ("simple_divisional", 3.0, None, 7, 1, 3, 479, 641, 479, 641, "smooth"),
    ("simple_divisional", -3.0, None, 1, 1, 4, 479, 641, 400, 500, "noise"),
    ("simple_divisional", 1e-4, None, 7, 1, 3, 479, 641, 479, 641, "noise"),
    ("simple_divisional", -1e-6, None, 7, 1, 1, 479, 641, 479, 641, "noise"),
    ("simple_radial", None, None, 64, 64, 3, 200, 333, 200, 333, "noise"),
    ("simple_divisional", None, None, 64, 1, 1, 200, 333, 250, 300, "smooth"),
]


def case_inputs(case, seed=0):
    """(cams (cam_batch, 8) float32, image (B, C, Hin, Win) float32) of one case."""
    model, k1, k2, B, nb, C, H, W, Hin, Win, kind = case
    return make_cameras(model, nb, H, W, k1, k2, seed), make_images(kind, B, C, Hin, Win, seed)
