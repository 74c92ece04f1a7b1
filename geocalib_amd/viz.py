"""The picture the reference's applications show: the perspective fields of a calibration drawn over the image
(interactive_demo.py: render_frame; viz2d.plot_perspective_fields / plot_confidences).

    draw_perspective_fields(img, camera, gravity, tint=True, contours=True, horizon=False, up=False, confidence=None, ...)

On a HIP device this is ONE launch per 65 535 images (gclm_draw_fields / gclm_draw_fields_u8, csrc/gclm_overlay.hip) that reads
a frame once and writes it once; nothing is copied to the host.  On CPU tensors it is the float32 torch composition below
(`compose`), which is also the readable statement of the definition in include/gclm.h.

The picture is the demo's stated per output pixel and antialiased, NOT cv2's rasteriser bit for bit: end points are not
truncated to integers, and the polylines of cv2.findContours are replaced by the distance to the isoline (|latitude - level|
divided by the latitude's slope in degrees per pixel, in closed form).  The palette lookup is linear between neighbouring
entries, not matplotlib's nearest bin.  Out of scope: the demo's box, grid and text, per-image min/max normalisation of the
confidence heatmap (the range is fixed per call), drawing in place, gradients."""
import ctypes
import math
from dataclasses import dataclass
from typing import Optional, Tuple, Union

import torch

from . import _call, _lib, fields
from .camera import BaseCamera
from .gravity import Gravity

LAT_HI = float(torch.tensor(1 - 1e-6, dtype=torch.float32))      # the latitude's clamp, as gclm_perspective_fields


@dataclass
class OverlayStyle:
    """The numbers of a drawing (struct gclm_overlay_style); `OverlayStyle.default(H, W)` gives the demo's for a frame size."""
    line_halfwidth: float
    arrow_step: int
    arrow_x0: int
    arrow_y0: int
    arrow_length: float
    arrow_halfwidth: float
    arrow_tip: float = 0.3
    tint_alpha: float = 0.4
    heat_alpha: float = 0.4
    levels: int = 15
    heat_range: Tuple[float, float] = (-4.0, 0.0)
    horizon_color: Tuple[int, int, int] = (255, 255, 0)          # the demo's yellow and green, for an RGB image; the colours
    arrow_color: Tuple[int, int, int] = (0, 255, 0)              # are in the image's channel order (a BGR frame: (0, 255, 255))

    @classmethod
    def default(cls, H: int, W: int, **changes) -> "OverlayStyle":
        """The demo's numbers as functions of the frame size, sc = min(H / 640, 2): lines int(5 sc) pixels wide (at least 1), an
        arrow every S = min(W, H) // 10 pixels from (((W % S) + S) // 2, int(0.9 S)), 40 sc long."""
        sc = min(H / 640.0, 2.0)
        half = max(int(5 * sc), 1) / 2
        S = max(min(W, H) // 10, 1)
        return cls(**{**dict(line_halfwidth=half, arrow_step=S, arrow_x0=((W % S) + S) // 2, arrow_y0=int(0.9 * S),
                             arrow_length=40 * sc, arrow_halfwidth=half), **changes})

    def c_struct(self, layers: int) -> "_lib.GclmOverlayStyle":
        st = _lib.GclmOverlayStyle()
        st.struct_size, st.layers = ctypes.sizeof(_lib.GclmOverlayStyle), layers
        st.heat_alpha, st.tint_alpha = self.heat_alpha, self.tint_alpha
        st.heat_lo, st.heat_hi = self.heat_range
        st.levels, st.line_halfwidth = self.levels, self.line_halfwidth
        st.arrow_step, st.arrow_x0, st.arrow_y0 = self.arrow_step, self.arrow_x0, self.arrow_y0
        st.arrow_length, st.arrow_halfwidth, st.arrow_tip = self.arrow_length, self.arrow_halfwidth, self.arrow_tip
        st.horizon_rgba[:3], st.arrow_rgba[:3] = [int(v) for v in self.horizon_color], [int(v) for v in self.arrow_color]
        return st

    def check(self, layers: int) -> None:
        """The conditions of the call on the style (the C entry refuses the same)."""
        ok = 0 <= self.heat_alpha <= 1 and 0 <= self.tint_alpha <= 1 and self.heat_range[1] > self.heat_range[0] and \
            all(math.isfinite(v) for v in self.heat_range) and self.levels >= 2 and \
            all(math.isfinite(v) and v >= 0 for v in (self.line_halfwidth, self.arrow_halfwidth, self.arrow_length))
        if not ok:
            raise ValueError(f"invalid overlay style {self}")
        if layers & _lib.OVERLAY_LAYERS["horizon"] and self.levels % 2 == 0:
            raise ValueError("the horizon is the middle latitude level: `levels` must be odd")
        if layers & _lib.OVERLAY_LAYERS["arrows"]:
            if self.arrow_step < 1 or self.arrow_x0 < 0 or self.arrow_y0 < 0 or not 0 <= self.arrow_tip <= 1:
                raise ValueError(f"invalid arrow grid in {self}")
            if not self.arrow_length + self.arrow_halfwidth + 0.5 <= self.arrow_step:
                raise ValueError(f"arrow_length + arrow_halfwidth + 0.5 = {self.arrow_length + self.arrow_halfwidth + 0.5} must not "
                                 f"exceed arrow_step = {self.arrow_step}: an arrow may reach the pixels of its own cells only")


# ------------------------------------------------------------------ palettes
_SEISMIC = ((0.0, 0.0, 0.3), (0.0, 0.0, 1.0), (1.0, 1.0, 1.0), (1.0, 0.0, 0.0), (0.5, 0.0, 0.0))     # its five anchor colours
_palettes = {}


def _named_palette(name: str) -> torch.Tensor:
    if name == "seismic":              # linear between five equally spaced anchors, 256 entries: no dependency
        x = torch.linspace(0, 4, 256, dtype=torch.float64)
        i = x.floor().clamp(max=3).long()
        a = torch.tensor(_SEISMIC, dtype=torch.float64)
        f = (x - i)[:, None]
        return ((a[i] * (1 - f) + a[i + 1] * f) * 255).round().to(torch.uint8)
    try:
        import matplotlib
        cmap = matplotlib.colormaps[name]
    except ImportError as e:
        raise RuntimeError(f"palette {name!r} needs matplotlib, which cannot be imported; pass a (256, 3) uint8 tensor or "
                           "\"seismic\"") from e
    except KeyError as e:
        raise ValueError(f"matplotlib knows no colormap {name!r}") from e
    return torch.from_numpy(cmap(torch.linspace(0, 1, 256, dtype=torch.float64).numpy(), bytes=True)[:, :3].copy())


def resolve_palette(p: Union[str, torch.Tensor], device) -> torch.Tensor:
    """A palette as the call takes it: (256, 3) uint8, contiguous, on `device`, RGB for a name.  Named palettes are cached per
    (name, device)."""
    device = torch.device(device)
    if isinstance(p, str):
        key = (p, device)
        if key not in _palettes:
            _palettes[key] = _named_palette(p).to(device).contiguous()
        return _palettes[key]
    if p.dtype != torch.uint8 or tuple(p.shape) != (256, 3):
        raise ValueError(f"a palette is a (256, 3) uint8 tensor or a name, got {p.dtype} {tuple(p.shape)}")
    return p.detach().to(device).contiguous()


# ------------------------------------------------------------------ the definition, as a torch composition
def _scales(model: str, k1, k2, r2):
    """(s, s', t, t') of include/gclm.h: the distort scale and ds/dr2 in the forms that do not cancel, the undistort scale and
    dt/dr2."""
    one, zero = torch.ones_like(r2), torch.zeros_like(r2)
    if model == "pinhole":
        return one, zero, one, zero
    if model == "simple_radial":
        return 1 + k1 * r2, k1 * one, 1 - k1 * r2, -k1 * one
    if model == "radial":
        return (1 + (k1 + k2 * r2) * r2, k1 + 2 * k2 * r2, 1 - k1 * r2 + (3 * k1 * k1 - k2) * (r2 * r2),
                -k1 + 2 * (3 * k1 * k1 - k2) * r2)
    kr = k1 * r2
    den = 1 + kr
    t = 1 / torch.where(den == 0, 1e6 * one, den)
    tau = 1 - 4 * kr
    rt = torch.sqrt(tau.clamp(min=0))
    d = 1 + rt
    s = torch.where(tau > 0, 2 / d, 1 / torch.where(kr == 0, one, 2 * kr))
    tt = 1e-3
    den = 2 * k1 * (r2 * r2) * tt
    sp = torch.where(tau >= 1e-6, 4 * k1 / torch.where(rt == 0, one, rt * d * d),
                     (2 * kr - (1 - tt) * tt) / torch.where(den == 0, 1e6 * one, den))
    return torch.where(kr == 0, one, s), torch.where(kr == 0, zero, sp), t, -k1 * t * t


def _lookup(pal: torch.Tensor, tau: torch.Tensor) -> torch.Tensor:
    """pal(L, tau): linear between entries floor(255 tau) and floor(255 tau) + 1 (continuous); `pal` (256, 3) float."""
    p = 255 * tau
    i = p.floor().clamp(0, 254)
    f = (p - i)[..., None]
    i = i.long()
    return pal[i] + (pal[i + 1] - pal[i]) * f


def _coverage(halfwidth: float, d: torch.Tensor) -> torch.Tensor:
    return torch.nan_to_num((halfwidth + 0.5 - d), nan=0.0).clamp(0, 1)


def _segment(wx, wy, dx, dy):
    """Distance from w = P - A to the segment A + s D, s in [0, 1]."""
    len2 = dx * dx + dy * dy
    s = torch.where(len2 > 0, (wx * dx + wy * dy) / torch.where(len2 > 0, len2, torch.ones_like(len2)), torch.zeros_like(len2))
    s = s.clamp(0, 1)
    return torch.sqrt((wx - s * dx) ** 2 + (wy - s * dy) ** 2)


def compose(model: str, cam: torch.Tensor, grav: torch.Tensor, img: torch.Tensor, layers: int, style: OverlayStyle,
            conf: Optional[torch.Tensor] = None, pal: Optional[torch.Tensor] = None, heat_pal: Optional[torch.Tensor] = None,
            unit: float = 1.0) -> torch.Tensor:
    """The definition (include/gclm.h: gclm_draw_fields) in the dtype of `img`: `img` (B, C, H, W) floating, cameras (1 or B, 8),
    gravities (1 or B, 3), palettes (256, 3) uint8; `unit` is a colour byte in the image's units (1 for 0..255 images, 1 / 255
    for 0..1 images).  Returns the drawn image unrounded; channel 3 is copied."""
    L = _lib.OVERLAY_LAYERS
    dt, dev = img.dtype, img.device
    B, C, H, W = img.shape
    out = img[:, :3].permute(0, 2, 3, 1).clone()                 # (B, H, W, 3)
    c, g = cam.to(dev, dt), grav.to(dev, dt)
    fx, fy, cx, cy, k1, k2 = (c[:, i, None, None] for i in range(2, 8))
    a, b, gc = (g[:, i, None, None] for i in range(3))
    deg = 180 / math.pi

    def blend(o, colour, alpha):
        alpha = alpha if isinstance(alpha, float) else alpha[..., None]
        return o * (1 - alpha) + colour * unit * alpha

    if layers & L["heat"]:
        cf = conf.to(dev, dt).reshape(B, H, W)
        lo, hi = style.heat_range
        tau = (torch.log10(cf.clamp(min=1e-6)).clamp(lo, hi) - lo) / (hi - lo)
        ok = torch.isfinite(cf)
        drawn = blend(out, _lookup(heat_pal.to(dev, dt), torch.where(ok, tau, torch.zeros_like(tau))), float(style.heat_alpha))
        out = torch.where(ok[..., None], drawn, out)
    if layers & (L["tint"] | L["contours"] | L["horizon"]):
        x = torch.arange(W, device=dev, dtype=dt)[None, None, :]
        y = torch.arange(H, device=dev, dtype=dt)[None, :, None]
        u, v = ((x - cx) / fx).expand(-1, H, -1), ((y - cy) / fy).expand(-1, -1, W)
        r2 = u * u + v * v
        _, _, t, tp = _scales(model, k1, k2, r2)
        X, Y = u * t, v * t
        n = torch.sqrt(X * X + Y * Y + 1)
        s = (X * a + Y * b + gc) / n
        sc = s.clamp(-LAT_HI, LAT_HI)
        lat = torch.asin(sc) * deg
        gX, gY = (a - s * X / n) / n, (b - s * Y / n) / n
        w = 2 * tp * (u * gX + v * gY)
        sx, sy = (t * gX + w * u) / fx, (t * gY + w * v) / fy
        slope = torch.sqrt(sx * sx + sy * sy) * deg / torch.sqrt((1 - sc) * (1 + sc))
        ok_lat = torch.isfinite(lat)
        ok_line = ok_lat & torch.isfinite(slope)
        lat0 = torch.where(ok_lat, lat, torch.zeros_like(lat))
        dist = 1 / torch.where(ok_line, slope, torch.ones_like(slope)).clamp(min=1e-4)
        if layers & L["tint"]:
            drawn = blend(out, _lookup(pal.to(dev, dt), (lat0 + 90) / 180), float(style.tint_alpha))
            out = torch.where(ok_lat[..., None], drawn, out)
        if layers & L["contours"]:
            last = style.levels - 1
            step = 180 / last
            k = torch.round((lat0 + 90) / step)
            alpha = _coverage(style.line_halfwidth, (lat0 - (2 * k - last) * 90 / last).abs() * dist)       # (level k, exact at 0)
            drawn = blend(out, _lookup(pal.to(dev, dt), k / last), alpha)
            out = torch.where(ok_line[..., None], drawn, out)
        if layers & L["horizon"]:
            alpha = _coverage(style.line_halfwidth, lat0.abs() * dist)
            drawn = blend(out, torch.tensor(style.horizon_color, device=dev, dtype=dt), alpha)
            out = torch.where(ok_line[..., None], drawn, out)
    if layers & L["arrows"]:
        S, Ln = style.arrow_step, float(style.arrow_length)
        ax = torch.arange(style.arrow_x0, max(W, style.arrow_x0), S, device=dev, dtype=dt)
        ay = torch.arange(style.arrow_y0, max(H, style.arrow_y0), S, device=dev, dtype=dt)
        best = torch.zeros((c.shape[0], H, W), device=dev, dtype=dt)
        if ax.numel() and ay.numel():
            u, v = (ax[None, None, :] - cx) / fx, (ay[None, :, None] - cy) / fy            # (n, 1, nx), (n, ny, 1)
            u, v = u.expand(-1, ay.numel(), -1), v.expand(-1, -1, ax.numel())
            s, sp, _, _ = _scales(model, k1, k2, u * u + v * v)
            px, py = a - gc * u, b - gc * v
            o = 2 * sp * (u * px + v * py)
            qx, qy = s * px + o * u, s * py + o * v
            n = torch.sqrt(qx * qx + qy * qy)
            draws = (n >= 1e-6) & torch.isfinite(n)
            n = torch.where(draws, n, torch.ones_like(n))
            ex, ey = qx / n, qy / n
            x = torch.arange(W, device=dev, dtype=dt)[None, None, :]
            y = torch.arange(H, device=dev, dtype=dt)[None, :, None]
            tip = style.arrow_tip * Ln * math.sqrt(0.5)
            for j in range(ay.numel()):
                for i in range(ax.numel()):          # (every anchor against every pixel: the reach condition is not used here)
                    e_x, e_y = ex[:, j, i, None, None], ey[:, j, i, None, None]
                    wx, wy = (x - ax[i]).expand(-1, H, -1), (y - ay[j]).expand(-1, -1, W)
                    d = _segment(wx, wy, Ln * e_x, Ln * e_y)
                    tx, ty = wx - Ln * e_x, wy - Ln * e_y
                    d = torch.minimum(d, _segment(tx, ty, tip * (-e_x - e_y), tip * (-e_y + e_x)))
                    d = torch.minimum(d, _segment(tx, ty, tip * (-e_x + e_y), tip * (-e_y - e_x)))
                    cov = _coverage(style.arrow_halfwidth, d)
                    best = torch.maximum(best, torch.where(draws[:, j, i, None, None], cov, torch.zeros_like(cov)))
        out = blend(out, torch.tensor(style.arrow_color, device=dev, dtype=dt), best)
    out = out.permute(0, 3, 1, 2)
    return out if C == 3 else torch.cat([out, img[:, 3:]], 1)


# ------------------------------------------------------------------ the public call
def draw_perspective_fields(img: torch.Tensor, camera: BaseCamera, gravity: Gravity, *, tint: bool = True, contours: bool = True,
                            horizon: bool = False, up: bool = False, confidence: Optional[torch.Tensor] = None,
                            palette: Union[str, torch.Tensor] = "seismic", heat_palette: Union[str, torch.Tensor] = "turbo",
                            style: Optional[OverlayStyle] = None) -> torch.Tensor:
    """`img` (B, C, H, W), C = 3 or 4, with the perspective fields of `camera` and `gravity` drawn over it: the latitude as a
    tint and as isolines, the horizon, the up field as arrows on a grid, and `confidence` (B, H, W) float32 as a log-scaled
    heatmap under them.  torch.uint8 images are contiguous or channels_last and read as they lie; float32 images are planar,
    nominal range 0..1.  The output has the dtype and memory format of `img`; channel 3 of a C = 4 image is copied.

    `camera` and `gravity` hold one calibration shared by the batch or one per image, at the image's resolution (what
    `calibrate` returns); the call reads nothing back from the device and trusts H, W of the image, not camera.size.
    Palettes: a (256, 3) uint8 tensor in the image's channel order, or a name ("seismic" is built in, other names come from
    matplotlib if it can be imported).  `style`: an OverlayStyle, default OverlayStyle.default(H, W), the demo's numbers.

    One HIP launch per 65 535 images on torch's current stream; on CPU tensors the float32 torch composition of the same
    definition (`compose`), rounded for uint8 as the other image calls round.  Not differentiable.  Not cv2's rasteriser bit
    for bit (module docstring)."""
    if img.dim() != 4 or img.shape[1] not in (3, 4) or img.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"`img` must be (B, 3 or 4, H, W) uint8 or float32, got {img.dtype} {tuple(img.shape)}")
    B, C, H, W = img.shape
    L = _lib.OVERLAY_LAYERS
    layers = (L["heat"] if confidence is not None else 0) | (L["tint"] if tint else 0) | (L["contours"] if contours else 0) | \
        (L["horizon"] if horizon else 0) | (L["arrows"] if up else 0)
    style = style if style is not None else OverlayStyle.default(H, W)
    style.check(layers)
    dev = img.device
    cam, grav = fields._rows(camera._data, 8, dev), fields._rows(gravity._data, 3, dev)
    if cam.shape[0] != grav.shape[0] or cam.shape[0] not in (1, B):
        raise ValueError(f"camera batch {cam.shape[0]} and gravity batch {grav.shape[0]} must be equal, and 1 or {B}")
    if confidence is not None and (confidence.dtype != torch.float32 or confidence.numel() != B * H * W or confidence.device != dev):
        raise ValueError(f"`confidence` must be float32 ({B}, {H}, {W}) on {dev}")
    pal = resolve_palette(palette, dev) if layers & (L["tint"] | L["contours"]) else None
    heat = resolve_palette(heat_palette, dev) if layers & L["heat"] else None
    if B * H * W == 0:
        return img.clone()
    model = camera.name()

    if not img.is_cuda:
        out = compose(model, cam, grav, img.detach().float(), layers, style, confidence, pal, heat,
                      unit=1.0 if img.dtype == torch.uint8 else 1 / 255)
        if img.dtype == torch.uint8:
            out = out.round().clamp(0, 255).to(torch.uint8)
        channels_last = not img.is_contiguous() and img.is_contiguous(memory_format=torch.channels_last)
        return out.contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)

    src, layout, dst, like_input = fields._warp_image(img, (H, W), "draw_perspective_fields")
    conf = None if confidence is None else _call.dev_f32(confidence, "confidence")
    st = style.c_struct(layers)
    for b0, n in _call.slices(B):
        _call.call("gclm_draw_fields_u8" if src.dtype == torch.uint8 else "gclm_draw_fields", _lib.CAMERA_MODEL_IDS[model],
                   fields._rows_at(cam, b0, n)[0], *fields._rows_at(grav, b0, n), src[b0].data_ptr(), n, C, H, W, *layout,
                   _call.ptr_at(conf, b0), _call.ptr(pal), _call.ptr(heat), ctypes.byref(st), dst[b0].data_ptr(),
                   _call.raw_stream(dev), device=dev)
    return like_input(dst)
