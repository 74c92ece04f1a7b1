"""Camera tensors: pinhole, simple radial, radial and simple divisional models.

API-compatible with the reference's geocalib/camera.py (BaseCamera :18, Pinhole :522,
SimpleRadial :565, Radial :663, SimpleDivisional :789, camera_models :945): a `(..., 8)` tensor
`{w, h, fx, fy, cx, cy, k1, k2}` wrapped with accessors, resize / crop bookkeeping and the
(un)distortion maps.  Every model here is *radial*: distort(p) = p * s(r2) and
undistort(p) = p * t(r2) with r2 = |p|^2, so a model only supplies s, t and their derivatives
and all Jacobians follow in closed form (the reference falls back to torch.func.jacfwd for the
generic cases).  Host-side torch code: the per-pixel hot paths are csrc/gclm_pass.hip and, for undistort_image,
get_img_from_pano and reproject_image / upright_image, csrc/gclm_image.hip, csrc/gclm_pano.hip and csrc/gclm_reproject.hip.
"""
from typing import Dict, Tuple, Union

import torch
from torch.nn import functional as F

from .misc import TensorWrapper, autocast
from .utils import deg2rad, focal2fov, fov2focal, rad2rotmat


def _outer(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return a[..., :, None] * b[..., None, :]


def _one_of(pts, p2d):
    """The positional / `pts=` argument or its `p2d=` alias (exactly one of them)."""
    if (pts is None) == (p2d is None):
        raise TypeError("pass the points once: positionally, as pts= or as p2d=")
    return pts if p2d is None else p2d


def _eye_like(p2d: torch.Tensor) -> torch.Tensor:
    return torch.eye(2, device=p2d.device, dtype=p2d.dtype).expand(p2d.shape[:-1] + (2, 2))


class BaseCamera(TensorWrapper):
    """(..., {w, h, fx, fy, cx, cy, k1, k2}) camera parameters."""

    eps = 1e-3
    dist_range = (-0.7, 0.7)

    @autocast
    def __init__(self, data: torch.Tensor):
        assert data.shape[-1] in {6, 7, 8}, data.shape
        if data.shape[-1] != 8:
            data = torch.cat([data, data.new_zeros(data.shape[:-1] + (8 - data.shape[-1],))], -1)
        super().__init__(data)

    # ------------------------------------------------------------------ construction
    @classmethod
    def name(cls) -> str:
        raise NotImplementedError

    @classmethod
    def from_dict(cls, param_dict: Dict[str, torch.Tensor]) -> "BaseCamera":
        """Keys: height, width, one of {f, vfov}, optional cx, cy, scales, and one of
        {dist, k1_hat, k1[, k2]} (same precedence as the reference, camera.py:49-93)."""
        d = {k: v if isinstance(v, torch.Tensor) else torch.tensor(v) for k, v in param_dict.items()}
        param_dict.update(d)
        h, w = d["height"], d["width"]
        cx, cy = d.get("cx", w / 2), d.get("cy", h / 2)
        if "f" in d:
            f = d["f"]
        elif "vfov" in d:
            f = fov2focal(d["vfov"], h)
        else:
            raise ValueError("Focal length or vertical field of view must be provided.")
        if "dist" in d:
            k1 = d["dist"][..., (0,)]
            k2 = d["dist"][..., (1,)] if d["dist"].shape[-1] == 2 else torch.zeros_like(k1)
        elif "k1_hat" in d:
            k1 = d["k1_hat"] * (f / h) ** 2
            k2 = d.get("k2", torch.zeros_like(k1))
        else:
            k1 = d.get("k1", torch.zeros_like(f))
            k2 = d.get("k2", torch.zeros_like(f))
        fx, fy = f, f
        if "scales" in d:
            fx = fx * d["scales"][..., 0] / d["scales"][..., 1]
        return cls(torch.stack([w, h, fx, fy, cx, cy, k1, k2], dim=-1))

    def pinhole(self):
        """Same intrinsics without distortion."""
        return self.__class__(self._data[..., :6])

    def _rebuild(self, size=None, f=None, c=None, dist=None):
        size = self.size if size is None else size
        f = self.f if f is None else f
        c = self.c if c is None else c
        if dist is None:
            dist = self.dist if hasattr(self, "dist") else self.new_zeros(self.f.shape)
        return self.__class__(torch.cat([size, f, c, dist], -1))

    # ------------------------------------------------------------------ accessors
    @property
    def size(self) -> torch.Tensor:
        return self._data[..., :2]

    @property
    def f(self) -> torch.Tensor:
        return self._data[..., 2:4]

    @property
    def c(self) -> torch.Tensor:
        return self._data[..., 4:6]

    @property
    def vfov(self) -> torch.Tensor:
        return focal2fov(self.f[..., 1], self.size[..., 1])

    @property
    def hfov(self) -> torch.Tensor:
        return focal2fov(self.f[..., 0], self.size[..., 0])

    @property
    def K(self) -> torch.Tensor:
        K = self._data.new_zeros(self.shape + (3, 3))
        K[..., 0, 0], K[..., 1, 1] = self.f[..., 0], self.f[..., 1]
        K[..., 0, 2], K[..., 1, 2] = self.c[..., 0], self.c[..., 1]
        K[..., 2, 2] = 1
        return K

    # ------------------------------------------------------------------ parameter updates
    def update_focal(self, delta: torch.Tensor, as_log: bool = False):
        """f <- f + delta (or exp(log f + delta)), clamped to a vertical fov in [5, 150] degrees of
        the image HEIGHT for both axes; fx follows fy with the previous aspect (camera.py:136-152)."""
        f = torch.exp(torch.log(self.f) + delta) if as_log else self.f + delta
        ones = self.new_ones(self.shape[0])
        lo = fov2focal(ones * deg2rad(150), self.size[..., 1]).unsqueeze(-1)
        hi = fov2focal(ones * deg2rad(5), self.size[..., 1]).unsqueeze(-1)
        fy = torch.minimum(torch.maximum(f, lo), hi)[..., 1]
        return self._rebuild(f=torch.stack([fy * self.f[..., 0] / self.f[..., 1], fy], -1))

    def update_dist(self, delta: torch.Tensor, dist_range: Tuple[float, float] = None):
        lo, hi = dist_range or self.dist_range
        return self._rebuild(dist=(self.dist + self.new_ones(self.dist.shape) * delta).clamp(lo, hi))

    def scale(self, scales: Union[float, int, Tuple[Union[float, int]]]):
        """Intrinsics after resizing the image by `scales` (sx, sy)."""
        scales = (scales, scales) if isinstance(scales, (int, float)) else scales
        s = scales if isinstance(scales, torch.Tensor) else self.new_tensor(scales)
        return self._rebuild(size=self.size * s, f=self.f * s, c=self.c * s)

    def crop(self, pad: Tuple[float]):
        """Intrinsics after padding (+) / cropping (-) the image by `pad` pixels in total per axis."""
        pad = pad if isinstance(pad, torch.Tensor) else self.new_tensor(pad)
        return self._rebuild(size=self.size + pad.to(self.size), c=self.c + pad.to(self.c) / 2)

    def undo_scale_crop(self, data: Dict[str, torch.Tensor]):
        cam = self.crop(-data["crop_pad"]) if "crop_pad" in data else self
        return cam.scale(1.0 / data["scales"])

    # ------------------------------------------------------------------ radial model hooks
    def _k(self, i: int) -> torch.Tensor:
        return self._data[..., 6 + i][..., None, None]

    def _distort_scale(self, r2: torch.Tensor) -> torch.Tensor:
        """s(r2) with distort(p) = p * s(|p|^2)."""
        raise NotImplementedError

    def _distort_scale_dr2(self, r2: torch.Tensor) -> torch.Tensor:
        """ds/dr2."""
        raise NotImplementedError

    def _undistort_scale(self, r2: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def _undistort_scale_dr2(self, r2: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def check_valid(self, p2d: torch.Tensor) -> torch.Tensor:
        return p2d.new_ones(p2d.shape[:-1]).bool()

    # The reference names the argument `pts` on BaseCamera (camera.py:212,242) and `p2d` on the distortion models
    # (camera.py:611,631,712,737,829,863); one body serves them all here, so both keywords are accepted.
    def distort(self, pts: torch.Tensor = None, return_scale: bool = False, *, p2d: torch.Tensor = None):
        """Distort normalised coordinates; (scale, None) with return_scale."""
        pts = _one_of(pts, p2d)
        s = self._distort_scale((pts**2).sum(-1, keepdim=True))
        return (s, None) if return_scale else (pts * s, self.check_valid(pts))

    def undistort(self, pts: torch.Tensor = None, *, p2d: torch.Tensor = None):
        pts = _one_of(pts, p2d)
        return pts * self._undistort_scale((pts**2).sum(-1, keepdim=True)), self.check_valid(pts)

    def J_distort(self, p2d: torch.Tensor, wrt: str = "pts") -> torch.Tensor:
        r2 = (p2d**2).sum(-1, keepdim=True)
        if wrt == "pts":                      # d(p s)/dp = s I + 2 s' p p^T
            return self._distort_scale(r2)[..., None] * _eye_like(p2d) + \
                2 * self._distort_scale_dr2(r2)[..., None] * _outer(p2d, p2d)
        if wrt == "scale2pts":                # ds/dp = 2 s' p
            return 2 * self._distort_scale_dr2(r2) * p2d
        if wrt == "scale2dist":               # ds/dk_j  (..., N, nd)
            return self._hook_ddist("_distort_scale", p2d)
        raise NotImplementedError(f"Jacobian not implemented for wrt={wrt}")

    def J_undistort(self, p2d: torch.Tensor, wrt: str = "pts") -> torch.Tensor:
        r2 = (p2d**2).sum(-1, keepdim=True)
        if wrt == "pts":
            return self._undistort_scale(r2)[..., None] * _eye_like(p2d) + \
                2 * self._undistort_scale_dr2(r2)[..., None] * _outer(p2d, p2d)
        raise NotImplementedError(f"Jacobian not implemented for wrt={wrt}")

    @autocast
    def up_projection_offset(self, p2d: torch.Tensor) -> torch.Tensor:
        """ds/dp of the distortion scale (enters the distorted up field, perspective_fields.py:72)."""
        return self.J_distort(p2d, wrt="scale2pts")

    # Generic derivatives of the radial hooks by autograd (the models with closed forms override the public
    # methods; the reference's generic versions use torch.func.jacfwd per point, camera.py:216-298).
    def _per_point(self, p2d: torch.Tensor):
        """One camera row per point, distortion parameters as a differentiable leaf: (camera, r2, dist)."""
        n = p2d.shape[-2]
        data = self._data.reshape(-1, self._data.shape[-1])
        rows = data[:, None, :].expand(-1, n, -1).reshape(-1, data.shape[-1])
        nd = self.num_dist_params() if hasattr(self, "num_dist_params") else 0
        dist = rows[:, 6:6 + nd].detach().clone().requires_grad_(True)
        cam = self.__class__(torch.cat([rows[:, :6].detach(), dist, rows[:, 6 + nd:].detach()], -1))
        r2 = (p2d.detach() ** 2).sum(-1).reshape(-1, 1, 1)
        return cam, r2, dist

    def _hook_dr2(self, hook_name: str, r2: torch.Tensor) -> torch.Tensor:
        """d hook(r2) / d r2 (elementwise)."""
        x = r2.detach().clone().requires_grad_(True)
        with torch.enable_grad():
            (g,) = torch.autograd.grad((getattr(self, hook_name)(x) + 0 * x).sum(), x)     # 0*x: constant hooks
        return g

    def _hook_ddist(self, hook_name: str, p2d: torch.Tensor) -> torch.Tensor:
        """d hook(|p|^2) / d dist per point: (..., N, num_dist)."""
        with torch.enable_grad():
            cam, r2, dist = self._per_point(p2d)
            (g,) = torch.autograd.grad(getattr(cam, hook_name)(r2).sum() + 0 * dist.sum(), dist)
        return g.reshape(*p2d.shape[:-1], -1)

    def J_up_projection_offset(self, p2d: torch.Tensor, wrt: str = "uv") -> torch.Tensor:
        """Jacobian of up_projection_offset(p) = 2 s'(r2) p: wrt "uv" (..., N, 2, 2), wrt "dist" (..., N, 2, nd)."""
        r2 = (p2d**2).sum(-1, keepdim=True)
        if wrt == "uv":        # 2 s' I + 4 s'' p p^T
            s2 = self._hook_dr2("_distort_scale_dr2", r2)
            return 2 * self._distort_scale_dr2(r2)[..., None] * _eye_like(p2d) + 4 * s2[..., None] * _outer(p2d, p2d)
        if wrt == "dist":      # 2 p ds'/dk_j
            return 2 * p2d[..., None] * self._hook_ddist("_distort_scale_dr2", p2d)[..., None, :]
        raise NotImplementedError(f"Jacobian not implemented for wrt={wrt}")

    # ------------------------------------------------------------------ projection chain
    @autocast
    def in_image(self, p2d: torch.Tensor):
        assert p2d.shape[-1] == 2
        return torch.all((p2d >= 0) & (p2d <= (self.size.unsqueeze(-2) - 1)), -1)

    @autocast
    def project(self, p3d: torch.Tensor):
        """(x, y, z) -> (x/z, y/z) and the z > eps visibility mask."""
        z = p3d[..., -1]
        return p3d[..., :-1] / z.clamp(min=self.eps).unsqueeze(-1), z > self.eps

    def J_project(self, p3d: torch.Tensor):
        x, y, z = p3d[..., 0], p3d[..., 1], p3d[..., 2].clamp(min=self.eps)
        zero = torch.zeros_like(z)
        return torch.stack([1 / z, zero, -x / z**2, zero, 1 / z, -y / z**2], -1).reshape(p3d.shape[:-1] + (2, 3))

    @autocast
    def denormalize(self, p2d: torch.Tensor) -> torch.Tensor:
        return p2d * self.f.unsqueeze(-2) + self.c.unsqueeze(-2)

    def J_denormalize(self):
        return torch.diag_embed(self.f)

    @autocast
    def normalize(self, p2d: torch.Tensor) -> torch.Tensor:
        return (p2d - self.c.unsqueeze(-2)) / self.f.unsqueeze(-2)

    def J_normalize(self, p2d: torch.Tensor, wrt: str = "f"):
        if wrt == "f":
            return torch.diag_embed(-(p2d - self.c.unsqueeze(-2)) / self.f.unsqueeze(-2) ** 2)
        if wrt == "pts":
            return torch.diag_embed(1 / self.f)
        raise NotImplementedError(f"Jacobian not implemented for wrt={wrt}")

    def pixel_coordinates(self) -> torch.Tensor:
        """(B, h*w, 2) integer pixel grid, row-major, x in [0, w), y in [0, h) (no half-pixel offset)."""
        w, h = (int(v) for v in self.size[0].round().tolist())
        ys, xs = torch.meshgrid(torch.arange(h, dtype=self.dtype, device=self.device),
                                torch.arange(w, dtype=self.dtype, device=self.device), indexing="ij")
        xy = torch.stack((xs, ys), -1).reshape(-1, 2)
        return xy.unsqueeze(0).expand(self.shape[0], -1, -1)

    @autocast
    def pixel_bearing_many(self, p3d: torch.Tensor) -> torch.Tensor:
        return F.normalize(p3d, dim=-1)

    @autocast
    def world2image(self, p3d: torch.Tensor):
        p2d, visible = self.project(p3d)
        p2d, mask = self.distort(p2d)
        p2d = self.denormalize(p2d)
        return p2d, visible & mask & self.in_image(p2d)

    @autocast
    def J_world2image(self, p3d: torch.Tensor):
        p2d, valid = self.project(p3d)
        J = self.J_denormalize().unsqueeze(-3) @ self.J_distort(p2d) @ self.J_project(p3d)
        return J, valid

    @autocast
    def image2world(self, p2d: torch.Tensor):
        p2d, valid = self.undistort(self.normalize(p2d))
        return torch.cat([p2d, p2d.new_ones(p2d.shape[:-1] + (1,))], -1), valid

    @autocast
    def J_image2world(self, p2d: torch.Tensor, wrt: str = "f"):
        if wrt == "dist":
            return self.J_undistort(self.normalize(p2d), wrt)
        if wrt == "f":
            return self.J_undistort(self.normalize(p2d), "pts") @ self.J_normalize(p2d, wrt)
        raise ValueError(f"Unknown wrt: {wrt}")

    @autocast
    def undistort_image(self, img: torch.Tensor) -> torch.Tensor:
        """Remove the distortion from `img` (B, C, Hin, Win): (B, C, H, W) with (W, H) = self.size truncated, as the
        reference's camera.py:396-412, which asserts B = 1.  Here the camera batch is 1 (shared by every image) or B (one
        camera per image, all of one size).  Output pixel (x, y) samples the image bilinearly at
        denormalize(distort(normalize(x, y))), scaled by (Win - 1) / (W - 1), (Hin - 1) / (H - 1), with zero padding
        (F.grid_sample(bilinear, zeros, align_corners=True)).

        A float32 image on a HIP device runs one gclm_undistort_image launch (not differentiable); a non-finite
        coordinate gives 0 there.  Every other input (CPU, other dtypes) runs the reference's torch composition.  The two
        differ for simple_divisional at small |k1 r2|: the torch path keeps the reference's cancelling float32 form of the
        distort scale, the HIP path evaluates the identical 2 / (1 + sqrt(1 - 4 k1 r2)), held to float64.

        A uint8 image gives a uint8 image in its memory format: the float32 sample rounded to nearest, ties to even, saturated
        to 0..255.  On a HIP device that is one gclm_undistort_image_u8 launch, which reads a contiguous image, or a
        channels_last one of up to 4 channels (a decoded frame, H x W x C in memory), as it lies; elsewhere the composition
        runs on img.float()."""
        assert img.dim() == 4, f"expected a (B, C, H, W) image, got {tuple(img.shape)}"
        data = self._data.reshape(-1, self._data.shape[-1])
        n, B = data.shape[0], img.shape[0]
        assert n in (1, B), f"camera batch {n} must be 1 or the image batch {B}"
        if n > 1:
            assert data[:, 0].unique().shape[0] == 1, "All images must have the same width."
            assert data[:, 1].unique().shape[0] == 1, "All images must have the same height."
        W, H = (int(v) for v in data[0, :2].int().tolist())
        if img.is_cuda and img.dtype in (torch.float32, torch.uint8):
            from .fields import undistort_image
            return undistort_image(self.name(), data, img, (H, W))
        if img.dtype == torch.uint8:
            return _to_u8(self.undistort_image(img.float()), img)
        cam = self.__class__(data)
        x, y = torch.meshgrid(torch.arange(0, W), torch.arange(0, H), indexing="xy")
        coords = torch.stack((x, y), dim=-1).reshape(-1, 2).to(device=self.device, dtype=self.dtype)
        p3d, _ = cam.pinhole().image2world(coords.expand(n, -1, -1))
        p2d, _ = cam.world2image(p3d)
        grid = p2d.reshape(n, H, W, 2)
        grid = 2.0 * grid / torch.tensor([W - 1, H - 1]).to(grid) - 1
        return F.grid_sample(img, grid.expand(B, -1, -1, -1).to(img), align_corners=True)

    def get_img_from_pano(self, pano_img: torch.Tensor, gravity, yaws=0.0, resize_factor=None) -> torch.Tensor:
        """Render perspective images (n, C, h, w) from an equirectangular panorama, as the reference's camera.py:414-514:
        image i looks along the rotation R_i = gravity.R[i] @ rad2rotmat(0, 0, yaws[i]), and its pixel (x, y) samples the
        panorama bilinearly (zero padding, align_corners=True, no wrap at the +-pi seam) at
            ix = (lon / pi + 1) / 2 (Ws - 1),   iy = (2 lat / pi + 1) / 2 (Hs - 1)
        where (lon, lat) are the spherical angles of its undistorted bearing and Hs x Ws the panorama's size.

        n = len(yaws) (a scalar yaw is a list of one); the camera and gravity batches broadcast against it and must each be 1
        or the broadcast size.  As in the reference, n cameras with ONE yaw give one image, rendered from camera 0.
        resize_factor (a scalar, or one per image) first resizes the panorama to int(Hp scale) x int(Wp scale) with
        scale = pi / vfov_i * h / Hp * resize_factor[i] in the camera's dtype (bicubic if scale >= 1, else area, clamped to the
        panorama's range); each distinct target shape is resized once.  `pano_img` is (C, Hp, Wp) or (1, C, Hp, Wp); as an
        extension it may also be (n, C, Hp, Wp), one panorama per image.

        A float32 panorama on a HIP device runs one gclm_render_from_pano launch per 192 images (not differentiable; a
        non-finite coordinate gives 0).  Every other input (CPU, other dtypes, a resized side < 2) runs the reference's torch
        composition.  The method reads the device once: the camera sizes, and with resize_factor the vfovs and factors, in
        one .tolist()."""
        assert isinstance(pano_img, torch.Tensor), "Panorama image must be a torch.Tensor."
        data = self._data.reshape(-1, self._data.shape[-1])
        if isinstance(yaws, (int, float)):
            yaws = [yaws]
        if isinstance(resize_factor, (int, float)):
            resize_factor = [resize_factor]
        yaws = yaws.to(self.dtype).to(self.device) if isinstance(yaws, torch.Tensor) else self.new_tensor(yaws)
        yaws = yaws.reshape(-1)
        if isinstance(resize_factor, torch.Tensor):
            resize_factor = resize_factor.to(self.dtype).to(self.device).reshape(-1)
        elif resize_factor is not None:
            resize_factor = self.new_tensor(resize_factor).reshape(-1)
        pano = pano_img if pano_img.dim() == 4 else pano_img.unsqueeze(0)
        n, nc, ng = yaws.shape[0], data.shape[0], gravity._data.reshape(-1, 3).shape[0]
        N = max(n, nc, ng)
        if n < 1 or any(b not in (1, N) for b in (n, nc, ng)):
            raise ValueError(f"camera batch {nc}, gravity batch {ng} and {n} yaws do not broadcast")
        if pano.shape[0] not in (1, n):
            raise ValueError(f"panorama batch {pano.shape[0]} must be 1 or the number of yaws {n}")
        if resize_factor is not None and resize_factor.shape[0] not in (1, n):
            raise ValueError(f"{resize_factor.shape[0]} resize factors for {n} yaws")

        # the one device-to-host read: sizes (and vfovs, resize factors)
        parts = [data[:, 0], data[:, 1]] + ([] if resize_factor is None else [self.vfov.reshape(-1), resize_factor])
        host = torch.cat(parts).tolist()
        ws, hs = host[:nc], host[nc:2 * nc]
        assert len(set(ws)) == 1, "All images must have the same width."
        assert len(set(hs)) == 1, "All images must have the same height."
        w, h = int(round(ws[0])), int(round(hs[0]))

        # per image: (panorama index, resized (H', W') or None, interpolation mode); each distinct one is resized once
        Hp, Wp = pano.shape[-2:]
        targets = []
        for i in range(n):
            p = i if pano.shape[0] > 1 else 0
            if resize_factor is None:
                targets.append((p, None, None))
                continue
            vfov, rf = host[2 * nc + (i if nc > 1 else 0)], host[3 * nc + (i if resize_factor.shape[0] > 1 else 0)]
            scale = torch.pi / float(vfov) * float(h) / Hp * torch.tensor(rf, dtype=self.dtype)
            shape = (int(Hp * scale), int(Wp * scale))
            targets.append((p, shape, "bicubic" if scale >= 1 else "area"))
        panos = {}
        for key in targets:
            if key not in panos:
                p, shape, mode = key
                src = pano[p:p + 1]
                # clamp as bicubic interpolation can over- or under-shoot
                panos[key] = src if shape is None else F.interpolate(src, size=shape, mode=mode).clamp(src.min(), src.max())

        R_yaw = rad2rotmat(yaws.new_zeros(yaws.shape), yaws.new_zeros(yaws.shape), yaws)
        if pano.is_cuda and pano.dtype == torch.float32 and all(min(v.shape[-2:]) >= 2 for v in panos.values()):
            from .fields import render_from_pano
            rot = (gravity.R.reshape(-1, 3, 3).to(R_yaw) @ R_yaw)[:n]
            return render_from_pano(self.name(), data[:n] if nc > 1 else data[:1], rot, [panos[k][0] for k in targets],
                                    (h, w))

        # the reference's torch composition
        cam = self.__class__(data)
        uv1, _ = cam.image2world(cam.pixel_coordinates())
        bearings = cam.pixel_bearing_many(uv1)
        rotated_bearings = bearings @ gravity.R @ R_yaw
        lon = torch.atan2(rotated_bearings[..., 0], rotated_bearings[..., 2])
        lat = torch.atan2(rotated_bearings[..., 1], torch.norm(rotated_bearings[..., [0, 2]], dim=-1))
        images = []
        for idx, key in enumerate(targets):
            resized_pano = panos[key]
            pano_shape = key[1] if key[1] is not None else resized_pano.shape[-2:][::-1]
            min_lon, max_lon = -torch.pi, torch.pi
            min_lat, max_lat = -torch.pi / 2.0, torch.pi / 2.0
            min_x, max_x = 0, pano_shape[0] - 1.0
            min_y, max_y = 0, pano_shape[1] - 1.0
            nx = (lon[idx] - min_lon) / (max_lon - min_lon) * (max_x - min_x) + min_x
            ny = (lat[idx] - min_lat) / (max_lat - min_lat) * (max_y - min_y) + min_y
            grid = torch.stack((nx.reshape((1, h, w)), ny.reshape((1, h, w))), dim=-1)
            grid = 2.0 * grid / torch.tensor([pano_shape[-2] - 1, pano_shape[-1] - 1]).to(grid) - 1
            images.append(F.grid_sample(resized_pano, grid.to(resized_pano), align_corners=True))
        return torch.cat(images, 0)

    def reproject_image(self, img: torch.Tensor, target: "BaseCamera" = None, rotation: torch.Tensor = None,
                        return_valid: bool = False):
        """`img` (B, C, Hin, Win), taken with this camera, as the camera `target` sees it after turning by `rotation`:
        (B, C, H, W) with (W, H) the target's size truncated.  Levelling a horizon (upright_image), rendering into a wider
        or longer camera, distorting a clean image (the inverse of undistort_image) and a virtual pan or tilt are all this
        one operation.  `self` has batch 1 or B; `target` is a camera of any of the four models, batch 1 or B, all of one
        size (default: this camera without its distortion); `rotation` is M (3, 3), (1, 3, 3) or (B, 3, 3), None for the
        identity.  Output pixel (x, y), integer pixel centres:
            b = target.image2world(x, y) = (u t, v t, 1),   q = b @ M,   visible = q_z > eps (1e-3, as project())
            p = (q_x, q_y) / q_z,  r2 = |p|^2,  (s, s') = this model's distort scale at r2 and ds/dr2
            inside_model = s + 2 r2 s' > 0          (r s(r^2) still increases: beyond, a polynomial model folds back)
            ix = (p_x s fx + cx) (Win - 1) / (Ws - 1),   iy = (p_y s fy + cy) (Hin - 1) / (Hs - 1)
        with (Ws, Hs) this camera's size truncated (the image may be stored at another resolution, as for
        undistort_image), sampled bilinearly with zero padding (F.grid_sample(bilinear, zeros, align_corners=True)); exactly
        0 where visible or inside_model fails or a coordinate is not finite.  With `return_valid` also the (B, H, W) bool
        mask visible & inside_model & 0 <= ix <= Win - 1 & 0 <= iy <= Hin - 1.

        A float32 image on a HIP device runs one gclm_reproject_image launch (not differentiable).  Every other input (CPU,
        other dtypes) runs a torch composition of the same definition, simple_divisional's scales in the forms that do not
        cancel (csrc/gclm_render.h).  A uint8 image gives a uint8 image in its memory format, as for undistort_image
        (gclm_reproject_image_u8 on a HIP device).  The method reads the device once: the two cameras' sizes, in one
        .tolist()."""
        if img.dim() != 4:
            raise ValueError(f"expected a (B, C, H, W) image, got {tuple(img.shape)}")
        B = img.shape[0]
        src = self._data.reshape(-1, self._data.shape[-1])
        if target is None:
            tgt_name, tgt = "pinhole", torch.cat([src[:, :6], torch.zeros_like(src[:, 6:])], -1)
        elif isinstance(target, BaseCamera):
            tgt_name, tgt = target.name(), target._data.reshape(-1, target._data.shape[-1]).to(src)
        else:
            raise ValueError(f"`target` must be a camera of one of the four models, got {type(target).__name__}")
        rot = None
        if rotation is not None:
            if rotation.dim() not in (2, 3) or rotation.shape[-2:] != (3, 3):
                raise ValueError(f"`rotation` must be (3, 3), (1, 3, 3) or (B, 3, 3), got {tuple(rotation.shape)}")
            rot = rotation.to(src).reshape(-1, 3, 3)
        for what, n in (("source camera", src.shape[0]), ("target camera", tgt.shape[0]),
                        ("rotation", 1 if rot is None else rot.shape[0])):
            if n not in (1, B):
                raise ValueError(f"{what} batch {n} must be 1 or the image batch {B}")
        ns, nt = src.shape[0], tgt.shape[0]
        host = torch.cat([src[:, :2].reshape(-1), tgt[:, :2].reshape(-1)]).tolist()      # the one device-to-host read
        sizes_s, sizes_t = set(zip(host[0:2 * ns:2], host[1:2 * ns:2])), set(zip(host[2 * ns::2], host[2 * ns + 1::2]))
        assert len(sizes_s) == 1, "All source cameras must have the same size."
        assert len(sizes_t) == 1, "All target cameras must have the same size."
        (Ws, Hs), (W, H) = (tuple(int(v) for v in s.pop()) for s in (sizes_s, sizes_t))
        if min(Ws, Hs) < 2 or min(W, H) < 1:
            raise ValueError(f"source camera size {Ws} x {Hs} must be at least 2 x 2, target size {W} x {H} at least 1 x 1")
        if ns != nt:                                                      # one batch for both cameras
            src, tgt = src.expand(B, -1), tgt.expand(B, -1)
        if img.is_cuda and img.dtype in (torch.float32, torch.uint8):
            from .fields import reproject_image
            return reproject_image(self.name(), src, tgt_name, tgt, rot, img, (Hs, Ws), (H, W), return_valid)
        if img.dtype == torch.uint8:
            out, valid = _reproject_torch(self.name(), src, tgt_name, tgt, rot, img.float(), (Hs, Ws), (H, W))
            out = _to_u8(out, img)
        else:
            out, valid = _reproject_torch(self.name(), src, tgt_name, tgt, rot, img, (Hs, Ws), (H, W))
        return (out, valid) if return_valid else out

    def upright_image(self, img: torch.Tensor, gravity, level_pitch: bool = False, target: "BaseCamera" = None,
                      return_valid: bool = False):
        """`img` (B, C, Hin, Win) with the roll that `gravity` says the camera had removed, and with `level_pitch` the pitch
        too (the horizon then runs through the principal point): reproject_image with M = R_t @ R_s^T, R_s = gravity.R and
        R_t = Gravity.from_rp(0, 0 if level_pitch else gravity.pitch).R.  The gravity batch is 1 or B; `target` and
        `return_valid` as for reproject_image."""
        from .gravity import Gravity
        R_s = gravity.R.reshape(-1, 3, 3)
        pitch = gravity.pitch.reshape(-1)
        zero = torch.zeros_like(pitch)
        R_t = Gravity.from_rp(zero, zero if level_pitch else pitch).R.reshape(-1, 3, 3)
        return self.reproject_image(img, target, R_t @ R_s.transpose(-1, -2), return_valid)

    def __repr__(self):
        return f"{self.__class__.__name__} {self.shape} {self.dtype} {self.device}"


def _to_u8(out: torch.Tensor, img: torch.Tensor) -> torch.Tensor:
    """The float32 composition of a uint8 image `img` as bytes: rounded to nearest, ties to even (torch.round), saturated to
    0..255, in the memory format of `img` -- the definition of the HIP path (include/gclm.h: gclm_undistort_image_u8)."""
    out = out.round().clamp(0, 255).to(torch.uint8)
    if not img.is_contiguous() and img.is_contiguous(memory_format=torch.channels_last):
        return out.contiguous(memory_format=torch.channels_last)
    return out.contiguous()


def _render_scales(model: str, k1: torch.Tensor, k2: torch.Tensor, r2: torch.Tensor):
    """(t, s, s') at r2 as the render kernels evaluate them (csrc/gclm_render.h): the undistort scale, the distort scale and
    ds/dr2, simple_divisional's in the forms that do not cancel."""
    one, zero = torch.ones_like(r2), torch.zeros_like(r2)
    if model == "pinhole":
        return one, one, zero
    if model == "simple_radial":
        return 1 - k1 * r2, 1 + k1 * r2, k1 + zero
    if model == "radial":
        return 1 - k1 * r2 + (3 * k1 * k1 - k2) * (r2 * r2), 1 + (k1 + k2 * r2) * r2, k1 + 2 * k2 * r2
    den = 1 + k1 * r2
    t = 1 / torch.where(den == 0, 1e6 * one, den)
    kr = k1 * r2
    tau = 1 - 4 * kr
    rt = torch.sqrt(tau.clamp(min=0))
    d = 1 + rt
    s = torch.where(tau > 0, 2 / d, 1 / torch.where(kr == 0, one, 2 * kr))
    tt = 1e-6 ** 0.5
    den = 2 * k1 * (r2 * r2) * tt
    sp = torch.where(tau >= 1e-6, 4 * k1 / torch.where(tau >= 1e-6, rt * d * d, one),
                     (2 * kr - (1 - tt) * tt) / torch.where(den == 0, 1e6 * one, den))
    return t, torch.where(kr == 0, one, s), torch.where(kr == 0, zero, sp)


def _reproject_torch(src_model, src, tgt_model, tgt, rot, img, src_size, size):
    """BaseCamera.reproject_image as a torch composition: cameras (n, 8) of one batch n in {1, B}, `rot` (1 or B, 3, 3) or
    None; returns the (B, C, H, W) image and the (B, H, W) bool mask."""
    grid, seen, valid = _reproject_grid(src_model, src, tgt_model, tgt, rot, img.shape, src_size, size)
    out = F.grid_sample(img, grid.to(img), mode="bilinear", padding_mode="zeros", align_corners=True)
    return torch.where(seen[:, None].to(img.device), out, torch.zeros_like(out)), valid


def _reproject_grid(src_model, src, tgt_model, tgt, rot, img_shape, src_size, size):
    """The sampling grid of _reproject_torch (B, H, W, 2) in F.grid_sample's normalised coordinates, the (B, H, W) mask of
    the pixels that sample at all (visible, inside the model, finite) and the (B, H, W) valid mask."""
    (Hs, Ws), (H, W) = src_size, size
    B, _, Hin, Win = img_shape
    assert min(Hin, Win) >= 2, "the torch composition needs a source image of at least 2 x 2"
    fxs, fys, cxs, cys, k1s, k2s = (src[:, i, None, None] for i in range(2, 8))
    fxt, fyt, cxt, cyt, k1t, k2t = (tgt[:, i, None, None] for i in range(2, 8))
    x = torch.arange(W, device=src.device, dtype=src.dtype)[None, None, :]
    y = torch.arange(H, device=src.device, dtype=src.dtype)[None, :, None]
    u, v = (x - cxt) / fxt, (y - cyt) / fyt
    t = _render_scales(tgt_model, k1t, k2t, u * u + v * v)[0]
    qx, qy, qz = u * t, v * t, torch.ones_like(u * t)
    if rot is not None:
        M = rot[:, :, :, None, None]
        qx, qy, qz = (qx * M[:, 0, j] + qy * M[:, 1, j] + M[:, 2, j] for j in range(3))
    ok = (qz > BaseCamera.eps) & torch.isfinite(qz)
    iz = 1 / torch.where(ok, qz, torch.ones_like(qz))
    px, py = qx * iz, qy * iz
    r2 = px * px + py * py
    _, s, sp = _render_scales(src_model, k1s, k2s, r2)
    ok = ok & (s + 2 * r2 * sp > 0)
    ix, iy = (px * s * fxs + cxs) * ((Win - 1) / (Ws - 1)), (py * s * fys + cys) * ((Hin - 1) / (Hs - 1))
    ok = ok.expand(B, -1, -1)
    ix, iy = ix.expand(B, -1, -1), iy.expand(B, -1, -1)
    valid = ok & (ix >= 0) & (ix <= Win - 1) & (iy >= 0) & (iy <= Hin - 1)
    seen = ok & torch.isfinite(ix) & torch.isfinite(iy)
    outside = torch.full_like(ix, -2.0)                 # where no tap lies inside the source
    gx, gy = torch.where(seen, ix, outside).clamp(-2, Win + 1), torch.where(seen, iy, outside).clamp(-2, Hin + 1)
    return torch.stack([2 * gx / (Win - 1) - 1, 2 * gy / (Hin - 1) - 1], -1), seen, valid


class Pinhole(BaseCamera):
    """No distortion."""

    @classmethod
    def name(cls) -> str:
        return "pinhole"

    def distort(self, p2d: torch.Tensor, return_scale: bool = False):
        if return_scale:
            return p2d.new_ones(p2d.shape[:-1] + (1,))
        return p2d, p2d.new_ones((p2d.shape[0], 1)).bool()

    def undistort(self, pts: torch.Tensor):
        return pts, pts.new_ones((pts.shape[0], 1)).bool()

    def J_distort(self, p2d: torch.Tensor, wrt: str = "pts") -> torch.Tensor:
        if wrt == "pts":
            return _eye_like(p2d)
        raise ValueError(f"Unknown wrt: {wrt}")

    J_undistort = J_distort

    def J_up_projection_offset(self, p2d: torch.Tensor, wrt: str = "uv") -> torch.Tensor:
        if wrt == "uv":
            return torch.zeros(p2d.shape[:-1] + (2, 2), device=p2d.device, dtype=p2d.dtype)
        raise ValueError(f"Unknown wrt: {wrt}")


class _OneParam(BaseCamera):
    """Models with a single coefficient k1 (`dist` still spans both storage slots, as upstream)."""

    @property
    def dist(self) -> torch.Tensor:
        return self._data[..., 6:]

    @classmethod
    def num_dist_params(cls) -> int:
        return 1

    @property
    def k1(self) -> torch.Tensor:
        return self._data[..., 6]


class SimpleRadial(_OneParam):
    """s = 1 + k1 r2; inverse approximated by t = 1 - k1 r2 (Drap & Lefevre)."""

    @classmethod
    def name(cls) -> str:
        return "simple_radial"

    @property
    def k1_hat(self) -> torch.Tensor:
        return self.k1 / (self.f[..., 1] / self.size[..., 1]) ** 2

    def _distort_scale(self, r2):
        return 1 + self._k(0) * r2

    def _distort_scale_dr2(self, r2):
        return self._k(0).expand_as(r2)

    def _undistort_scale(self, r2):
        return 1 - self._k(0) * r2

    def _undistort_scale_dr2(self, r2):
        return (-self._k(0)).expand_as(r2)

    def J_distort(self, p2d, wrt: str = "pts"):
        if wrt == "scale2dist":
            return (p2d**2).sum(-1, keepdim=True)
        return super().J_distort(p2d, wrt)

    def J_undistort(self, p2d, wrt: str = "pts"):
        if wrt == "dist":
            return (-(p2d**2).sum(-1, keepdim=True) * p2d)[..., None]
        return super().J_undistort(p2d, wrt)

    def J_up_projection_offset(self, p2d, wrt: str = "uv"):
        if wrt == "uv":
            return 2 * self._k(0)[..., None] * _eye_like(p2d)
        if wrt == "dist":
            return (2 * p2d)[..., None]
        raise NotImplementedError(f"Jacobian not implemented for wrt={wrt}")


class Radial(BaseCamera):
    """s = 1 + k1 r2 + k2 r4; t = 1 - k1 r2 + (3 k1^2 - k2) r4."""

    @classmethod
    def name(cls) -> str:
        return "radial"

    @property
    def dist(self) -> torch.Tensor:
        return self._data[..., 6:8]

    @classmethod
    def num_dist_params(cls) -> int:
        return 2

    @property
    def k1(self) -> torch.Tensor:
        return self._data[..., 6]

    @property
    def k2(self) -> torch.Tensor:
        return self._data[..., 7]

    def _b(self):
        k1, k2 = self._k(0), self._k(1)
        return -k1, 3 * k1**2 - k2

    def _distort_scale(self, r2):
        return 1 + self._k(0) * r2 + self._k(1) * r2**2

    def _distort_scale_dr2(self, r2):
        return self._k(0) + 2 * self._k(1) * r2

    def _undistort_scale(self, r2):
        b1, b2 = self._b()
        return 1 + b1 * r2 + b2 * r2**2

    def _undistort_scale_dr2(self, r2):
        b1, b2 = self._b()
        return b1 + 2 * b2 * r2

    def J_distort(self, p2d, wrt: str = "pts"):
        if wrt == "scale2dist":
            r2 = (p2d**2).sum(-1, keepdim=True)
            return torch.cat([r2, r2**2], -1)
        return super().J_distort(p2d, wrt)

    def J_undistort(self, p2d, wrt: str = "pts"):
        if wrt == "dist":
            r2 = (p2d**2).sum(-1, keepdim=True)
            return torch.stack([(6 * r2**2 * self._k(0) - r2) * p2d, -(r2**2) * p2d], -1)
        return super().J_undistort(p2d, wrt)

    def J_up_projection_offset(self, p2d, wrt: str = "uv"):
        r2 = (p2d**2).sum(-1, keepdim=True)
        if wrt == "uv":
            return 8 * self._k(1)[..., None] * _outer(p2d, p2d) + \
                (2 * self._k(0) + 4 * self._k(1) * r2)[..., None] * _eye_like(p2d)
        if wrt == "dist":
            return torch.stack([2 * p2d, 4 * r2 * p2d], -1)
        raise NotImplementedError(f"Jacobian not implemented for wrt={wrt}")


class SimpleDivisional(_OneParam):
    """t = 1 / (1 + k1 r2); s = (1 - sqrt(1 - 4 k1 r2)) / (2 k1 r2)."""

    dist_range = (-3.0, 3.0)

    @classmethod
    def name(cls) -> str:
        return "simple_divisional"

    def _distort_scale(self, r2):
        k1 = self._k(0)
        num = 1 - torch.sqrt((1 - 4 * k1 * r2).clamp(min=0))
        den = 2 * k1 * r2
        return torch.where(den == 0, torch.ones_like(num), num / den.masked_fill(den == 0, 1e6))

    def _distort_scale_dr2(self, r2):
        k1 = self._k(0)
        t = torch.sqrt((1 - 4 * k1 * r2).clamp(min=1e-6))
        den = 2 * k1 * r2**2 * t
        return (2 * k1 * r2 - (1 - t) * t) / den.masked_fill(den == 0, 1e6)

    def _undistort_scale(self, r2):
        den = 1 + self._k(0) * r2
        return 1 / den.masked_fill(den == 0, 1e6)

    def _undistort_scale_dr2(self, r2):
        den = 1 + self._k(0) * r2
        den = den.masked_fill(den == 0, 1e6)
        return -self._k(0) / den**2

    def J_undistort(self, p2d, wrt: str = "pts"):
        if wrt == "dist":
            r2 = (p2d**2).sum(-1, keepdim=True)
            den = (1 + self._k(0) * r2) ** 2
            return (-r2 / den.masked_fill(den == 0, 1e6) * p2d)[..., None]
        return super().J_undistort(p2d, wrt)


camera_models = {
    "pinhole": Pinhole,
    "radial": Radial,
    "simple_radial": SimpleRadial,
    "simple_divisional": SimpleDivisional,
}
