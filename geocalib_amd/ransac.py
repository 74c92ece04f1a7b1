"""A robust estimator beside the LM: the reference's RANSAC baseline (siclib/models/optimization/ransac.py: MinimalSolver,
RPFSolver) -- roll, pitch and focal length of a pinhole camera from three pixels of the perspective fields, N samples per
image, the best of them by the reference's inlier score.

`solve_rpf` is the minimal solver.  Its definition is stated in full at gclm_rpf_hypotheses in include/gclm.h; DESIGN.md 3.11
says where it leaves the reference and why (the reference divides the vanishing point by V_z and so loses the sign of the
gravity for every camera that looks down, swaps the principal point's coordinates, and keeps the root that squaring the
latitude equation introduces).  In short, per sample of three pixels (x_k, y_k), principal point (W / 2, H / 2):
    V = l_0 x l_1 of the two up lines, homogeneous;  v = (V_x - c_x V_z, V_y - c_y V_z, V_z) / |.|
    a0 F^2 + a1 F + a2 = 0 in F = f^2 from sin(latitude) at pixel 2, solved without cancellation: two roots (one, F =
    prior_focal^2, with a prior focal length)
    g = normalize(v_x / f, v_y / f, v_z), its sign from the up direction at pixel 0
    valid iff f, g finite, f inside the LM's focal clamp and the unsquared latitude equation holds in sign;  invalid rows are NaN.
float32 HIP tensors without grad take one HIP launch (gclm_rpf_hypotheses, one lane per sample); anything else (CPU,
float64) the torch composition of the same operations in the same order, `_solve_torch`.

`RPFSolver` keeps the reference's conf keys and output dict: solve_rpf -> metrics.rank_calibrations -> the winner per image.
Inference only: no loss(), no gradients."""
import math
from types import SimpleNamespace
from typing import Any, Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _call, _lib, fields, metrics
from .camera import Pinhole
from .lm_optimizer import _unit_gravity, get_trivial_estimation

_MASK64 = (1 << 64) - 1
# the LM's focal clamp (csrc/gclm_device.h): H / 2 / tan(75 deg) and H / 2 / tan(2.5 deg) as the float32 constants it divides by
_TAN_MAX, _TAN_MIN = 3.7320504, 0.043660942


def focal_range(H: int):
    """(f_min, f_max) of a valid row, as float32 values: the kernel's H * 0.5f / 3.7320504f and H * 0.5f / 0.043660942f."""
    h = np.float32(H) * np.float32(0.5)
    return float(h / np.float32(_TAN_MAX)), float(h / np.float32(_TAN_MIN))


def _mix64(z: np.ndarray) -> np.ndarray:
    """The splitmix64 finaliser on uint64 arrays (arithmetic modulo 2^64)."""
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draw_samples(seed: int, first_index: int, B: int, N: int, H: int, W: int) -> torch.Tensor:
    """The pixels gclm_rpf_hypotheses draws when it is given none (include/gclm.h): (B, N, 3, 2) int32 = (x, y), a function
    of (seed, first_index + b, n, k), W and H alone."""
    with np.errstate(over="ignore"):
        i = (np.arange(B, dtype=np.uint64) + np.uint64(first_index & _MASK64))
        base = _mix64(np.uint64((seed ^ _lib.RPF_DRAW_SALT) & _MASK64) ^ _mix64(i * np.uint64(0xD1342543DE82EF95) + np.uint64(1)))
        n = np.arange(N, dtype=np.uint64)[None, :, None] * np.uint64(4) + np.arange(3, dtype=np.uint64)[None, None, :]
        h = _mix64(base[:, None, None] + n)
        x = ((h >> np.uint64(32)) * np.uint64(W)) >> np.uint64(32)
        y = ((h & np.uint64(0xFFFFFFFF)) * np.uint64(H)) >> np.uint64(32)
    return torch.from_numpy(np.stack([x, y], -1).astype(np.int32))


def _solve_torch(up: torch.Tensor, lat: Optional[torch.Tensor], prior: Optional[torch.Tensor], samples: torch.Tensor):
    """The torch composition of the definition, in the dtype of `up`, operation by operation in the kernel's order:
    (cam (B, N Rn, 8), grav (B, N Rn, 3)), invalid rows NaN."""
    B, _, H, W = up.shape
    N, dt = samples.shape[1], up.dtype
    s = samples.long()
    x, y = s[..., 0], s[..., 1]                                    # (B, N, 3)
    rows = torch.arange(B, device=up.device)[:, None]
    flat = up.reshape(B, 2, H * W)
    o0, o1, o2 = (y[..., k] * W + x[..., k] for k in range(3))
    d0x, d0y, d1x, d1y = flat[rows, 0, o0], flat[rows, 1, o0], flat[rows, 0, o1], flat[rows, 1, o1]
    cx, cy = 0.5 * W, 0.5 * H
    x0, y0, x1, y1 = x[..., 0].to(dt), y[..., 0].to(dt), x[..., 1].to(dt), y[..., 1].to(dt)
    l0x, l0y, l0z = -d0y, d0x, x0 * d0y - y0 * d0x
    l1x, l1y, l1z = -d1y, d1x, x1 * d1y - y1 * d1x
    Vx, Vy, Vz = l0y * l1z - l0z * l1y, l0z * l1x - l0x * l1z, l0x * l1y - l0y * l1x
    vx, vy, vz = Vx - cx * Vz, Vy - cy * Vz, Vz
    vn = torch.sqrt(vx * vx + vy * vy + vz * vz)
    vx, vy, vz = vx / vn, vy / vn, vz / vn
    U, Vp, U0, V0 = x[..., 2].to(dt) - cx, y[..., 2].to(dt) - cy, x0 - cx, y0 - cy
    if prior is not None:
        p = prior.to(dt).reshape(B, 1).expand(B, N)
        roots, L = [p * p], None
    else:
        L = torch.sin(lat.reshape(B, H * W)[rows, o2])
        L2, R, S, D, vz2 = L * L, U * U + Vp * Vp, vx * vx + vy * vy, vx * U + vy * Vp, vz * vz
        a0 = (L2 - 1) * vz2
        a1 = L2 * (R * vz2 + S) - 2 * D * vz
        a2 = L2 * R * S - D * D
        root = torch.sqrt(a1 * a1 - 4 * a0 * a2)
        q = -(a1 + torch.where(a1 >= 0, root, -root)) / 2
        roots = [a2 / q, q / a0]
    fmin, fmax = focal_range(H)
    cams, gravs = [], []
    for F in roots:
        f = torch.sqrt(F)
        gx, gy, gz = vx / f, vy / f, vz
        n = torch.sqrt(gx * gx + gy * gy + gz * gz)
        gx, gy, gz = gx / n, gy / n, gz / n
        dot = (gx - gz * (U0 / f)) * d0x + (gy - gz * (V0 / f)) * d0y
        sign = torch.where(dot < 0, -torch.ones_like(dot), torch.ones_like(dot))
        gx, gy, gz = gx * sign, gy * sign, gz * sign
        valid = (f >= fmin) & (f <= fmax) & (gx.abs() + gy.abs() + gz.abs() <= 2)
        if L is not None:
            valid = valid & (L * (gx * (U / f) + gy * (Vp / f) + gz) >= 0)
        one, nan = torch.ones_like(f), torch.full_like(f, math.nan)
        cam = torch.stack([one * W, one * H, f, f, one * cx, one * cy, one * 0, one * 0], -1)
        cams.append(torch.where(valid[..., None], cam, nan[..., None]))
        gravs.append(torch.where(valid[..., None], torch.stack([gx, gy, gz], -1), nan[..., None]))
    Rn = len(roots)
    return torch.stack(cams, 2).reshape(B, N * Rn, 8), torch.stack(gravs, 2).reshape(B, N * Rn, 3)


def _check_samples(samples: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
    if samples.dim() != 4 or samples.shape[0] != B or samples.shape[2:] != (3, 2) or samples.shape[1] < 1 or \
            samples.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"`samples` {tuple(samples.shape)} {samples.dtype} must be (B = {B}, N >= 1, 3, 2) integer pixels (x, y)")
    lim = samples.new_tensor([W, H])
    if bool(((samples < 0) | (samples >= lim)).any()):
        raise ValueError(f"`samples` holds a pixel outside the {W} x {H} image")
    return samples.to(torch.int32).contiguous()


def solve_rpf(pred: Dict[str, torch.Tensor], samples: Optional[torch.Tensor] = None, prior_focal: Optional[torch.Tensor] = None,
              n: int = 1000, seed: int = 0, first_index: int = 0) -> Dict[str, Any]:
    """The minimal solver over N samples of three pixels per image (module docstring; include/gclm.h: gclm_rpf_hypotheses).

    `pred`: "up_field" (B, 2, H, W) and "latitude_field" (B, 1, H, W) in radians; the latitude may be absent with a
    `prior_focal` (B,), which fixes f.  `samples` (B, N, 3, 2) integer pixels (x, y) -- pixels 0 and 1 give the up vectors,
    pixel 2 the latitude; a pixel outside the image raises ValueError (the check reads the samples back: one host
    synchronisation where they live on a device; the C entry cannot look and leaves invalid rows) -- or None: `n` samples per image are drawn from
    (seed, first_index + b, sample, pixel) by the rule of include/gclm.h, the same on both paths.  Returns
        cameras:   Pinhole of batch shape (B, N Rn), Rn = 2 roots per sample, 1 with a prior focal; sample n, root r at n Rn + r
        gravities: Gravity of the same shape, stored as written (not renormalised)
        valid:     (B, N Rn) bool; an invalid row is NaN throughout and scores 0 in metrics.rank_calibrations
        samples:   (B, N, 3, 2) int32, the pixels used."""
    return _solve(pred, samples, prior_focal, n, seed, first_index, check=True)


def _solve(pred, samples, prior_focal, n, seed, first_index, check):
    """solve_rpf; `check` = False takes samples that are inside the image by construction (RPFSolver's own) as they are."""
    up = pred["up_field"]
    if up.dim() != 4 or up.shape[1] != 2:
        raise ValueError(f"`up_field` {tuple(up.shape)} must be (B, 2, H, W)")
    B, _, H, W = up.shape
    lat = pred.get("latitude_field")
    if lat is None and prior_focal is None:
        raise ValueError("without a `latitude_field` the focal length needs a `prior_focal`")
    if lat is not None and (lat.numel() != B * H * W or lat.shape[-2:] != (H, W)):
        raise ValueError(f"`latitude_field` {tuple(lat.shape)} does not fit {B} images of {H} x {W}")
    if prior_focal is not None:
        prior_focal = torch.as_tensor(prior_focal, device=up.device).detach().to(up.dtype).reshape(-1)
        if prior_focal.numel() != B:
            raise ValueError(f"`prior_focal` {tuple(prior_focal.shape)} must hold one value per image ({B})")
    if samples is not None:
        samples = (_check_samples(samples, B, H, W) if check else samples.to(torch.int32).contiguous()).to(up.device)
    elif int(n) < 1:
        raise ValueError(f"n = {n}: at least one sample per image")
    given = [up] + [t for t in (lat, prior_focal) if t is not None]
    if metrics._on_hip(given):
        cam, grav, samples = fields.rpf_hypotheses(up, None if prior_focal is not None else lat, prior_focal, samples, int(n),
                                                   int(seed), int(first_index))
    else:
        if samples is None:
            samples = draw_samples(int(seed), int(first_index), B, int(n), H, W).to(up.device)
        with torch.no_grad():
            cam, grav = _solve_torch(up.detach(), None if lat is None else lat.detach().to(up.dtype), prior_focal, samples)
    return {"cameras": Pinhole(cam), "gravities": _unit_gravity(grav), "valid": ~cam[..., 2].isnan(), "samples": samples}


class RPFSolver(nn.Module):
    """RANSAC over the minimal solver (reference: siclib/models/optimization/ransac.py, RPFSolver): `n_iter` samples per
    image, every root scored by metrics.rank_calibrations -- per field the confidence-weighted count of the pixels whose
    error against the candidate's perspective field lies below `*_inlier_th` degrees --, the best one returned."""

    default_conf = {
        "n_iter": 1000,
        "up_inlier_th": 1,
        "latitude_inlier_th": 1,
        "error_fn": "angle",  # the reference's "mse" is not provided
        "up_weight": 1,
        "latitude_weight": 1,
        "loss_weight": 1,
        "use_latitude": True,
        # extension: the samples are a function of (seed, image index, sample, pixel) -- two calls agree
        "seed": 0,
    }

    def __init__(self, conf: Dict[str, Any] = None):
        super().__init__()
        conf = dict(conf or {})
        unknown = set(conf) - set(self.default_conf)
        if unknown:
            raise ValueError(f"unknown RPFSolver conf keys: {sorted(unknown)}")
        self.conf = conf = SimpleNamespace(**{**self.default_conf, **conf})
        if conf.error_fn != "angle":
            raise NotImplementedError(f"error_fn = {conf.error_fn!r}: only \"angle\" is provided")
        if int(conf.n_iter) < 1 or 2 * int(conf.n_iter) > _call.MAX_CALL:
            raise ValueError(f"n_iter = {conf.n_iter} must lie in 1..{_call.MAX_CALL // 2} (two roots per sample are ranked in one call)")

    def _masked_samples(self, inliers: torch.Tensor, W: int) -> torch.Tensor:
        """(B, n_iter, 3, 2) pixels drawn with replacement among the pixels of `inliers` (B, H, W) that equal 1 (the reference's
        np.random.choice), in one multinomial; an image without any draws from the whole image (and scores 0 everywhere)."""
        B = inliers.shape[0]
        w = (inliers.reshape(B, -1) == 1).to(torch.float32)
        w = torch.where(w.sum(1, keepdim=True) > 0, w, torch.ones_like(w))
        gen = torch.Generator(device=w.device)
        gen.manual_seed(int(self.conf.seed))
        idx = torch.multinomial(w, 3 * int(self.conf.n_iter), replacement=True, generator=gen).reshape(B, -1, 3)
        return torch.stack([idx % W, idx // W], -1).to(torch.int32)

    def forward(self, data: Dict[str, torch.Tensor]) -> Dict[str, Any]:
        """`data`: "up_field", "latitude_field", optional "up_confidence", "latitude_confidence", "inliers" (B, H, W),
        "prior_focal" (B,).  Returns camera_opt (Pinhole, B), gravity_opt (Gravity, B), up_inliers and latitude_inliers
        (B, H, W): (error < th) x confidence of the winner, score (B,) and n_valid (B,): the valid rows of each image.  An
        image without a valid row, or without a pixel in `inliers`, gets get_trivial_estimation's estimate and score 0."""
        c = self.conf
        keys = ["up_field", "up_confidence"] + (["latitude_field", "latitude_confidence"] if c.use_latitude else [])
        pred = {k: data[k] for k in keys if k in data}
        up = pred["up_field"]
        B, _, H, W = up.shape
        prior = data.get("prior_focal")
        if "latitude_field" not in pred and prior is None:
            raise ValueError("use_latitude = False (or no `latitude_field`) leaves the focal length to a `prior_focal`")
        with torch.no_grad():
            inliers = data.get("inliers")
            samples = None if inliers is None else self._masked_samples(inliers, W)
            hyp = _solve(pred, samples, prior, int(c.n_iter), int(c.seed), 0, check=False)
            mask = None if inliers is None else inliers.reshape(B, H, W).to(up.dtype)
            # The rows are ranked with their image size written into the invalid ones too: the torch composition of the ranking
            # -- taken for CPU, float64 and grad-requiring tensors, whatever the solve took -- reads the size from the first
            # camera row of a chunk, and the HIP ranking reads neither number.  f stays NaN: such a row still scores 0.
            sized = hyp["cameras"]._data.clone()
            sized[..., 0], sized[..., 1] = W, H
            rank = metrics.rank_calibrations(pred, Pinhole(sized), hyp["gravities"], float(c.up_inlier_th), float(c.latitude_inlier_th),
                                             float(c.up_weight), float(c.latitude_weight), mask=mask)
            rows = torch.arange(B, device=up.device)
            fallback = ~hyp["valid"][rows, rank["best"]]
            if mask is not None:
                fallback = fallback | (mask.reshape(B, -1) == 1).sum(1).eq(0)
            first = {"latitude_field": up, **{k: v for k, v in data.items() if k in ("up_field", "latitude_field", "prior_focal")}}
            cam0, grav0 = get_trivial_estimation(first, Pinhole)
            cam = torch.where(fallback[:, None], cam0._data.to(up.dtype), rank["camera"]._data)
            grav = torch.where(fallback[:, None], grav0._data.to(up.dtype), rank["gravity"]._data)
            score = torch.where(fallback, torch.zeros_like(rank["scores"][:, 0]), rank["scores"][rows, rank["best"]])
            camera, gravity = Pinhole(cam), _unit_gravity(grav)
            errors = metrics.perspective_field_metrics(pred, camera, gravity, (1.0,), return_errors=True)
            conf_of = lambda k: pred[k].reshape(B, H, W) if k in pred else 1  # noqa: E731
            up_in = (errors["up_error"] < float(c.up_inlier_th)) * conf_of("up_confidence")
            if "latitude_field" in pred:
                lat_in = (errors["latitude_error"] < float(c.latitude_inlier_th)) * conf_of("latitude_confidence")
            else:
                lat_in = up.new_zeros((B, H, W))
        return {"camera_opt": camera, "gravity_opt": gravity, "up_inliers": up_in.to(up.dtype), "latitude_inliers": lat_in.to(up.dtype),
                "score": score, "n_valid": hyp["valid"].sum(1)}

    def metrics(self, pred: Dict[str, Any], data: Dict[str, Any]) -> Dict[str, torch.Tensor]:
        return {"roll_opt_error": metrics.roll_error(pred["gravity_opt"], data["gravity"]),
                "pitch_opt_error": metrics.pitch_error(pred["gravity_opt"], data["gravity"]),
                "vfov_opt_error": metrics.vfov_error(pred["camera_opt"], data["camera"])}
