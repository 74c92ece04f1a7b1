"""Metrics of a calibration and of perspective fields (reference: siclib/models/utils/metrics.py and the decoders' metrics,
siclib/models/decoders/up_decoder.py:111-128, latitude_decoder.py:116-133).

The seven functions of the reference keep their signatures, units (degrees; dist_error in the distortion's own unit) and
shapes.  `perspective_field_metrics` answers how well a set of fields agrees with a calibration: the decoders' metrics with
the target fields taken from a camera and a gravity, which is how the reference's datasets make their targets.

float32 inputs on one HIP device that do not require grad are scored by one HIP pass (gclm_field_errors: the target is
evaluated per pixel in registers and never written); anything else (CPU, float64, autograd) runs the reference's torch
composition on get_perspective_field, which stays the differentiable path.  The one deliberate difference: the HIP path takes
the up angle as atan2(|p x t|, p . t), which resolves small angles; the torch path in float32 takes acos of a cosine, whose
smallest non-zero value is 0.02 degrees, so it quantises every up error below about that.

`rank_calibrations` answers which of N candidate calibrations per image fits the fields best: the confidence-weighted
inlier sums the reference's RANSAC baseline ranks its hypotheses with (siclib/models/optimization/ransac.py:
check_up_inliers, check_latitude_inliers, get_best_index), on the same two paths (gclm_hypothesis_scores on the device).
"""
from typing import Dict, Optional, Sequence

import torch
from torch.nn import functional as F

from . import fields
from .camera import BaseCamera
from .gravity import Gravity
from .perspective_fields import get_perspective_field
from .utils import rad2deg


def pitch_error(pred_gravity: Gravity, target_gravity: Gravity) -> torch.Tensor:
    """Pitch error between two gravities, in degrees."""
    return rad2deg(torch.abs(pred_gravity.pitch - target_gravity.pitch))


def roll_error(pred_gravity: Gravity, target_gravity: Gravity) -> torch.Tensor:
    """Roll error between two gravities, in degrees."""
    return rad2deg(torch.abs(pred_gravity.roll - target_gravity.roll))


def gravity_error(pred_gravity: Gravity, target_gravity: Gravity) -> torch.Tensor:
    """Angle between two (B, 3) gravities, in degrees."""
    assert pred_gravity.vec3d.shape == target_gravity.vec3d.shape, f"{pred_gravity.vec3d.shape} != {target_gravity.vec3d.shape}"
    assert pred_gravity.vec3d.ndim == 2, f"{pred_gravity.vec3d.ndim} != 2"
    assert pred_gravity.vec3d.shape[1] == 3, f"{pred_gravity.vec3d.shape[1]} != 3"
    cossim = F.cosine_similarity(pred_gravity.vec3d, target_gravity.vec3d, dim=-1).clamp(-1, 1)
    return rad2deg(torch.acos(cossim))


def vfov_error(pred_cam: BaseCamera, target_cam: BaseCamera) -> torch.Tensor:
    """Vertical field of view error between two cameras, in degrees."""
    return rad2deg(torch.abs(pred_cam.vfov - target_cam.vfov))


def dist_error(pred_cam: BaseCamera, target_cam: BaseCamera) -> torch.Tensor:
    """Error of the first distortion parameter; zeros if a camera has none."""
    if hasattr(pred_cam, "dist") and hasattr(target_cam, "dist"):
        return torch.abs(pred_cam.dist[..., 0] - target_cam.dist[..., 0])
    return pred_cam.new_zeros(pred_cam.f.shape[0])


def latitude_error(predictions: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """Latitude error of (B, 1, H, W) fields in radians: (B, H, W) in degrees."""
    return rad2deg(torch.abs(predictions - targets)).squeeze(1)


def up_error(predictions: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """Angle between (B, 2, H, W) up fields: (B, H, W) in degrees."""
    assert predictions.shape == targets.shape, f"{predictions.shape} != {targets.shape}"
    assert predictions.ndim == 4, f"{predictions.ndim} != 4"
    assert predictions.shape[1] == 2, f"{predictions.shape[1]} != 2"
    angle = F.cosine_similarity(predictions, targets, dim=1).clamp(-1, 1)
    return rad2deg(torch.acos(angle))


_FIELDS = (("up", "up_field", "up_confidence", "up_angle", "up_error"),
           ("latitude", "latitude_field", "latitude_confidence", "latitude_angle", "latitude_error"))


def _on_hip(tensors) -> bool:
    """Whether these inputs take gclm_field_errors: all float32 on one HIP device, none requiring grad."""
    dev = tensors[0].device
    return all(t.is_cuda and t.dtype == torch.float32 and t.device == dev and not t.requires_grad for t in tensors)


def _field_metrics_torch(pred: Dict[str, torch.Tensor], camera: BaseCamera, gravity: Gravity, thresholds, return_errors: bool):
    """The reference's composition: the decoders' metrics against the fields of (camera, gravity)."""
    use_up, use_lat = "up_field" in pred, "latitude_field" in pred
    up_t, lat_t = get_perspective_field(camera, gravity, use_up=use_up, use_latitude=use_lat)
    out = {}
    for name, field, conf, key, err_key in _FIELDS:
        if field not in pred:
            continue
        if name == "up":
            error = up_error(pred[field], up_t) * (pred[field].sum(axis=1) != 0)
        else:
            error = latitude_error(pred[field], lat_t)
        out[f"{key}_error"] = error.mean(axis=(1, 2))
        if conf in pred:
            c = pred[conf].reshape(error.shape)
            out[f"{key}_error_weighted"] = (error * c).sum(axis=(1, 2)) / c.sum(axis=(1, 2))
        for th in thresholds:
            out[f"{key}_recall@{th}"] = (error < th).float().mean(axis=(1, 2))
        if return_errors:
            out[err_key] = error
    return out


def perspective_field_metrics(pred: Dict[str, torch.Tensor], camera: BaseCamera, gravity: Gravity,
                              recall_thresholds: Sequence[float] = (1, 3, 5, 10), return_errors: bool = False) -> Dict[str, torch.Tensor]:
    """How well the fields in `pred` agree with the calibration (camera, gravity), per image.

    `pred` is the dict LMOptimizer takes and returns: "up_field" (B, 2, H, W), "latitude_field" (B, 1, H, W) in radians, and
    optionally "up_confidence", "latitude_confidence" (B, H, W); at least one field.  `camera` (B) and `gravity` (B) define the
    target fields (get_perspective_field); the output of GeoCalib.calibrate, which carries the fields together with "camera"
    and "gravity", therefore scores directly.  Returns the decoders' keys, each (B,):
        up_angle_error, up_angle_error_weighted, up_angle_recall@{th}, latitude_angle_error, latitude_angle_error_weighted,
        latitude_angle_recall@{th}
    in degrees / as a share of all pixels.  A field's keys are present only when the field is in `pred`, a weighted key only
    when that confidence is.  The up error of a pixel with p_x + p_y == 0 is zero (the reference's mask, as written); the means
    run over all pixels.  `return_errors` adds "up_error" and "latitude_error", the per-pixel errors (B, H, W).

    float32 HIP tensors without grad take one HIP pass; anything else the torch composition (module docstring: the HIP path
    resolves small up angles, the float32 torch path quantises them at about 0.02 degrees)."""
    if "up_field" not in pred and "latitude_field" not in pred:
        raise ValueError("`pred` holds neither up_field nor latitude_field")
    thresholds = list(recall_thresholds)
    if len(camera.shape) == 0:
        camera, gravity = camera.unsqueeze(0), gravity.unsqueeze(0)
    given = [pred[k] for _, f, c, _, _ in _FIELDS for k in (f, c) if k in pred]
    cam, grav = camera._data, gravity._data
    if not (_on_hip(given + [cam, grav]) and cam.dim() == grav.dim() == 2 and cam.shape[0] == grav.shape[0]
            and len(thresholds) <= 8):
        return _field_metrics_torch(pred, camera, gravity, thresholds, return_errors)
    stats, up_err, lat_err = fields.field_errors(
        camera.name(), cam, grav, pred.get("up_field"), pred.get("latitude_field"), pred.get("up_confidence"),
        pred.get("latitude_confidence"), thresholds, return_errors)
    per = 2 + len(thresholds)
    out = {}
    for i, (_, field, conf, key, err_key) in enumerate(_FIELDS):
        if field not in pred:
            continue
        out[f"{key}_error"] = stats[:, i * per]
        if conf in pred:
            out[f"{key}_error_weighted"] = stats[:, i * per + 1]
        for j, th in enumerate(thresholds):
            out[f"{key}_recall@{th}"] = stats[:, i * per + 2 + j]
        if return_errors:
            out[err_key] = up_err if i == 0 else lat_err
    return out


_RANK_CHUNK_PIXELS = 1 << 22       # pixels x hypotheses x images of one chunk of the torch composition (a dozen such planes live)


def _rank_torch(pred, cameras, cam, grav, thresholds, mask):
    """The torch composition: up / latitude inlier sums (B, N) of the hypotheses `cam` (B, N, 8), `grav` (B, N, 3), the fields
    of get_perspective_field scored by up_error / latitude_error, in chunks of hypotheses."""
    B, N = cam.shape[:2]
    out = []
    for name, field, conf, _, _ in _FIELDS:
        if field not in pred:
            out.append(cam.new_zeros((B, N)))
            continue
        p = pred[field]
        H, W = p.shape[-2:]
        weight = pred[conf].reshape(B, H, W) if conf in pred else p.new_ones((B, H, W))
        if mask is not None:
            weight = weight * mask.reshape(B, H, W)
        step, parts = max(1, _RANK_CHUNK_PIXELS // (B * H * W)), []
        for n0 in range(0, N, step):
            k = min(step, N - n0)
            camera = type(cameras)(cam[:, n0:n0 + k].reshape(B * k, 8))
            gravity = Gravity(grav[:, n0:n0 + k].reshape(B * k, 3))
            gravity._data = grav[:, n0:n0 + k].reshape(B * k, 3)               # as stored
            up_t, lat_t = get_perspective_field(camera, gravity, use_up=name == "up", use_latitude=name != "up")
            rep = p[:, None].expand(B, k, *p.shape[1:]).reshape(B * k, *p.shape[1:])
            if name == "up":
                error = up_error(rep, up_t.to(rep.dtype)) * (rep.sum(axis=1) != 0)
            else:
                error = latitude_error(rep, lat_t.to(rep.dtype))
            hit = (error < thresholds[name]).to(weight.dtype).reshape(B, k, H, W)
            parts.append((hit * weight[:, None]).sum(axis=(2, 3)))
        out.append(torch.cat(parts, 1))
    return out


def rank_calibrations(pred: Dict[str, torch.Tensor], cameras: BaseCamera, gravities: Gravity, up_threshold: float = 1.0,
                      latitude_threshold: float = 1.0, up_weight: float = 1.0, latitude_weight: float = 1.0,
                      mask: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """Which of N candidate calibrations per image fits the fields in `pred` best.

    `pred` is the dict perspective_field_metrics takes (B images).  `cameras` / `gravities` hold N hypotheses per image: of
    batch shape (B, N), or flat (B N) in the reference's order (hypothesis n of image b at b N + n), N = len // B.  A
    hypothesis' score is the reference's RANSAC score (ransac.py): per field the sum of confidence x mask over the pixels
    whose error -- up_error times the decoders' mask, latitude_error, against the hypothesis' perspective field -- lies
    strictly below the field's threshold in degrees, and
        scores = up_weight up_scores + latitude_weight latitude_scores.
    A missing confidence counts as 1, `mask` (B, H, W) multiplies both fields' contributions (the reference's inliers), a
    missing field scores 0.  The defaults are RPFSolver.default_conf's.  Returns
        scores, up_scores, latitude_scores (B, N);  best (B,) int64: the first index of the largest score per image;
        camera, gravity: the winning hypotheses (batch B), gravity as stored.
    A hypothesis with a NaN parameter scores 0; a NaN confidence makes that field's scores of that image NaN, and NaN counts
    as the maximum (torch.argmax).

    float32 HIP tensors without grad take one HIP pass (each plane read once per fields.HYPOTHESIS_CHUNK hypotheses);
    anything else the torch composition on get_perspective_field, in chunks of hypotheses.  Not differentiable in the
    hypotheses either way: a hit is a comparison."""
    if "up_field" not in pred and "latitude_field" not in pred:
        raise ValueError("`pred` holds neither up_field nor latitude_field")
    B = (pred["up_field"] if "up_field" in pred else pred["latitude_field"]).shape[0]
    cam, grav = cameras._data, gravities._data
    if B < 1 or cam.shape[:-1] != grav.shape[:-1] or cam.dim() not in (2, 3) or cam.shape[:-1].numel() % B or \
            (cam.dim() == 3 and cam.shape[0] != B):
        raise ValueError(f"cameras {tuple(cam.shape[:-1])} and gravities {tuple(grav.shape[:-1])} must both be (B, N) or (B N,) "
                         f"hypotheses of {B} images")
    N = cam.shape[:-1].numel() // B
    cam, grav = cam.reshape(B, N, 8), grav.reshape(B, N, 3)
    given = [pred[k] for _, f, c, _, _ in _FIELDS for k in (f, c) if k in pred] + ([] if mask is None else [mask])
    if _on_hip(given + [cam, grav]) and 1 <= N <= 65535:
        scores, best = fields.hypothesis_scores(
            cameras.name(), cam, grav, pred.get("up_field"), pred.get("latitude_field"), pred.get("up_confidence"),
            pred.get("latitude_confidence"), mask, up_threshold, latitude_threshold, up_weight, latitude_weight)
        up_s, lat_s, total, best = scores[..., 0], scores[..., 1], scores[..., 2], best.long()
    else:
        with torch.no_grad():
            up_s, lat_s = _rank_torch(pred, cameras, cam, grav, {"up": up_threshold, "latitude": latitude_threshold}, mask)
            total = up_weight * up_s + latitude_weight * lat_s
            best = torch.argmax(total, dim=1)
    rows = torch.arange(B, device=cam.device)
    gravity = Gravity(grav[rows, best])
    gravity._data = grav[rows, best]              # as stored: the constructor renormalises
    return {"scores": total, "up_scores": up_s, "latitude_scores": lat_s, "best": best, "camera": type(cameras)(cam[rows, best]),
            "gravity": gravity}
