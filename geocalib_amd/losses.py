"""The losses the up and latitude heads are trained with (reference: UpDecoder.calculate_losses, LatitudeDecoder.calculate_losses
and PerspectiveDecoder.loss, siclib/models/decoders/up_decoder.py:51-109, latitude_decoder.py:53-114, perspective_decoder.py:41-59).

`field_loss` is the reference's calculate_losses for explicit target tensors, as a torch composition: differentiable in
everything torch can differentiate, on any device and dtype.

`perspective_field_loss` takes the targets from a camera and a gravity, which is how the reference's datasets make them.
float32 fields on one HIP device, with a camera and a gravity that do not require grad, take the HIP path: one pass
evaluates the target per pixel in registers and reduces the loss per image (gclm_field_loss), and when a field requires
grad a torch.autograd.Function hands autograd the gradient of a second such pass (gclm_field_loss_grad) -- no target field
is rendered, nothing but the inputs is kept for backward.  That path is differentiable with respect to the predicted fields
only, once; the confidences are detached, as in the reference.  Anything else (CPU, float64, half-precision predictions, a
camera or gravity that requires grad) renders the target with get_perspective_field and runs `field_loss`.
`calibration_grad=True` keeps a float32 HIP camera or gravity that requires grad on the HIP path: backward then also returns
the gradients to `camera._data` (B, 8) and `gravity._data` (B, 3), from one pass that evaluates the target again and pulls
its cotangent back to the calibration (gclm_field_loss_param_grad), once differentiable.  Off by default: every default
route is as it was.

The two paths differ where arithmetic leaves no choice: the l1 gradient of a NaN residual is NaN on the HIP path and 0 in
torch (torch's sgn), and the HIP path takes the cauchy loss as log1p, which keeps small residuals the float32 log(1 + x)
rounds away.

`bin_loss` and `perspective_bin_loss` are the same pair for CLASSIFICATION heads (the heads fields.pack_fields_from_logits
decodes): per-pixel cross-entropy of the logits against the bins of a calibration's fields.  The reference trains no such head
(up_decoder.py:99, latitude_decoder.py:104 raise); the definition is the composition get_perspective_field + the encoders of
perspective_encoding + F.cross_entropy with the weighting of `field_loss`.  float32, float16 or bfloat16 logits on a HIP
device take gclm_bin_loss / gclm_bin_loss_grad: the logits are read once each way and nothing of their size is written but
the gradient."""
import math
from typing import Dict, Optional, Sequence

import torch
from torch.autograd.function import once_differentiable

from . import _lib, fields, metrics
from .camera import BaseCamera
from .gravity import Gravity
from .perspective_fields import get_perspective_field

LOSS_TYPES = ("l1", "l2", "dot", "cauchy", "huber")
CAUCHY_C = 0.007                    # the reference's scale: "corresponds to about 5 degrees"
HUBER_DELTA = math.pi / 180         # deg2rad(1)


def _check_loss_type(loss_type: str, field: str) -> None:
    if loss_type not in LOSS_TYPES or (loss_type == "dot" and field != "up"):
        raise ValueError(f"unknown {field} loss type {loss_type!r}: one of {LOSS_TYPES} ('dot' for the up field only)")


def field_loss(predictions: torch.Tensor, targets: torch.Tensor, confidence: Optional[torch.Tensor] = None, loss_type: str = "l1",
               use_uncertainty_loss: bool = True) -> torch.Tensor:
    """The reference's calculate_losses without its weight: predictions and targets (B, C, H, W) (up: C = 2, latitude: C = 1),
    an optional confidence (B, H, W); returns (B,).  Per pixel, with r = predictions - targets: l1 sum |r|, l2 sum r^2,
    dot 1 - sum r t, cauchy c^2 / 2 log(1 + sum r^2 / c^2) with c = 0.007, huber nn.HuberLoss(delta=deg2rad(1)) summed over
    C.  With a confidence and `use_uncertainty_loss` the pixel is weighted by conf / sum conf * H W, detached; then the mean.
    Half-precision predictions are cast to float32 as the reference casts them (its predictions.float()); float64 stays
    float64, which the reference's cast would round."""
    if loss_type not in LOSS_TYPES:
        raise ValueError(f"unknown loss type {loss_type!r}: one of {LOSS_TYPES}")
    predictions = predictions.float() if predictions.dtype in (torch.float16, torch.bfloat16) else predictions
    residuals = predictions - targets
    if loss_type == "l2":
        loss = (residuals ** 2).sum(axis=1)
    elif loss_type == "l1":
        loss = residuals.abs().sum(axis=1)
    elif loss_type == "dot":
        loss = 1 - (residuals * targets).sum(axis=1)
    elif loss_type == "cauchy":
        c = CAUCHY_C
        loss = c ** 2 / 2 * torch.log(1 + (residuals ** 2).sum(axis=1) / c ** 2)
    else:
        loss = torch.nn.HuberLoss(reduction="none", delta=HUBER_DELTA)(predictions, targets.expand_as(predictions)).sum(axis=1)
    if confidence is not None and use_uncertainty_loss:
        confidence = confidence.reshape(loss.shape)
        weight = confidence / confidence.sum(axis=(-2, -1), keepdims=True)
        loss = loss * (weight * (weight.size(-1) * weight.size(-2))).detach()
    return loss.mean(axis=(1, 2))


class _FieldLossFunction(torch.autograd.Function):
    """(up, lat) -> (B, 2) weighted losses [up, latitude] on the HIP path; a missing field is None and its column NaN."""

    @staticmethod
    def forward(ctx, up, lat, model, cam, grav, up_conf, lat_conf, up_loss, lat_loss, up_weight, lat_weight):
        out = fields.field_loss(model, cam, grav, up, lat, up_conf, lat_conf, up_loss, lat_loss)
        ctx.save_for_backward(*(t for t in (up, lat, up_conf, lat_conf) if t is not None), cam, grav, out[:, 2:])
        ctx.given = [t is not None for t in (up, lat, up_conf, lat_conf)]
        ctx.call = (model, up_loss, lat_loss, up_weight, lat_weight)
        # (the weights stay host floats: a tensor of them would be a blocking copy to the device in every step)
        return torch.stack([out[:, 0] * up_weight, out[:, 1] * lat_weight], 1)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        saved = list(ctx.saved_tensors)
        up, lat, up_conf, lat_conf = (saved.pop(0) if g else None for g in ctx.given)
        cam, grav, den = saved
        model, up_loss, lat_loss, up_weight, lat_weight = ctx.call
        want_up, want_lat, want_cam, want_grav = (ctx.needs_input_grad[i] for i in (0, 1, 3, 4))
        # grad_output x weight / denominator, on the device; an absent field's column is never read
        scale = grad_out.to(torch.float32) / den
        scale[:, 0] *= up_weight
        scale[:, 1] *= lat_weight
        g_up = g_lat = g_cam = g_grav = None
        f_up, f_upc = (up, up_conf) if want_up else (None, None)      # a field that asks for no gradient is left out of the pass
        f_lat, f_latc = (lat, lat_conf) if want_lat else (None, None)
        if f_up is not None or f_lat is not None:
            g_up, g_lat = fields.field_loss_grad(model, cam, grav, scale, f_up, f_lat, f_upc, f_latc, up_loss, lat_loss)
        if want_cam or want_grav:                    # (calibration_grad: the same targets' cotangent pulled back to the calibration)
            g_cam, g_grav = fields.field_loss_param_grad(model, cam, grav, scale, up, lat, up_conf, lat_conf, up_loss, lat_loss,
                                                         want_cam=want_cam, want_grav=want_grav)
        return (g_up, g_lat, None, g_cam, g_grav) + (None,) * 6


def _hip_path(tensors, cam: torch.Tensor, grav: torch.Tensor) -> bool:
    """Whether these inputs take gclm_field_loss: all float32 on one HIP device, matching batches, camera and gravity without
    grad (the fields may require it; `calibration_grad` asks with the detached camera and gravity)."""
    dev = cam.device
    return (all(t.is_cuda and t.dtype == torch.float32 and t.device == dev for t in list(tensors) + [cam, grav])
            and not (cam.requires_grad or grav.requires_grad) and cam.dim() == grav.dim() == 2 and cam.shape[0] == grav.shape[0]
            and all(t.shape[0] == cam.shape[0] for t in tensors))


def _field_loss_torch(pred, camera, gravity, types, use_uncertainty_loss):
    """The torch composition: {field: (B,) unweighted loss} against the fields of get_perspective_field."""
    up_t, lat_t = get_perspective_field(camera, gravity, use_up="up_field" in pred, use_latitude="latitude_field" in pred)
    out = {}
    for name, target in (("up", up_t), ("latitude", lat_t)):
        if f"{name}_field" in pred:
            out[name] = field_loss(pred[f"{name}_field"], target, pred.get(f"{name}_confidence"), types[name], use_uncertainty_loss)
    return out


def perspective_field_loss(pred: Dict[str, torch.Tensor], camera: BaseCamera, gravity: Gravity, up_loss: str = "l1",
                           latitude_loss: str = "l1", use_uncertainty_loss: bool = True, up_loss_weight: float = 1.0,
                           latitude_loss_weight: float = 1.0, calibration_grad: bool = False) -> Dict[str, torch.Tensor]:
    """The decoders' losses of the fields in `pred` against the calibration (camera, gravity), per image.

    `pred` is the dict LMOptimizer and metrics.perspective_field_metrics take: "up_field" (B, 2, H, W), "latitude_field"
    (B, 1, H, W) in radians, optionally "up_confidence", "latitude_confidence" (B, H, W) or (B, 1, H, W); at least one field.
    Returns the reference's keys, each (B,): "up-{type}-loss" and "up_total", "latitude-{type}-loss" and "latitude_total" --
    a field's keys only when the field is in `pred` -- and "perspective_total", their sum.  The weights multiply the losses,
    as the decoders' loss_weight.  A confidence weights its field's pixels by conf / sum conf (detached) when
    `use_uncertainty_loss`; sum conf = 0 gives NaN.

    float32 HIP fields with a camera and gravity that do not require grad take the HIP path (module docstring), also when a
    field requires grad; anything else the torch composition.  `calibration_grad=True` keeps float32 HIP inputs on the HIP path
    also when `camera._data` or `gravity._data` require grad: the forward is the same pass, bit for bit, and backward hands
    autograd their gradients from one more pass (gclm_field_loss_param_grad) -- the loss of an optimised calibration, e.g. the
    differentiable LMOptimizer's out["camera"], out["gravity"], stays on the HIP path.  Raises ValueError for an unknown loss
    type and for 'dot' on the latitude, on both paths."""
    if "up_field" not in pred and "latitude_field" not in pred:
        raise ValueError("`pred` holds neither up_field nor latitude_field")
    types = {"up": up_loss, "latitude": latitude_loss}
    for name, t in types.items():
        _check_loss_type(t, name)
    if len(camera.shape) == 0:
        camera, gravity = camera.unsqueeze(0), gravity.unsqueeze(0)
    pred = dict(pred)
    for name in ("up", "latitude"):
        conf = pred.get(f"{name}_confidence")
        if f"{name}_field" not in pred:
            pred.pop(f"{name}_confidence", None)
        elif conf is not None and conf.dim() == 4:
            pred[f"{name}_confidence"] = conf.reshape(conf.shape[0], *conf.shape[-2:])
    given = [pred[k] for f in ("up", "latitude") for k in (f"{f}_field", f"{f}_confidence") if k in pred]
    cam, grav = camera._data, gravity._data
    # (calibration_grad: the question is put for the detached calibration, so that one that requires grad stays on the HIP path)
    if _hip_path(given, *((cam.detach(), grav.detach()) if calibration_grad else (cam, grav))):
        confs = [pred.get(f"{f}_confidence") if use_uncertainty_loss else None for f in ("up", "latitude")]
        both = _FieldLossFunction.apply(pred.get("up_field"), pred.get("latitude_field"), camera.name(), cam, grav,
                                        *(None if c is None else c.detach() for c in confs), up_loss, latitude_loss,
                                        float(up_loss_weight), float(latitude_loss_weight))
        per_field = {name: both[:, i] for i, name in enumerate(("up", "latitude")) if f"{name}_field" in pred}
    else:
        weights = {"up": up_loss_weight, "latitude": latitude_loss_weight}
        per_field = {k: v * weights[k] for k, v in _field_loss_torch(pred, camera, gravity, types, use_uncertainty_loss).items()}
    out, total = {}, 0
    for name, loss in per_field.items():
        out[f"{name}-{types[name]}-loss"] = loss
        out[f"{name}_total"] = 0 + loss
        total = total + loss
    out["perspective_total"] = total
    return out


def perspective_decoder_loss(pred: Dict[str, torch.Tensor], camera: BaseCamera, gravity: Gravity,
                             recall_thresholds: Sequence[float] = (1, 3, 5, 10), **loss_options):
    """(losses, metrics), the pair PerspectiveDecoder.loss returns: perspective_field_loss(pred, camera, gravity,
    **loss_options) and metrics.perspective_field_metrics on the detached fields -- the scorer keeps its HIP pass while the
    loss carries the graph."""
    losses = perspective_field_loss(pred, camera, gravity, **loss_options)
    detached = {k: v.detach() for k, v in pred.items() if torch.is_tensor(v) and k in
                ("up_field", "latitude_field", "up_confidence", "latitude_confidence")}
    for name in ("up", "latitude"):
        conf = detached.get(f"{name}_confidence")
        if f"{name}_field" not in detached:
            detached.pop(f"{name}_confidence", None)
        elif conf is not None and conf.dim() == 4:
            detached[f"{name}_confidence"] = conf.reshape(conf.shape[0], *conf.shape[-2:])
    with torch.no_grad():
        return losses, metrics.perspective_field_metrics(detached, camera, gravity, recall_thresholds)


# ------------------------------------------------------------------------------------------ classification heads
def bin_loss(logits: torch.Tensor, target_bins: torch.Tensor, confidence: Optional[torch.Tensor] = None,
             use_uncertainty_loss: bool = True) -> torch.Tensor:
    """The loss of one classification head for explicit target bins, as a torch composition: logits (B, K, H, W), target_bins
    (B, H, W) integer, an optional confidence (B, H, W) or (B, 1, H, W); returns (B,).  Per pixel ce = logsumexp_k z_k - z_t
    (F.cross_entropy without a reduction); per image sum(w ce) / sum w with w the confidence, detached, when one is given and
    `use_uncertainty_loss`, else the mean -- the weighting of `field_loss`; sum conf = 0 gives NaN.  Half-precision logits are
    read as the float32 values they widen to; float64 stays float64.  Differentiable in the logits, on any device."""
    if logits.dim() != 4 or target_bins.shape != (logits.shape[0], *logits.shape[-2:]):
        raise ValueError(f"logits are (B, K, H, W) and target bins (B, H, W), got {tuple(logits.shape)} and {tuple(target_bins.shape)}")
    z = logits.float() if logits.dtype in (torch.float16, torch.bfloat16) else logits
    ce = torch.logsumexp(z, 1) - z.gather(1, target_bins.long()[:, None])[:, 0]
    if confidence is not None and use_uncertainty_loss:
        w = confidence.detach().reshape(ce.shape).to(ce.dtype)
        return (w * ce).sum((1, 2)) / w.sum((1, 2))
    return ce.mean((1, 2))


def bin_accuracy(logits: torch.Tensor, target_bins: torch.Tensor) -> torch.Tensor:
    """(B,): the share of pixels whose torch.argmax bin (the first index of the greatest value) is the target bin."""
    hits = logits.detach().argmax(1) == target_bins
    return hits.to(torch.float64 if logits.dtype == torch.float64 else torch.float32).mean((1, 2))


def perspective_target_bins(camera: BaseCamera, gravity: Gravity, up_bins: Optional[int] = None,
                            latitude_bins: Optional[int] = None):
    """(up bins, latitude bins), each (B, H, W) long or None where its count is: perspective_encoding.encode_up_bin /
    encode_bin_latitude of the fields get_perspective_field renders for the calibration, at the camera's size."""
    from . import perspective_encoding as pe
    up, lat = get_perspective_field(camera, gravity, use_up=up_bins is not None, use_latitude=latitude_bins is not None)
    up, lat = up.detach(), lat.detach()
    t_up = None if up_bins is None else torch.stack([pe.encode_up_bin(u, up_bins) for u in up])
    if latitude_bins is None:
        return t_up, None
    inner = pe._latitude_edges(latitude_bins)[1:].to(device=lat.device, dtype=lat.dtype)      # (encode_bin_latitude, any dtype)
    return t_up, torch.bucketize(lat[:, 0] / math.pi * 180, inner, right=False).long()


class _BinLossFunction(torch.autograd.Function):
    """(up_logits, lat_logits) -> ((B, 2) weighted losses [up, latitude], (B, 2) accuracies) on the HIP path; an absent head is
    None and its columns NaN."""

    @staticmethod
    def forward(ctx, up_logits, lat_logits, model, cam, grav, up_conf, lat_conf, up_weight, lat_weight):
        out, lse, bins = fields.bin_loss(model, cam, grav, up_logits, lat_logits, up_conf, lat_conf)
        ctx.save_for_backward(*(t for t in (up_logits, lat_logits, up_conf, lat_conf) if t is not None), lse, bins, out[:, 1::3])
        ctx.given = [t is not None for t in (up_logits, lat_logits, up_conf, lat_conf)]
        ctx.weights = (up_weight, lat_weight)
        pixels = lse.shape[-2] * lse.shape[-1]
        loss = torch.stack([out[:, 0] / out[:, 1] * up_weight, out[:, 3] / out[:, 4] * lat_weight], 1)
        accuracy = out[:, 2::3] / pixels
        ctx.mark_non_differentiable(accuracy)
        return loss, accuracy

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, _grad_accuracy):
        saved = list(ctx.saved_tensors)
        up_logits, lat_logits, up_conf, lat_conf = (saved.pop(0) if g else None for g in ctx.given)
        lse, bins, den = saved
        want_up, want_lat = ctx.needs_input_grad[:2]
        # grad_output x weight / denominator, on the device; an absent head's column is never read
        scale = grad_loss.to(torch.float32) / den
        scale[:, 0] *= ctx.weights[0]
        scale[:, 1] *= ctx.weights[1]
        g_up = g_lat = None
        if want_up or want_lat:                  # a head that asks for no gradient is left out of the pass
            g_up, g_lat = fields.bin_loss_grad(scale, lse, bins, up_logits if want_up else None, lat_logits if want_lat else None,
                                               up_conf if want_up else None, lat_conf if want_lat else None)
        return (g_up, g_lat) + (None,) * 7


def _bin_hip_path(logits, confs, cam: torch.Tensor, grav: torch.Tensor) -> bool:
    """Whether these inputs take gclm_bin_loss: contiguous float32, float16 or bfloat16 logits of one dtype, float32
    confidences, a float32 camera and gravity, all on one HIP device with matching batches."""
    dev = cam.device
    return (cam.is_cuda and all(t.device == dev for t in logits + confs + [grav])
            and all(t.dtype in (torch.float32, torch.float16, torch.bfloat16) and t.dtype == logits[0].dtype and t.is_contiguous()
                    for t in logits)
            and all(t.dtype == torch.float32 for t in confs + [cam, grav]) and cam.dim() == grav.dim() == 2
            and cam.shape[0] == grav.shape[0] and all(t.shape[0] == cam.shape[0] for t in logits))


def perspective_bin_loss(pred: Dict[str, torch.Tensor], camera: BaseCamera, gravity: Gravity, use_uncertainty_loss: bool = True,
                         up_loss_weight: float = 1.0, latitude_loss_weight: float = 1.0) -> Dict[str, torch.Tensor]:
    """The training loss of the classification heads in `pred` against the calibration (camera, gravity), per image: the
    cross-entropy of every pixel's logits against the bin of the calibration's perspective field there.

    `pred` holds "up_logits" (B, Ku, H, W) and / or "latitude_logits" (B, Kl, H, W) -- the heads fields.pack_fields_from_logits
    decodes, 73 and 180 bins in the original PerspectiveFields weights -- and optionally "up_confidence", "latitude_confidence"
    (B, H, W) or (B, 1, H, W).  The targets are perspective_encoding.encode_up_bin / encode_bin_latitude of
    get_perspective_field(camera, gravity), at (H, W); `bin_loss` is the definition of a head's loss.  Returns, each (B,):
    "up-classification-loss" and "up_total", "latitude-classification-loss" and "latitude_total" -- a head's keys only when the
    head is in `pred` --, "perspective_total", their sum, and "up_bin_accuracy" / "latitude_bin_accuracy", the share of pixels
    whose argmax bin is the target's (no graph).  The weights multiply the losses.  A confidence weights its head's pixels by
    conf / sum conf (detached) when `use_uncertainty_loss`; sum conf = 0 gives NaN.  No gradient goes to the confidences, the
    camera or the gravity: the targets are discrete.

    Contiguous float32, float16 or bfloat16 logits (both heads of one dtype) on one HIP device, with float32 confidences and a
    float32 camera and gravity (detached if they require grad), take the HIP path: one pass evaluates the target per pixel in
    registers, streams the logits once and reduces the loss per image (gclm_bin_loss); backward streams them once more and
    writes the gradients in the logits' dtype (gclm_bin_loss_grad) -- no field, no target map and no log-softmax is written.
    That path is once differentiable.  Anything else takes the torch composition.  Raises ValueError, on both paths, when
    neither head is given, for logits that are not 4-D of one (B, H, W), for fewer than 2 up bins, and for a latitude count
    whose classes perspective_encoding cannot lay out (its _latitude_edges raises)."""
    from . import perspective_encoding as pe
    names = [n for n in ("up", "latitude") if f"{n}_logits" in pred]
    if not names:
        raise ValueError("`pred` holds neither up_logits nor latitude_logits")
    logits = [pred[f"{n}_logits"] for n in names]
    if any(t.dim() != 4 for t in logits) or any(t.shape[0] != logits[0].shape[0] or t.shape[-2:] != logits[0].shape[-2:] for t in logits):
        raise ValueError(f"logits are (B, bins, H, W) of one B, H and W, got {[tuple(t.shape) for t in logits]}")
    B, (H, W) = logits[0].shape[0], logits[0].shape[-2:]
    counts = {n: int(t.shape[1]) for n, t in zip(names, logits)}
    if "up" in counts:
        pe._up_step(counts["up"])
    if "latitude" in counts:
        pe._latitude_edges(counts["latitude"])
    confs = {}
    for n in names:
        c = pred.get(f"{n}_confidence") if use_uncertainty_loss else None
        if c is not None:
            if c.numel() != B * H * W or c.shape[-2:] != (H, W):
                raise ValueError(f"`{n}_confidence` {tuple(c.shape)} does not fit {B} images of {H} x {W}")
            confs[n] = c.detach().reshape(B, H, W)
    if len(camera.shape) == 0:
        camera, gravity = camera.unsqueeze(0), gravity.unsqueeze(0)
    cam, grav = camera._data.detach(), gravity._data.detach()
    weights = {"up": float(up_loss_weight), "latitude": float(latitude_loss_weight)}
    if _bin_hip_path(logits, list(confs.values()), cam, grav) and max(counts.values()) <= _lib.MAX_BINS:
        both, acc = _BinLossFunction.apply(pred.get("up_logits"), pred.get("latitude_logits"), camera.name(), cam, grav,
                                           confs.get("up"), confs.get("latitude"), weights["up"], weights["latitude"])
        per_head = {n: (both[:, i], acc[:, i]) for i, n in enumerate(("up", "latitude")) if n in counts}
    else:
        targets = dict(zip(("up", "latitude"), perspective_target_bins(camera, gravity, counts.get("up"), counts.get("latitude"))))
        per_head = {}
        for n, z in zip(names, logits):
            t = targets[n].to(z.device)
            if t.shape != (B, H, W):
                raise ValueError(f"the camera's size gives targets {tuple(t.shape)}, the logits are {B} images of {H} x {W}")
            per_head[n] = (bin_loss(z, t, confs.get(n)) * weights[n], bin_accuracy(z, t))
    out, total = {}, 0
    for n, (loss, accuracy) in per_head.items():
        out[f"{n}-classification-loss"] = loss
        out[f"{n}_total"] = 0 + loss
        out[f"{n}_bin_accuracy"] = accuracy
        total = total + loss
    out["perspective_total"] = total
    return out
