"""PerspectiveParamOpt: Adam on (roll, pitch, vfov) of a pinhole camera against predicted perspective fields (reference:
siclib/models/optimization/perspective_opt.py, the optimiser of the original PerspectiveFields pipeline and the baseline
the reference's evaluation compares the LM with).

The reference takes one image per call, renders both fields and runs autograd every step.  Here the whole batch runs on the
device (C: gclm_param_opt): a step is one HIP pass over the three planes with the gradient in closed form, and one small
launch that does, per image, the reference's Adam step, ReduceLROnPlateau step and check_convergence.  Every image is its own
reference call -- own moments, own learning rate, own stop --, so a batch gives per image the bits of that image alone.
There is no CPU path: the fields must live on a HIP device."""
import math
from types import SimpleNamespace
from typing import Any, Dict

import torch
from torch import nn

from . import _call, _lib, metrics
from .camera import Pinhole
from .gravity import Gravity

_SCHEDULER_OPTIONS = {"mode": "min", "patience": 10, "factor": 0.1, "threshold": 1e-4, "threshold_mode": "rel", "cooldown": 0,
                      "min_lr": 0.0, "eps": 1e-8}        # torch's ReduceLROnPlateau defaults


def _fields(data: Dict[str, torch.Tensor]):
    up, lat = _call.dev_f32(data["up_field"], "up_field"), _call.dev_f32(data["latitude_field"], "latitude_field")
    if up.dim() != 4 or up.shape[1] != 2 or lat.dim() != 4 or lat.shape[1] != 1 or up.shape[0] != lat.shape[0] \
            or up.shape[-2:] != lat.shape[-2:] or up.device != lat.device:
        raise ValueError(f"`up_field` {tuple(up.shape)} and `latitude_field` {tuple(lat.shape)} must be (B, 2, H, W) and "
                         "(B, 1, H, W) on one device")
    B, _, H, W = up.shape
    if B < 1 or H < 2 or W < 2:
        raise ValueError(f"{B} images of {H} x {W}: at least one image of 2 x 2 is needed")
    return up, lat, B, H, W


def _workspace(B: int, H: int, W: int, dev) -> torch.Tensor:
    nbytes = int(_lib.load().gclm_param_opt_workspace(min(B, _call.MAX_CALL), H, W))
    if nbytes == 0:
        raise ValueError(f"images of {H} x {W} are out of range")
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)


def _rpv(camera_or_rpv, B: int, dev) -> torch.Tensor:
    """(B, 3) float32 (roll, pitch, vfov): a tensor as it is, or a (camera, gravity) pair read as the reference reads its own."""
    if isinstance(camera_or_rpv, (tuple, list)):
        camera, gravity = camera_or_rpv
        camera_or_rpv = torch.stack([gravity.roll.reshape(-1), gravity.pitch.reshape(-1), camera.vfov.reshape(-1)], -1)
    rpv = _call.dev_f32(camera_or_rpv, "rpv").reshape(-1, 3)
    if rpv.shape[0] != B or rpv.device != dev:
        raise ValueError(f"{rpv.shape[0]} parameter rows on {rpv.device} for {B} images on {dev}")
    return rpv


def cost_function(camera_or_rpv, data: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The reference's cost and its gradient at given parameters, in one pass (C: gclm_param_opt_cost).  `camera_or_rpv`: a
    (B, 3) tensor of (roll, pitch, vfov) in radians or a (Pinhole, Gravity) pair; `data`: "up_field" (B, 2, H, W) and
    "latitude_field" (B, 1, H, W) on a HIP device.  Returns per image (B,) "up" and "latitude" -- the two means of
    PerspectiveParamOpt.cost_function; its "total" is lamb * latitude + (1 - lamb) * up -- and (B, 3) "up_grad", "latitude_grad":
    their derivatives with respect to (roll, pitch, vfov)."""
    up, lat, B, H, W = _fields(data)
    rpv = _rpv(camera_or_rpv, B, up.device)
    out = up.new_empty((B, 8))
    ws = _workspace(B, H, W, up.device)
    for b0, n in _call.slices(B):
        _call.call("gclm_param_opt_cost", _call.ptr_at(up, b0), _call.ptr_at(lat, b0), _call.ptr_at(rpv, b0), n, H, W, ws.data_ptr(),
                   ws.numel() * 8, _call.ptr_at(out, b0), _call.raw_stream(up.device), device=up.device)
    return {"up": out[:, 0], "latitude": out[:, 1], "up_grad": out[:, 2:5], "latitude_grad": out[:, 5:8]}


class PerspectiveParamOpt(nn.Module):
    """The reference's module for any B >= 1: same `default_conf` keys plus `poll_every`, same output keys plus the per-image
    `steps`, `converged` and final costs.  `lr_scheduler.name` is "ReduceLROnPlateau" or None; its options are torch's, of which
    mode "min" and threshold_mode "rel" are provided.  `verbose` is accepted and prints nothing."""

    default_conf = {
        "max_steps": 1000,
        "lr": 0.01,
        "lr_scheduler": {"name": "ReduceLROnPlateau", "options": {"mode": "min", "patience": 3}},
        "patience": 3,
        "abs_tol": 1e-7,
        "rel_tol": 1e-9,
        "lamb": 0.5,
        "verbose": False,
        # extension: read the count of live images back every n steps and stop launching once none is left (0: never; the
        # results are the same bits either way)
        "poll_every": 16,
    }
    required_data_keys = ["up_field", "latitude_field"]

    def __init__(self, conf: Dict[str, Any] = None):
        super().__init__()
        conf = dict(conf or {})
        unknown = set(conf) - set(self.default_conf)
        if unknown:
            raise ValueError(f"unknown PerspectiveParamOpt conf keys: {sorted(unknown)}")
        self.conf = c = SimpleNamespace(**{**self.default_conf, **conf})
        sched = dict(c.lr_scheduler or {"name": None})
        name, options = sched.get("name"), dict(sched.get("options") or {})
        if name not in (None, "ReduceLROnPlateau"):
            raise NotImplementedError(f"lr_scheduler {name!r}: only \"ReduceLROnPlateau\" (or None) is provided")
        extra = set(sched) - {"name", "options"} or set(options) - set(_SCHEDULER_OPTIONS)
        if extra:
            raise NotImplementedError(f"lr_scheduler keys or options {sorted(extra)} are not provided")
        o = {**_SCHEDULER_OPTIONS, **options}
        if o["mode"] != "min" or o["threshold_mode"] != "rel":
            raise NotImplementedError(f"ReduceLROnPlateau mode {o['mode']!r} / threshold_mode {o['threshold_mode']!r}: only "
                                      "\"min\" / \"rel\" are provided")
        if isinstance(o["min_lr"], (list, tuple)):
            raise NotImplementedError("ReduceLROnPlateau min_lr per parameter group is not provided")
        if not 1 <= int(c.patience) <= _lib.PARAM_OPT_MAX_PATIENCE:
            raise ValueError(f"patience = {c.patience} must lie in 1..{_lib.PARAM_OPT_MAX_PATIENCE}")
        if not 0.0 <= float(o["factor"]) < 1.0:
            raise ValueError("ReduceLROnPlateau factor must lie in [0, 1)")
        if int(c.max_steps) < 1 or not (0 <= float(c.lr) < math.inf) or not 0.0 <= float(c.lamb) <= 1.0:
            raise ValueError(f"max_steps = {c.max_steps}, lr = {c.lr}, lamb = {c.lamb}: need max_steps >= 1, a finite lr >= 0 and "
                             "lamb in [0, 1]")
        self._scheduler = None if name is None else o

    def _config(self) -> "_lib.GclmParamOptConfig":
        c, o = self.conf, self._scheduler
        cfg = _lib.GclmParamOptConfig.default()
        cfg.max_steps, cfg.patience, cfg.poll_every = int(c.max_steps), int(c.patience), int(c.poll_every)
        cfg.lr, cfg.abs_tol, cfg.rel_tol, cfg.lamb = float(c.lr), float(c.abs_tol), float(c.rel_tol), float(c.lamb)
        cfg.use_scheduler = 0 if o is None else 1
        if o is not None:
            cfg.sched_patience, cfg.sched_cooldown = int(o["patience"]), int(o["cooldown"])
            cfg.sched_factor, cfg.sched_threshold = float(o["factor"]), float(o["threshold"])
            cfg.sched_min_lr, cfg.sched_eps = float(o["min_lr"]), float(o["eps"])
        return cfg

    def cost_function(self, camera_or_rpv, data: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """The module-level cost_function plus "total" at this module's `lamb`."""
        out = cost_function(camera_or_rpv, data)
        lamb = float(self.conf.lamb)
        out["total"] = (lamb * out["latitude"].double() + (1 - lamb) * out["up"].double()).float()
        return out

    def forward(self, data: Dict[str, torch.Tensor], init=None) -> Dict[str, Any]:
        """`data`: "up_field" (B, 2, H, W), "latitude_field" (B, 1, H, W) on a HIP device.  `init`: optional (B, 3) (roll, pitch,
        vfov) or (Pinhole, Gravity) to start from, else the reference's _get_init_params.  Returns camera_opt (Pinhole, B),
        gravity_opt (Gravity, B), and per image steps (int32), converged (bool), final_cost / final_up_cost /
        final_latitude_cost (the last evaluated loss, as the reference's last `loss`), lr and initial (B, 3)."""
        up, lat, B, H, W = _fields(data)
        dev = up.device
        init = None if init is None else _rpv(init, B, dev)
        rpv, info = up.new_empty((B, 3)), up.new_empty((B, _lib.PARAM_OPT_INFO_WORDS))
        ws, cfg = _workspace(B, H, W, dev), self._config()
        for b0, n in _call.slices(B):
            _call.call("gclm_param_opt", _call.ptr_at(up, b0), _call.ptr_at(lat, b0), _call.ptr_at(init, b0), n, H, W,
                       _lib.C.byref(cfg), ws.data_ptr(), ws.numel() * 8, _call.ptr_at(rpv, b0), _call.ptr_at(info, b0),
                       _call.raw_stream(dev), device=dev)
        size = up.new_ones(B)
        camera = Pinhole.from_dict({"height": size * H, "width": size * W, "vfov": rpv[:, 2]})
        k = _lib.PARAM_OPT_INFO
        return {"camera_opt": camera, "gravity_opt": Gravity.from_rp(rpv[:, 0], rpv[:, 1]), "steps": info[:, k["steps"]].to(torch.int32),
                "converged": info[:, k["converged"]] != 0, "final_cost": info[:, k["final_cost"]],
                "final_up_cost": info[:, k["final_up_cost"]], "final_latitude_cost": info[:, k["final_latitude_cost"]],
                "lr": info[:, k["lr"]], "initial": info[:, k["initial"]:k["initial"] + 3], "rpv": rpv}

    def metrics(self, pred: Dict[str, Any], data: Dict[str, Any]) -> Dict[str, torch.Tensor]:
        return {"roll_opt_error": metrics.roll_error(pred["gravity_opt"], data["gravity"]),
                "pitch_opt_error": metrics.pitch_error(pred["gravity_opt"], data["gravity"]),
                "vfov_opt_error": metrics.vfov_error(pred["camera_opt"], data["camera"])}
