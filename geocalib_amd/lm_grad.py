"""The unrolled LM loop as a torch composition, and the step record of the HIP solve.

`lm_unrolled_torch` restates LMOptimizer's loop (reference: geocalib/lm_optimizer.py:551-644) with torch operations only, on
any device and in any floating dtype, so autograd differentiates it: the gradients of the optimised camera and gravity
reach the predicted fields and both confidence maps through every LM step, as they do in the reference's training-time
optimiser (siclib/models/optimization/lm_optimizer.py).  It is the float64 yardstick of those gradients where the reference
is not at hand (tests/test_lm_grad_oracle.py holds it to the reference's own float64 gradients), not a fast path: one step
materialises the (B, N, 3, P) Jacobians.

  * fields: the package's torch field compositions (perspective_fields._up_field_torch, _latitude_field_torch);
  * updates: Gravity.update, BaseCamera.update_focal, BaseCamera.update_dist through LMOptimizer.update_estimate;
  * Jacobian: the derivative of fields(theta [+] delta) at delta = 0 over the full columns (d1, d2, focal, k...), taken
    column by column in forward mode; the free columns are then selected as the reference selects them.  That is the
    reference's analytic Jacobian as a function of theta (tests/test_lm_grad_oracle.py: golden_jac.npz), so its derivative with
    respect to theta -- which the backward pass needs -- is the reference's too;
  * the damping lambda depends on the costs through a comparison only: no gradient flows through it; the initial estimate
    is detached, as in the reference.

`recorded_solve` runs the HIP solve with a step record (gclm_solve_recorded / gclm_calibrate_recorded, include/gclm.h): per
executed LM step the state the step started from, the damping it used, the step it took and the reduced normal equations.
That is what an adjoint pass needs from the forward solve; results equal the plain solve's bit for bit.
"""
from typing import Any, Dict, Optional, Tuple

import torch
import torch.autograd.forward_ad as fwAD
from torch.autograd.function import once_differentiable

from . import _lib
from .camera import BaseCamera
from .gravity import Gravity
from .lm_optimizer import LMOptimizer, get_trivial_estimation, update_lambda
from .perspective_fields import _latitude_field_torch, _up_field_torch

_FLOAT32_EPS = float(torch.finfo(torch.float32).eps)


def _huber_weight(sq: torch.Tensor, scale: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(cost, weight) of squared residual norms: the reference's scaled Huber loss and its first derivative, its
    sqrt(x + 1e-8) and max(eps, .) included (geocalib/lm_optimizer.py:61-87)."""
    a2 = scale ** 2
    x = sq / a2
    inlier = x <= 1
    sx = torch.sqrt(x + 1e-8)
    isx = torch.clamp(1 / sx, min=_FLOAT32_EPS)
    return torch.where(inlier, x, 2 * sx - 1) * a2, torch.where(inlier, torch.ones_like(x), isx)


def _model_fields(camera: BaseCamera, gravity: Gravity, hw: Tuple[int, int], use_up: bool) -> torch.Tensor:
    """(B, N, 3) [up_x, up_y, sin(latitude)] of the calibration, or (B, N, 1) without the up field."""
    h, w = hw
    B = camera.shape[0]
    rows = [_up_field_torch(camera, gravity, h, w, True).reshape(B, h * w, 2)] if use_up else []
    rows.append(torch.sin(_latitude_field_torch(camera, gravity, h, w)).reshape(B, h * w, 1))
    return torch.cat(rows, -1)


def _full_update(camera: BaseCamera, gravity: Gravity, delta: torch.Tensor, rpf: bool = False) -> Tuple[BaseCamera, Gravity]:
    """theta [+] delta over the full columns (d1, d2, log focal, k...); `rpf`: over (roll, pitch, plain focal, k...), the
    parametrisation of the uncertainty pass."""
    g = gravity.update(delta[..., :2], spherical=not rpf)
    c = camera.update_focal(delta[..., 2:3], as_log=not rpf)
    if hasattr(c, "dist"):
        c = c.update_dist(delta[..., 3:3 + c.num_dist_params()])
    return c, g


def fields_and_jacobian(camera: BaseCamera, gravity: Gravity, hw: Tuple[int, int], use_up: bool = True, rpf: bool = False):
    """(model (B, N, R), J (B, N, R, P)) with R = 3 rows [up_x, up_y, sin latitude] (1 without the up field) and P = 3 +
    the model's distortion parameters: J[..., j] is the forward-mode derivative of fields(theta [+] delta) along column j
    at delta = 0, on the spherical manifold and the log focal length.  Both carry the autograd graph of (camera, gravity)."""
    B = camera.shape[0]
    P = 3 + (camera.num_dist_params() if hasattr(camera, "dist") else 0)
    zero = camera._data.new_zeros((B, P))
    model, cols = None, []
    for j in range(P):
        e = torch.zeros_like(zero)
        e[:, j] = 1
        with fwAD.dual_level():
            c, g = _full_update(camera, gravity, fwAD.make_dual(zero, e), rpf)
            out = fwAD.unpack_dual(_model_fields(c, g, hw, use_up))
            if model is None:
                model = out.primal
            t = out.tangent
            cols.append(t if t is not None else torch.zeros_like(out.primal))
    return model, torch.stack(cols, -1)


def _initial_estimate(opt: LMOptimizer, data: Dict[str, Any], dtype: torch.dtype):
    """get_trivial_estimation on the run's data, detached and cast to the run's dtype: the estimate itself is rounded to
    float32, as the reference rounds it (geocalib/lm_optimizer.py:50-52)."""
    camera, gravity = get_trivial_estimation({k: (v.detach() if torch.is_tensor(v) else v) for k, v in data.items()}, opt.camera_model)
    return opt.camera_model(camera._data.detach().to(dtype)), Gravity(gravity._data.detach().to(dtype))


def _soft_priors(data: Dict[str, Any], dtype: torch.dtype, B: int, device) -> Dict[str, torch.Tensor]:
    """The soft priors of `data` in `dtype`: {"f0", "sf"} and / or {"g0", "sg"} -- a prior with its standard deviation
    (`prior_focal_uncertainty` in pixels of fy, `prior_gravity_uncertainty` in radians); empty without either."""
    out = {}

    def vec(key, shape):
        t = data[key]
        t = t._data if hasattr(t, "_data") else torch.as_tensor(t)
        return t.detach().to(device=device, dtype=dtype).reshape(shape)

    for key, prior in (("prior_focal_uncertainty", "prior_focal"), ("prior_gravity_uncertainty", "prior_gravity")):
        if key in data and prior not in data:
            raise ValueError(f"lm_unrolled_torch: `{key}` needs `{prior}`")
    if "prior_focal_uncertainty" in data:
        out["f0"], out["sf"] = vec("prior_focal", (B,)), vec("prior_focal_uncertainty", (B,))
    if "prior_gravity_uncertainty" in data:
        g0 = vec("prior_gravity", (B, 3))
        out["g0"], out["sg"] = g0 / g0.norm(dim=-1, keepdim=True), vec("prior_gravity_uncertainty", (B,))
    return out


def soft_prior_terms(soft: Dict[str, torch.Tensor], camera: BaseCamera, gravity: Gravity, dims, rpf: bool = False):
    """(cost (B,), G (B, P), H (B, P, P)) of the soft priors at (camera, gravity) over the free columns `dims`, in the
    sum convention of the data terms (cost sum rho, H = sum w J^T J, G = sum w J^T r, r = target - model):
      focal    w = (f0 / sigma_f)^2, r = log f0 - log fy on the log-focal column;
      gravity  w = 1 / sigma_g^2, r = g0 - g, J = T, the tangent basis of the gravity columns (SphericalManifold.J_plus).
    `rpf`: the information in the uncertainty pass's parametrisation -- T = Gravity.J_rp, 1 / sigma_f^2 on the plain focal --
    with the same cost; G is then zero (the pass takes no step)."""
    fy = camera.f[..., 1]
    B, P = fy.shape[0], len(dims)
    cost, G, H = fy.new_zeros(B), fy.new_zeros(B, P), fy.new_zeros(B, P, P)
    if "sf" in soft:
        j = dims.index(2)
        w, r = (soft["f0"] / soft["sf"]) ** 2, torch.log(soft["f0"] / fy)
        cost = cost + w * r * r
        if rpf:
            H[:, j, j] = H[:, j, j] + 1 / soft["sf"] ** 2
        else:
            G[:, j] = G[:, j] + w * r
            H[:, j, j] = H[:, j, j] + w
    if "sg" in soft:
        assert dims[:2] == [0, 1]
        w, r = 1 / soft["sg"] ** 2, soft["g0"] - gravity.vec3d
        T = gravity.J_rp() if rpf else gravity.J_update(spherical=True)
        cost = cost + w * (r * r).sum(-1)
        if not rpf:
            G[:, :2] = G[:, :2] + w[:, None] * torch.einsum("bik,bi->bk", T, r)
        H[:, :2, :2] = H[:, :2, :2] + w[:, None, None] * torch.einsum("bik,bil->bkl", T, T)
    return cost, G, H


def lm_unrolled_torch(data: Dict[str, Any], conf: Optional[Dict[str, Any]] = None, dtype: torch.dtype = torch.float64,
                      init: Optional[Tuple[BaseCamera, Gravity]] = None, detach_init: bool = True) -> Dict[str, Any]:
    """The unrolled LM loop of LMOptimizer(conf) on `data`, in `dtype`, differentiable by autograd with respect to
    "up_field", "latitude_field", "up_confidence" and "latitude_confidence".

    `conf` takes LMOptimizer's keys; per-image solves on the spherical manifold and the log focal length (shared intrinsics,
    the manifold flags off and init_conf other than trivial raise ValueError).  `init` replaces the trivial initial estimate;
    it is detached, as the reference detaches its own, unless `detach_init` is False: then `init` (in `dtype`) is used as it
    stands, and autograd also reaches the state the loop starts from -- the state adjoint of a step (num_steps=1).
    Returns the dict of LMOptimizer.forward in training mode -- "camera", "gravity", "stop_at", the initial and final costs --
    plus "lambdas" (num executed steps, B), the damping after each step's rule, "deltas", the steps taken, and "hessians", each
    step's J^T W J over the free columns, before the damping.

    Soft priors (`prior_focal_uncertainty`, `prior_gravity_uncertainty` in `data`, each with its prior; LMOptimizer documents
    them): the prior seeds the initial estimate and keeps its column free, `soft_prior_terms` joins every step's system (the
    "hessians" are then the systems as solved) and prior / N the compared cost; the dict gains "initial_prior_cost" and
    "final_prior_cost", and "initial_cost" / "final_cost" are the compared sums.  Without those keys nothing changes."""
    opt = LMOptimizer(dict(conf or {}))
    c = opt.conf
    if c.shared_intrinsics or not (c.use_spherical_manifold and c.use_log_focal):
        raise ValueError("lm_unrolled_torch: per-image solves on the spherical manifold and the log focal length only")
    if init is None and opt._init_name != "trivial":
        raise ValueError("lm_unrolled_torch: the trivial initial estimate, or an explicit `init`")
    lat = data["latitude_field"]
    B, (h, w) = lat.shape[0], lat.shape[-2:]
    use_up = "up_field" in data
    d = {k: data[k].to(dtype) for k in ("up_field", "latitude_field", "up_confidence", "latitude_confidence") if k in data}
    opt.setup_optimization_and_priors(data, shared_intrinsics=False)
    if init is None:
        camera, gravity = _initial_estimate(opt, {**data, **d}, dtype)
    elif detach_init:
        camera, gravity = init[0].__class__(init[0]._data.detach().to(dtype)), Gravity(init[1]._data.detach().to(dtype))
    else:
        camera, gravity = init
        if camera._data.dtype is not dtype or gravity._data.dtype is not dtype:
            raise ValueError(f"lm_unrolled_torch: with detach_init=False `init` must be {dtype}")
    squared = c.loss_fn == "squared_loss"
    scales = [opt._SQUARED_LOSS_SCALE if squared else float(s) for s in (c.up_loss_fn_scale, c.lat_loss_fn_scale)]

    target = [d["up_field"].permute(0, 2, 3, 1).reshape(B, h * w, 2)] if use_up else []
    target.append(torch.sin(d["latitude_field"]).permute(0, 2, 3, 1).reshape(B, h * w, 1))
    target = torch.cat(target, -1)
    confs = [d["up_confidence"].reshape(B, -1) if "up_confidence" in d and use_up else None,
             d["latitude_confidence"].reshape(B, -1) if "latitude_confidence" in d else None]

    def costs_weights(model):
        """({name: (B, N) cost}, (B, N, R) weight of every residual row, residuals)"""
        r = target - model
        out, ws = {}, []
        parts = ((("up", r[..., :2], scales[0], confs[0]),) if use_up else ()) + (("latitude", r[..., -1:], scales[1], confs[1]),)
        for name, rr, a, cf in parts:
            cost, wt = _huber_weight((rr ** 2).sum(-1), a)
            if cf is not None:
                cost, wt = cost * cf, wt * cf
            out[f"{name}_cost"] = cost
            ws.append(wt[..., None].expand_as(rr))
        return out, torch.cat(ws, -1), r

    total = lambda costs: sum(v.mean(-1) for v in costs.values())  # noqa: E731
    dims = opt._column_dims()
    soft = _soft_priors(data, dtype, B, d["latitude_field"].device)
    prior_mean = lambda cam, grav: soft_prior_terms(soft, cam, grav, dims)[0] / (h * w)  # noqa: E731
    lamb = d["latitude_field"].new_full((B,), float(c.lambda_))
    infos: Dict[str, Any] = {"stop_at": opt.num_steps}
    lambdas, deltas, hessians, prev_cost = [], [], [], None
    for i in range(opt.num_steps):
        model, J = fields_and_jacobian(camera, gravity, (h, w), use_up)
        costs, wt, r = costs_weights(model)
        if i == 0:
            prev_cost = total(costs)
            infos.update({f"initial_{k}": v.mean(-1) for k, v in costs.items()})
            if soft:
                infos["initial_prior_cost"] = prior_mean(camera, gravity)
                prev_cost = prev_cost + infos["initial_prior_cost"]
            infos["initial_cost"] = prev_cost
        J = J[..., dims]
        wr = wt * r
        G = torch.einsum("bnrk,bnr->bk", J, wr)
        Hm = torch.einsum("bnrk,bnr,bnrl->bkl", J, wt, J)
        if soft:
            _, Gp, Hp = soft_prior_terms(soft, camera, gravity, dims)
            G, Hm = G + Gp, Hm + Hp
        damp = (Hm.diagonal(dim1=-2, dim2=-1) * lamb[:, None]).clamp(min=1e-6)
        A = Hm + torch.diag_embed(damp)
        L, fail = torch.linalg.cholesky_ex(A)
        if bool(fail.any()):                    # the reference: a zero step for the whole batch
            delta = torch.zeros_like(G)
        else:
            delta = torch.cholesky_solve(G[..., None], L)[..., 0]
        deltas.append(delta.detach())
        hessians.append(Hm.detach())
        camera, gravity = opt.update_estimate(camera, gravity, delta)
        new_cost = total(costs_weights(_model_fields(camera, gravity, (h, w), use_up))[0])
        if soft:
            new_cost = new_cost + prior_mean(camera, gravity)
        if not c.fix_lambda:
            lamb = update_lambda(lamb, prev_cost.detach(), new_cost.detach())
        lambdas.append(lamb.detach().clone())
        if torch.allclose(new_cost, prev_cost, atol=c.atol, rtol=c.rtol):
            infos["stop_at"] = min(i + 1, infos["stop_at"])
            if c.early_stop:
                break
        prev_cost = new_cost
    final = costs_weights(_model_fields(camera, gravity, (h, w), use_up))[0]
    infos["stop_at"] = camera._data.new_ones(B) * infos["stop_at"]
    infos.update({f"final_{k}": v.mean(-1) for k, v in final.items()})
    infos["final_cost"] = total(final)
    if soft:
        infos["final_prior_cost"] = prior_mean(camera, gravity)
        infos["final_cost"] = infos["final_cost"] + infos["final_prior_cost"]
    infos["lambdas"] = torch.stack(lambdas) if lambdas else lamb.new_zeros((0, B))
    infos["deltas"] = torch.stack(deltas) if deltas else lamb.new_zeros((0, B, len(dims)))
    infos["hessians"] = torch.stack(hessians) if hessians else lamb.new_zeros((0, B, len(dims), len(dims)))
    return {"camera": camera, "gravity": gravity, **infos}


# ---------------------------------------------------------------------------------------------- the HIP solve's step record

RECORD = {"camera": slice(0, 8), "gravity": slice(8, 11), "lambda": 11, "delta": slice(12, 17), "failed": 17, "executed": 18,
          "system": slice(24, 24 + 24)}


def recorded_solve(optimizer: LMOptimizer, data: Dict[str, torch.Tensor], init: Optional[Tuple[BaseCamera, Gravity]] = None):
    """(camera, gravity, infos, record): LMOptimizer.calibrate_fields (or .optimize from `init`) with the step record of
    gclm_calibrate_recorded / gclm_solve_recorded, (B, num_steps, LM_RECORD_STRIDE) float32 on the fields' device.  Slices of
    a record row are in `RECORD`: the camera row and gravity the step started from, the damping it used, the full-size step
    (d1, d2, focal, k1, k2; zeros in fixed columns and after a failed Cholesky), the "failed" and "executed" flags, and the
    reduced accumulator record of the step's sweep (costs, J^T W r, upper triangle of J^T W J).  A step after an early stop
    leaves its row zero.  Per-image solves of one call only (B <= LMOptimizer._MAX_CALL, no shared intrinsics); results equal
    the plain solve's bit for bit."""
    if optimizer.shared_intrinsics:
        raise ValueError("recorded_solve: per-image solves only (shared_intrinsics=False)")
    B = data["latitude_field"].shape[0]
    if B > optimizer._MAX_CALL:
        raise ValueError(f"recorded_solve: at most {optimizer._MAX_CALL} images per call")
    if "sin_latitude" in data:
        raise ValueError("recorded_solve: the recorded solve reads the latitudes in radians; drop `sin_latitude`")
    with torch.no_grad():
        optimizer.setup_optimization_and_priors(data, shared_intrinsics=False)
        dev = data["latitude_field"].device
        record = torch.empty((B, max(int(optimizer.num_steps), 1), _lib.LM_RECORD_STRIDE), dtype=torch.float32, device=dev)
        if init is None:
            cam, grav, infos = optimizer.calibrate_fields(data, record=record)
        else:
            cam, grav, infos = optimizer.optimize(data, init[0], init[1], record=record)
    return cam, grav, infos, record[:, :int(optimizer.num_steps)]


# ---------------------------------------------------------------------------------------------- the differentiable HIP solve

_GRAD_INPUTS = ("up_field", "latitude_field", "up_confidence", "latitude_confidence")
_GRAD_MODELS = ("pinhole", "simple_radial")


def check_differentiable(optimizer: LMOptimizer, data: Dict[str, Any]) -> None:
    """What LMOptimizer({"differentiable": True}) covers; anything else raises a ValueError that names the limit, before the
    library is touched.  The priors and `scales` are not checked: calibrate_fields converts them to float32 on the fields'
    device whatever they come as, and they take no gradient."""
    c, who = optimizer.conf, "LMOptimizer(differentiable=True)"
    if c.verbose:
        raise ValueError(f"{who}: conf.verbose is not covered (its log lines synchronise the device around the plain solve)")
    name = optimizer.camera_model.name()
    if name not in _GRAD_MODELS:
        raise ValueError(f"{who}: camera models {_GRAD_MODELS} only, got `{name}`")
    if optimizer.shared_intrinsics or c.shared_intrinsics:
        raise ValueError(f"{who}: per-image solves only (shared_intrinsics=False)")
    if optimizer._init_name not in ("trivial", "heuristic"):
        raise ValueError(f"{who}: init_conf trivial or heuristic only, got `{optimizer._init_name}`")
    if not (c.use_spherical_manifold and c.use_log_focal):
        raise ValueError(f"{who}: use_spherical_manifold and use_log_focal must stay True")
    if c.loss_fn not in ("huber_loss", "squared_loss"):
        raise ValueError(f"{who}: loss_fn huber_loss or squared_loss, got `{c.loss_fn}`")
    if not 1 <= int(optimizer.num_steps) <= 256:
        raise ValueError(f"{who}: num_steps in 1 .. 256, got {optimizer.num_steps}")
    if "sin_latitude" in data:
        raise ValueError(f"{who}: the solve reads `latitude_field` in radians; drop `sin_latitude` (it would take no gradient)")
    lat = data["latitude_field"]
    if lat.shape[0] > optimizer._MAX_CALL:
        raise ValueError(f"{who}: at most {optimizer._MAX_CALL} images per call")
    for k in _GRAD_INPUTS:
        t = data.get(k)
        if t is None:
            continue
        if t.dtype is not torch.float32:
            raise ValueError(f"{who}: `{k}` must be float32, got {t.dtype}")
        if not t.is_cuda:
            raise ValueError(f"{who}: `{k}` must live on a HIP device, got {t.device}")


class _LMSolveFunction(torch.autograd.Function):
    """(up, lat, up_conf, lat_conf) -> (camera data (B, 8), gravity data (B, 3), info rows): the recorded HIP solve forward,
    gclm_lm_backward backward.  Absent inputs are None.  Once differentiable."""

    @staticmethod
    def forward(ctx, optimizer, rest, up, lat, upc, latc):
        data = dict(rest)
        for k, t in zip(_GRAD_INPUTS, (up, lat, upc, latc)):
            if t is not None:
                data[k] = t.detach()
        cam, grav, _, record = recorded_solve(optimizer, data)
        info = optimizer._last_raw[2]
        c = optimizer.conf
        squared = c.loss_fn == "squared_loss"
        ctx.call = (optimizer.camera_model.name(), int(optimizer.num_steps), int(bool(c.early_stop)),
                    optimizer._SQUARED_LOSS_SCALE if squared else float(c.up_loss_fn_scale),
                    optimizer._SQUARED_LOSS_SCALE if squared else float(c.lat_loss_fn_scale),
                    int(optimizer.estimate_gravity), int(optimizer.estimate_focal), int(optimizer.estimate_dist))
        planes = optimizer._fields(data)[:4]
        ctx.given = [t is not None for t in planes]
        ctx.shapes = [None if t is None else t.shape for t in (up, lat, upc, latc)]
        ctx.save_for_backward(*(t for t in planes if t is not None), record, info)
        ctx.mark_non_differentiable(info)
        return cam._data, grav._data, info

    @staticmethod
    @once_differentiable
    def backward(ctx, g_cam, g_grav, _g_info):
        from . import _call
        saved = list(ctx.saved_tensors)
        up, lat, upc, latc = (saved.pop(0) if g else None for g in ctx.given)
        record, info = saved
        model, steps, early, up_scale, lat_scale, eg, ef, ed = ctx.call
        B, _, H, W = lat.shape
        dev = lat.device
        g_cam = torch.zeros((B, 8), dtype=torch.float32, device=dev) if g_cam is None else _call.dev_f32(g_cam, "grad camera")
        g_grav = torch.zeros((B, 3), dtype=torch.float32, device=dev) if g_grav is None else _call.dev_f32(g_grav, "grad gravity")
        need = ctx.needs_input_grad[2:6]
        # a plane nobody asked for, or whose input is absent, is None: neither computed nor written
        outs = [torch.empty_like(t) if t is not None and n else None for t, n in zip((up, lat, upc, latc), need)]
        ws_bytes = int(_lib.load().gclm_lm_backward_workspace(B, H, W))
        if ws_bytes == 0:
            raise _lib.GclmError(f"gclm_lm_backward: sizes out of range (B={B}, H={H}, W={W})")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        P = _call.ptr
        _call.call("gclm_lm_backward", _lib.CAMERA_MODEL_IDS[model], P(up), P(lat), P(upc), P(latc), B, H, W, record.data_ptr(), steps,
                   early, info.data_ptr(), up_scale, lat_scale, eg, ef, ed, g_cam.data_ptr(), g_grav.data_ptr(), *(P(t) for t in outs),
                   ws.data_ptr(), ws_bytes, _call.raw_stream(dev), device=dev)
        grads = [None if t is None else t.reshape(s) for t, s in zip(outs, ctx.shapes)]
        return (None, None, *grads)


def differentiable_forward(optimizer: LMOptimizer, data: Dict[str, Any]) -> Dict[str, Any]:
    """LMOptimizer.forward with conf.differentiable: the dict of the plain forward, bit for bit, with a camera and a gravity
    whose `_data` carry the graph of _LMSolveFunction; the infos carry none."""
    data["latitude_field"]            # KeyError like get_trivial_estimation
    check_differentiable(optimizer, data)
    rest = {k: v for k, v in data.items() if k not in _GRAD_INPUTS}
    has_up = "up_field" in data
    args = [data.get(k) for k in _GRAD_INPUTS]
    if not has_up:
        args[2] = None                 # a confidence without its field is not read
    cam, grav, info = _LMSolveFunction.apply(optimizer, rest, *args)
    from .lm_optimizer import _unit_gravity
    return {"camera": optimizer.camera_model(cam), "gravity": _unit_gravity(grav), **optimizer._unpack_info(info, has_up)}
