"""What the soft-prior tests share (a plain module, like the *_gate.py files): the inputs, the priors and the float64 yardstick's
posterior covariance.

Inputs: the recipe of tests/golden/make_golden_lm_grad.py (`make`) with the package's own classes -- random roll, pitch and
vfov (k1 for a distortion model; float32 draws, taken to float64 before anything is computed from them, so that the inputs do
not depend on a machine's float32 tan and sin), the fields rendered by the package's torch `get_perspective_field` in float64, noise 0.03 on
both fields, 5 % latitude outliers of 0.4 rad, confidences in 0.05 .. 0.95, everything rounded to float32.  The priors are off
the truth by 10 % (focal) and 0.07 rad (gravity: roll + 0.05, pitch - 0.05)."""
import functools

import torch

from geocalib_amd import LMOptimizer, lm_grad
from geocalib_amd.camera import camera_models
from geocalib_amd.gravity import Gravity
from geocalib_amd.perspective_fields import get_perspective_field

FIELDS = ("up_field", "latitude_field", "up_confidence", "latitude_confidence")


@functools.lru_cache(maxsize=None)
def make(model, B, H, W, seed):
    """(data, priors, gt_camera, gt_gravity): float32 CPU tensors; priors = {"prior_focal", "prior_gravity"}."""
    g = torch.Generator().manual_seed(seed)
    roll = (torch.rand(B, generator=g) - .5) * 0.6
    pitch = (torch.rand(B, generator=g) - .5) * 0.6
    vfov = 0.7 + 0.6 * torch.rand(B, generator=g)
    d = {"width": torch.full((B,), float(W)), "height": torch.full((B,), float(H)), "vfov": vfov}
    if model != "pinhole":
        d["k1"] = (torch.rand(B, generator=g) - .5) * 0.2
    # the draws are float32 (the generator's), everything computed from them float64: a float32 tan or sin differs in its last
    # bit between machines, and with it the inputs
    roll, pitch, d = roll.double(), pitch.double(), {k: v.double() for k, v in d.items()}
    cam = camera_models[model].from_dict(d).double()
    grav = Gravity.from_rp(roll, pitch).double()
    up, lat = get_perspective_field(cam, grav)
    up = up + 0.03 * torch.randn(up.shape, generator=g, dtype=torch.float64)
    lat = lat + 0.03 * torch.randn(lat.shape, generator=g, dtype=torch.float64)
    lat = lat + (torch.rand(B, H, W, generator=g) < 0.05)[:, None] * 0.4
    upc = 0.05 + 0.9 * torch.rand(B, H, W, generator=g, dtype=torch.float64)
    latc = 0.05 + 0.9 * torch.rand(B, H, W, generator=g, dtype=torch.float64)
    data = {k: v.float() for k, v in zip(FIELDS, (up, lat, upc, latc))}
    priors = {"prior_focal": (cam.f[:, 1] * 1.10).float(), "prior_gravity": Gravity.from_rp(roll + 0.05, pitch - 0.05).vec3d.float()}
    return data, priors, cam, grav


def conf_for(model, loss, steps=5):
    c = {"camera_model": model, "num_steps": steps, "early_stop": False}
    return {**c, "loss_fn": "squared_loss"} if loss == "squared" else {**c, "up_loss_fn_scale": 1e-2, "lat_loss_fn_scale": 1e-2}


KINDS = ("focal", "gravity", "both", "gravity_hard_focal")


def with_priors(data, priors, kind, sigma_f, sigma_g):
    """`data` plus the priors of `kind`: soft focal, soft gravity, both, or a soft gravity with a HARD focal."""
    out = dict(data)
    if kind in ("focal", "both"):
        out.update(prior_focal=priors["prior_focal"], prior_focal_uncertainty=sigma_f)
    if kind in ("gravity", "both", "gravity_hard_focal"):
        out.update(prior_gravity=priors["prior_gravity"], prior_gravity_uncertainty=sigma_g)
    if kind == "gravity_hard_focal":
        out["prior_focal"] = priors["prior_focal"]
    return out


def state(out):
    """(fy (B,), gravity (B,3), k1 (B,) or zeros) of a result dict, float64 on the CPU."""
    cam = out["camera"]._data.detach().double().cpu()
    k1 = cam[:, 6] if cam.shape[-1] > 6 else torch.zeros_like(cam[:, 3])
    return cam[:, 3], out["gravity"]._data.detach().double().cpu(), k1


def state_distance(sa, sb):
    """The distance of two states (fy, gravity, k1): the largest of |fy / fy' - 1|, |g - g'| (max-norm) and |k1 - k1'| over the images."""
    (fa, ga, ka), (fb, gb, kb) = sa, sb
    return max(float((fa / fb - 1).abs().max()), float((ga - gb).abs().max()), float((ka - kb).abs().max()))


def state_error(a, b):
    """state_distance of two result dicts."""
    return state_distance(state(a), state(b))


def packed(out):
    """state(out) as one (B, 5) float64 array [fy, gx, gy, gz, k1] (tests/golden/soft_priors_yardstick.npz), and back."""
    fy, g, k1 = state(out)
    return torch.cat([fy[:, None], g, k1[:, None]], 1).numpy()


def unpacked(rows):
    t = torch.as_tensor(rows, dtype=torch.float64)
    return t[:, 0], t[:, 1:4], t[:, 4]


def free_sigmas(data, conf):
    """(sigma_f, sigma_g) (B,) float32 read off a FREE float64 solve of the yardstick on `data`: the square root of its focal
    variance and of the larger eigenvalue of its gravity block."""
    free = lm_grad.lm_unrolled_torch(data, conf)
    cov = yardstick_covariance(data, conf, free["camera"], free["gravity"])
    return cov[:, 2, 2].sqrt().float(), torch.linalg.eigvalsh(cov[:, :2, :2])[:, -1].sqrt().float()


def yardstick_covariance(data, conf, camera, gravity):
    """inv(H_data + H_prior) in float64 at (camera, gravity), over the free columns in the uncertainty pass's parametrisation
    (roll, pitch, plain focal, k...): the data term from lm_grad's forward-mode Jacobian with the Huber weights of that state,
    the prior term from lm_grad.soft_prior_terms(rpf=True).  (B, P, P)."""
    opt = LMOptimizer(dict(conf))
    opt.setup_optimization_and_priors(data, shared_intrinsics=False)
    dims = opt._column_dims()
    dt = torch.float64
    lat = data["latitude_field"].to(dt)
    B, (h, w) = lat.shape[0], lat.shape[-2:]
    camera, gravity = camera.__class__(camera._data.detach().to(dt)), Gravity(gravity._data.detach().to(dt))
    model, J = lm_grad.fields_and_jacobian(camera, gravity, (h, w), True, rpf=True)
    target = torch.cat([data["up_field"].to(dt).permute(0, 2, 3, 1).reshape(B, h * w, 2),
                        torch.sin(lat).permute(0, 2, 3, 1).reshape(B, h * w, 1)], -1)
    r = target - model
    squared = conf.get("loss_fn") == "squared_loss"
    ws = []
    for rr, key, ckey in ((r[..., :2], "up_loss_fn_scale", "up_confidence"), (r[..., 2:], "lat_loss_fn_scale", "latitude_confidence")):
        a = LMOptimizer._SQUARED_LOSS_SCALE if squared else float(conf.get(key, 1e-2))
        wt = lm_grad._huber_weight((rr ** 2).sum(-1), a)[1] * data[ckey].to(dt).reshape(B, -1)
        ws.append(wt[..., None].expand_as(rr))
    wt = torch.cat(ws, -1)
    J = J[..., dims]
    Hm = torch.einsum("bnrk,bnr,bnrl->bkl", J, wt, J)
    soft = lm_grad._soft_priors(data, dt, B, lat.device)
    if soft:
        Hm = Hm + lm_grad.soft_prior_terms(soft, camera, gravity, dims, rpf=True)[2]
    return torch.linalg.inv(Hm)
