"""lm_grad.lm_unrolled_torch in float64 against the reference's own float64 autograd (tests/golden/lm_grad_reference.npz,
written by tests/golden/make_golden_lm_grad.py): gradients of the recorded L with respect to the four inputs, the final
state, the damping decisions -- and its forward-mode Jacobian against the reference's analytic one (golden_jac.npz).  No GPU.

Both sides are float64 evaluations of the same formulas, so they agree to summation order: the largest deviation measured
over all cases is 8.6e-10 for the gradients (per image: max-norm of the difference over max-norm of the reference's
gradient), 4.5e-12 for the final state and 3.3e-14 for the Jacobian.  The gates are 100 x those: summation
order cannot fail them, a formula error does (a wrong Huber branch moves a gradient by 1e-2).

The frozen-column plans with a distortion model (tests/golden/lm_grad_frozen_reference.npz, written by
tests/golden/make_golden_lm_grad_frozen.py: simple_radial with prior_focal, prior_gravity and both) run at the same gates:
measured 2.7e-9, 7.7e-11 and 4.8e-11 for the gradients, 5.7e-12 for the final state."""
import os

import numpy as np
import pytest
import torch

from geocalib_amd import lm_grad
from geocalib_amd.camera import camera_models
from geocalib_amd.gravity import Gravity

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GRAD_GATE, STATE_GATE, JAC_GATE = 8.6e-8, 4.5e-10, 3.3e-12
INPUTS = ("up_field", "latitude_field", "up_confidence", "latitude_confidence")


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "lm_grad_reference.npz"))


def case_names(ref):
    return sorted({k.rsplit("/w_cam", 1)[0] for k in ref.files if k.endswith("/w_cam")})


def case_conf(ref, name):
    steps, scale = ref[f"{name}/cfg"]
    squared = scale > 1.0
    conf = {"camera_model": name.split("/")[1], "num_steps": int(steps), "early_stop": False,
            "loss_fn": "squared_loss" if squared else "huber_loss"}
    if not squared:
        conf.update(up_loss_fn_scale=float(scale), lat_loss_fn_scale=float(scale))
    return conf


def case_data(ref, name, dtype=torch.float64, device="cpu", requires_grad=True):
    data = {}
    for k in ref.files:
        if k.startswith(f"{name}/in/"):
            t = torch.from_numpy(ref[k]).to(device=device, dtype=dtype)
            key = k.rsplit("/", 1)[1]
            data[key] = t.requires_grad_(True) if requires_grad and key in INPUTS else t
    return data


def recorded_loss(ref, name, camera, gravity):
    """L of the fixture on a result: sum w_c[:, 2:4] f / height + sum w_g gravity (+ sum w_c[:, 6] k1)."""
    cam, grav = camera._data, gravity._data
    wc, wg = (torch.from_numpy(ref[f"{name}/{k}"]).to(cam) for k in ("w_cam", "w_grav"))
    loss = (cam[:, 2:4] / cam[:, 1:2] * wc[:, 2:4]).sum() + (grav * wg).sum()
    if hasattr(camera, "dist"):
        loss = loss + (cam[:, 6] * wc[:, 6]).sum()
    return loss


def image_rel_err(got, want):
    dims = tuple(range(1, want.dim()))
    return ((got - want).abs().amax(dim=dims) / want.abs().amax(dim=dims)).max().item()


ALL_CASES = ["c1/pinhole/huber", "c1/pinhole/squared", "c1/simple_radial/huber", "c1/simple_radial/squared",
             "c2/pinhole/huber", "c2/pinhole/squared", "c2/simple_radial/huber", "c2/simple_radial/squared",
             "lat_only/pinhole/huber", "noconf/pinhole/huber", "prior_focal/pinhole/huber", "prior_gravity/pinhole/huber"]


def test_fixture_holds_every_case(ref):
    assert case_names(ref) == sorted(ALL_CASES)


# the frozen-column plans with a distortion model (tests/golden/make_golden_lm_grad_frozen.py): prior_focal is the reference's
# overlap quirk -- without a free focal length the distortion takes the first gravity step
FROZEN_CASES = ["prior_focal/simple_radial/huber", "prior_gravity/simple_radial/huber", "prior_focal_gravity/simple_radial/huber"]


@pytest.fixture(scope="module")
def ref_frozen():
    return np.load(os.path.join(GOLDEN, "lm_grad_frozen_reference.npz"))


def test_frozen_fixture_holds_every_case(ref_frozen):
    assert case_names(ref_frozen) == sorted(FROZEN_CASES)
    for name in FROZEN_CASES:
        extra = name.split("/")[0]
        priors = sorted(k.rsplit("/", 1)[1] for k in ref_frozen.files if k.startswith(f"{name}/in/prior_"))
        assert priors == {"prior_focal": ["prior_focal"], "prior_gravity": ["prior_gravity"],
                          "prior_focal_gravity": ["prior_focal", "prior_gravity"]}[extra], (name, priors)
        assert ref_frozen[f"{name}/in/latitude_field"].shape == (3, 1, 12, 20) and int(ref_frozen[f"{name}/cfg"][0]) == 5


@pytest.mark.parametrize("name", ALL_CASES)
def test_unrolled_matches_reference_float64(ref, name):
    unrolled_matches_reference_float64(ref, name)


@pytest.mark.parametrize("name", FROZEN_CASES)
def test_unrolled_matches_reference_float64_frozen_columns(ref_frozen, name):
    unrolled_matches_reference_float64(ref_frozen, name)


def unrolled_matches_reference_float64(ref, name):
    data = case_data(ref, name)
    out = lm_grad.lm_unrolled_torch(data, case_conf(ref, name), dtype=torch.float64)
    # the damping decisions: lambda went up exactly where the reference's new cost exceeded the previous one
    lamb = torch.cat([torch.full_like(out["lambdas"][:1], 0.1), out["lambdas"]])
    went_up = (lamb[1:] > lamb[:-1]).numpy()
    want_up = ref[f"{name}/decisions"]
    at_floor = (lamb[:-1] <= 1e-6).numpy() & ~want_up          # a "down" at the floor leaves lambda where it is
    assert (went_up == want_up)[~at_floor].all() and not went_up[at_floor].any()
    cam_err = np.abs(out["camera"]._data.detach().numpy() - ref[f"{name}/camera64"]).max() / np.abs(ref[f"{name}/camera64"]).max()
    grav_err = np.abs(out["gravity"]._data.detach().numpy() - ref[f"{name}/gravity64"]).max()
    print(f"{name}: final camera {cam_err:.2e} gravity {grav_err:.2e}")
    keys = [k for k in INPUTS if k in data]
    grads = torch.autograd.grad(recorded_loss(ref, name, out["camera"], out["gravity"]), [data[k] for k in keys])
    errs = {k: image_rel_err(g, torch.from_numpy(ref[f"{name}/grad64/{k}"])) for k, g in zip(keys, grads)}
    print(f"{name}: gradient errors {errs}")
    assert cam_err <= STATE_GATE and grav_err <= STATE_GATE
    assert max(errs.values()) <= GRAD_GATE, errs


@pytest.mark.parametrize("model", ["pinhole", "simple_radial", "radial", "simple_divisional"])
def test_forward_mode_jacobian_is_the_reference_jacobian(model):
    g = np.load(os.path.join(GOLDEN, "golden_jac.npz"))
    cam = camera_models[model](torch.from_numpy(g[f"{model}/camera"]))
    grav = Gravity(torch.from_numpy(g[f"{model}/gravity"]))
    J_up, J_lat = (torch.from_numpy(g[f"{model}/loop/{k}"]) for k in ("J_up", "J_lat"))
    B, h, w = J_up.shape[:3]
    _, J = lm_grad.fields_and_jacobian(cam, grav, (h, w))
    want = torch.cat([J_up, J_lat], -2).reshape(B, h * w, 3, -1)
    err = ((J - want).abs().amax() / want.abs().amax()).item()
    print(f"{model}: Jacobian error {err:.2e}")
    assert err <= JAC_GATE


def test_unsupported_configurations_raise():
    data = {"latitude_field": torch.zeros(1, 1, 4, 4)}
    for conf in ({"shared_intrinsics": True}, {"use_spherical_manifold": False}, {"use_log_focal": False},
                 {"init_conf": {"name": "heuristic"}}):
        with pytest.raises(ValueError):
            lm_grad.lm_unrolled_torch(data, conf)
