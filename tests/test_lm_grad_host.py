"""The host side of the differentiable LM solve, without a GPU: the ValueErrors of what LMOptimizer({"differentiable": True})
does not cover (raised before the library is touched), and LMOptimizer.loss / .metrics against the values the reference's
training-time optimiser gives (tests/golden/lm_grad_reference.npz)."""
import os

import numpy as np
import pytest
import torch

from geocalib_amd import LMOptimizer, _lib
from geocalib_amd.camera import camera_models
from geocalib_amd.gravity import Gravity

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "lm_grad_reference.npz"))


def fields(dtype=torch.float32):
    return {"up_field": torch.zeros(2, 2, 6, 8, dtype=dtype), "latitude_field": torch.zeros(2, 1, 6, 8, dtype=dtype)}


@pytest.mark.parametrize("conf, data, limit", [
    ({"camera_model": "radial"}, {}, "camera models"),
    ({"camera_model": "simple_divisional"}, {}, "camera models"),
    ({"shared_intrinsics": True}, {}, "shared_intrinsics"),
    ({"init_conf": {"name": "ransac"}}, {}, "init_conf"),
    ({"use_spherical_manifold": False}, {}, "use_spherical_manifold"),
    ({"use_log_focal": False}, {}, "use_log_focal"),
    ({"num_steps": 0}, {}, "num_steps"),
    ({"verbose": True}, {}, "verbose"),
    ({}, {"sin_latitude": torch.zeros(2, 1, 6, 8)}, "sin_latitude"),
    ({}, fields(torch.float64), "float32"),
    ({}, fields(), "HIP device"),
])
def test_unsupported_combinations_raise_before_the_library_is_touched(monkeypatch, conf, data, limit):
    def touched(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", touched)
    opt = LMOptimizer({"differentiable": True, **conf}).train()
    with pytest.raises(ValueError, match=limit):
        opt({**fields(), **data})


def test_differentiable_is_off_by_default():
    assert LMOptimizer.default_conf["differentiable"] is False and LMOptimizer.default_conf["loss_weight"] == 1.0


@pytest.mark.parametrize("name", ["c1/pinhole/huber", "c1/simple_radial/huber"])
@pytest.mark.parametrize("weight", [1.0, 0.5])
def test_loss_and_metrics_match_the_reference(ref, name, weight):
    model = name.split("/")[1]
    opt = LMOptimizer({"camera_model": model, "loss_weight": weight})
    cam = camera_models[model](torch.from_numpy(ref[f"{name}/camera32"]))
    grav = Gravity(torch.from_numpy(ref[f"{name}/gravity32"]))
    pred = {"camera": cam, "gravity": grav}
    prefix = f"{name}/metrics/"
    for k in ref.files:
        if k.startswith(prefix) and ("initial" in k or "final" in k or k.endswith("stop_at")):
            pred[k[len(prefix):]] = torch.from_numpy(ref[k])
    data = {"camera": camera_models[model](torch.from_numpy(ref[f"{name}/gt_camera"]).float()),
            "gravity": Gravity(torch.from_numpy(ref[f"{name}/gt_gravity"]).float())}
    losses, metrics = opt.loss(pred, data)
    assert sorted(losses) == ["dist", "focal", "gravity", "param_total"]
    for k, v in losses.items():
        np.testing.assert_allclose(v.numpy(), ref[f"{name}/loss{weight}/{k}"], rtol=2e-6, atol=1e-9, err_msg=k)
    want = sorted(k[len(prefix):] for k in ref.files if k.startswith(prefix))
    assert sorted(metrics) == want
    for k in want:
        # float32 on both sides; the angle errors go through asin / acos of rounded values: a few float32 ulps of a degree
        np.testing.assert_allclose(np.asarray(metrics[k]), ref[prefix + k], rtol=2e-5, atol=2e-5, err_msg=k)
