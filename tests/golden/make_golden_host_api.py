"""Goldens of the reference's host-side API for tests/test_host_api.py (run in the build container only):

    python tests/golden/make_golden_host_api.py      ->  tests/golden/golden_host_api.npz

The inputs are the test's own (test_host_api.make in float32, seeded points, seeded LM-loop inputs); the reference's
Camera / Gravity / perspective-field methods (test_host_api.api_outputs, one definition for both sides; in float32 and,
on the same inputs, in float64), its skew_symmetric / pitch2rho, and its update_lambda / early_stop / update_estimate
run on them.  Inputs and outputs are stored together: the test feeds the stored inputs to geocalib_amd and compares with
the stored outputs."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_import  # noqa: E402
from test_host_api import MODELS, api_outputs, loop_priors, make  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ref = ref_import.load()
    out = {}

    def put(key, t):
        out[key] = np.asarray(t.detach().numpy() if torch.is_tensor(t) else t).copy()

    # ---- test_small_utils
    v = torch.tensor([[0.3, -1.2, 2.0], [1.0, 0.5, -0.7]], dtype=torch.float64)
    pitch, f, h = torch.tensor([0.3, -0.5]), torch.tensor([500.0, 320.0]), torch.tensor([480.0, 480.0])
    for k, x in (("v", v), ("pitch", pitch), ("f", f), ("h", h)):
        put(f"utils/{k}", x)
    put("utils/skew_symmetric", ref.utils.skew_symmetric(v))
    put("utils/pitch2rho", ref.utils.pitch2rho(pitch, f, h))

    # ---- test_reference_api_comparison
    for model in MODELS:
        cam, grav = make(model, dtype=torch.float32)
        pts = torch.rand(3, 30, 2, generator=torch.Generator().manual_seed(2)) - 0.5
        put(f"api/{model}/camera", cam._data)
        put(f"api/{model}/gravity", grav._data)
        put(f"api/{model}/pts", pts)
        rc, rg = ref.camera.camera_models[model](cam._data.clone()), ref.gravity.Gravity(grav._data.clone())
        for name, t in api_outputs(model, rc, rg, ref.perspective_fields.get_perspective_field, pts).items():
            put(f"api/{model}/out/{name}", t)
        # the same float32 inputs evaluated in float64: the formulas without their float32 rounding
        rc, rg = ref.camera.camera_models[model](cam._data.double()), ref.gravity.Gravity(grav._data.double())
        for name, t in api_outputs(model, rc, rg, ref.perspective_fields.get_perspective_field, pts.double()).items():
            put(f"api/{model}/out64/{name}", t)

    # ---- test_loop_rules_against_the_reference
    gen = torch.Generator().manual_seed(8)
    prev, new, lamb = torch.rand(6, generator=gen), torch.rand(6, generator=gen), torch.rand(6, generator=gen) * 50
    put("loop/prev", prev)
    put("loop/new", new)
    put("loop/lamb", lamb)
    put("loop/update_lambda", ref.lm_optimizer.update_lambda(lamb, prev, new))
    put("loop/early_stop", [bool(ref.lm_optimizer.early_stop(a, b, 1e-8, 1e-8)) for a, b in ((new, prev), (prev, prev + 1e-10))])
    for model in MODELS:
        cam, grav = make(model, dtype=torch.float32)
        rc, rg = ref.camera.camera_models[model](cam._data.clone()), ref.gravity.Gravity(grav._data.clone())
        for j, data in enumerate(loop_priors(model)):
            theirs = ref.lm_optimizer.LMOptimizer({"camera_model": model})
            theirs.setup_optimization_and_priors(data, shared_intrinsics=False)
            n = 2 * theirs.estimate_gravity + theirs.estimate_focal + (cam.num_dist_params() if theirs.estimate_dist else 0)
            delta = (torch.rand(3, n, generator=gen) - 0.5) * 0.2
            c2, g2 = theirs.update_estimate(rc, rg, delta)
            put(f"loop/{model}/{j}/delta", delta)
            put(f"loop/{model}/{j}/camera", c2._data)
            put(f"loop/{model}/{j}/gravity", g2._data)

    np.savez_compressed(os.path.join(HERE, "golden_host_api.npz"), **out)
    print(f"{len(out)} arrays, {sum(a.nbytes for a in out.values())} bytes")


if __name__ == "__main__":
    main()
