"""Writes tests/golden/soft_priors_yardstick.npz: the float64 and the float32 run of lm_grad.lm_unrolled_torch on the 32 parity
cases of tests/test_soft_priors.py.  Data only; nothing but this package is needed.

Per case `<model>/<H>x<W>/<kind>/<loss>`: the seed, the damping after every step's rule in both precisions, and the final state
[fy, gx, gy, gz, k1] of both runs.  The seed of a case is the first, from 11 on, at which both runs take the same damping
decision at every step (the condition of tests/golden/make_golden_lm_grad.py).  A float32 run of torch on the CPU depends on the
machine's summation order, and under the squared loss the last decisions compare costs that differ by less than float32
resolves, so the float32 run is RECORDED here, where the seeds were chosen, and not run again by the test: its distance from
the float64 run is the unit of the test's gate.

    python tests/golden/make_golden_soft_priors.py
"""
import itertools
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from geocalib_amd import lm_grad  # noqa: E402
from soft_prior_cases import KINDS, conf_for, free_sigmas, make, packed, state_error, with_priors  # noqa: E402

B = 3


def main():
    rec = {}
    for model, (H, W), kind, loss in itertools.product(("pinhole", "simple_radial"), ((13, 19), (67, 65)), KINDS, ("huber", "squared")):
        conf = conf_for(model, loss)
        for seed in range(11, 200):
            data, priors, _, _ = make(model, B, H, W, seed)
            d = with_priors(data, priors, kind, *free_sigmas(data, conf))
            y64 = lm_grad.lm_unrolled_torch(d, conf, dtype=torch.float64)
            y32 = lm_grad.lm_unrolled_torch(d, conf, dtype=torch.float32)
            if torch.allclose(y64["lambdas"].float(), y32["lambdas"], rtol=1e-4, atol=0):
                break
        else:
            raise SystemExit(f"{model} {H}x{W} {kind} {loss}: no seed met the condition")
        name = f"{model}/{H}x{W}/{kind}/{loss}"
        rec[f"{name}/seed"] = np.array(seed)
        rec[f"{name}/lambdas64"], rec[f"{name}/lambdas32"] = y64["lambdas"].numpy(), y32["lambdas"].numpy()
        rec[f"{name}/state64"], rec[f"{name}/state32"] = packed(y64), packed(y32)
        print(f"{name:48s} seed {seed:3d}  float32 against float64 {state_error(y32, y64):.2e}")
    out = os.path.join(HERE, "soft_priors_yardstick.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes,", len(rec), "arrays")


if __name__ == "__main__":
    main()
