"""Writes tests/golden/lm_grad_frozen_reference.npz: the frozen-column plans of the reference's LM optimiser with a
distortion model, by the recipe, the conditions and the replacement rule of make_golden_lm_grad.py (its `make`, `run` and
`record_case`, unchanged).  Data only: inputs, priors, weights, both precisions' gradients, decisions, states.

Cases, simple_radial, huber at scale 1e-2, B = 3, 12 x 20, 5 steps:
    prior_focal          gravity and k1 free.  The reference's overlap quirk: without a free focal length its distortion step
                         reads the FIRST gravity column of delta (geocalib/lm_optimizer.py: focal_delta_dims = (-1,), so
                         dist_delta_dims starts at 0), while the system's columns stay (d1, d2, k1);
    prior_gravity        focal length and k1 free (columns 0 and 1 of the step);
    prior_focal_gravity  k1 alone.

lm_grad_reference.npz is not touched.

    python tests/golden/make_golden_lm_grad_frozen.py
"""
import os

import numpy as np

import make_golden_lm_grad as base

CASES = ("prior_focal", "prior_gravity", "prior_focal_gravity")


def cases():
    cfg = dict(model="simple_radial", scale=base.HUBER, B=3, H=12, W=20, steps=5)
    return [(f"{extra}/simple_radial/huber", dict(cfg, extra=extra)) for extra in CASES]


def main():
    ns = base.ref_import.load()
    rec = {}
    for name, cfg in cases():
        base.record_case(ns, rec, name, cfg)
        print(f"{name}: seed {int(rec[f'{name}/seed'])}, {int(rec[f'{name}/cfg'][0])} steps, final k1 "
              f"{rec[f'{name}/camera64'][:, 6].tolist()} (ground truth {rec[f'{name}/gt_camera'][:, 6].tolist()})")
    out = os.path.join(base.HERE, "lm_grad_frozen_reference.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes,", len(rec), "arrays")


if __name__ == "__main__":
    main()
