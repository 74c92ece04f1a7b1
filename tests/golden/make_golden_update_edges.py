"""Goldens of the reference's update at the edge table of tests/update_edges.py (run in the build container only):

    python tests/golden/make_golden_update_edges.py      ->  tests/golden/golden_update_edges.npz

For every (model, form) of the table: the start states, the float64 oracle's step `delta` from them, and the REFERENCE's
own Gravity.roll / pitch / J_rp / update(spherical=True / False), BaseCamera.update_focal(as_log=True / False) and
update_dist at those states and deltas, in float64 (update_edges.class_outputs: one definition for both sides), and
the float32 focal bounds its update_focal clamps to.  Inputs
and outputs are stored together; tests/test_update_edge_oracle.py checks that the stored inputs are still the table's,
feeds them to geocalib_amd's classes and to the oracle's restatement, and compares with the stored outputs."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import lm_oracle, ref_import  # noqa: E402
import update_edges as ue  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ref = ref_import.load()
    lm_oracle.build()
    out = {}
    for model in ue.MODELS:
        for form in ue.FORMS:
            b = ue.batch(model, form)
            delta = ue.oracle_step(lm_oracle, model, form, b)["trace"]["delta"][0]
            pre = f"{model}/{form}/"
            out[pre + "names"] = np.array(b["names"])
            out[pre + "cam0"], out[pre + "grav0"], out[pre + "delta"] = b["cam0"], b["grav0"], delta
            got = ue.class_outputs(model, ref.gravity.Gravity, ref.camera.camera_models[model], b["cam0"], b["grav0"], delta)
            for k, v in got.items():
                out[pre + "out/" + k] = v
    # what the reference's update_focal clamps to in float32, at the table's height and at two others
    import torch
    for h in (ue.H, 231, 480):
        cam = ref.camera.camera_models["pinhole"](torch.tensor([[64.0, h, 50.0, 50.0, 32.0, h / 2, 0.0, 0.0]]))
        out[f"bounds_f32/{h}"] = np.array([cam.update_focal(torch.tensor([[d]]), as_log=True)._data[0, 3].item()
                                           for d in (-20.0, 20.0)], np.float32)
    np.savez_compressed(os.path.join(HERE, "golden_update_edges.npz"), **out)
    print(f"{len(out)} arrays, {sum(a.nbytes for a in out.values())} bytes")


if __name__ == "__main__":
    main()
