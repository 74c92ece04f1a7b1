"""Writes tests/golden/rpf_reference.npz: what the reference's minimal solver (siclib/models/optimization/ransac.py:
RPFSolver.solve_rpf) returns on recorded inputs.  Data only: the noisy 64 x 64 fields of three poses (rendered by
tests/rpf_gate.py), 4000 recorded samples per pose, and the reference's (roll, pitch, f) of both roots.

Runs where a checkout of the reference is available (oracle/ref_import.py says where); the test that reads the file,
tests/test_rpf_solver_abi.py, needs neither.  siclib's optimisation package pulls in omegaconf, h5py, hydra and
albumentations at import time; the solver touches none of them, so placeholder modules stand in where they are missing.

    python tests/golden/make_golden_rpf.py
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import ref_import  # noqa: E402
import rpf_gate as rg  # noqa: E402

POSES = ((10, 20, 60), (-35, 40, 90), (5, 3, 40))      # (roll, pitch, vfov): what the reference's roll / pitch can express
H = W = 64
NOISE, N, SEED = 0.02, 4000, 23


def reference_solver():
    ref_import.load()
    for name in ("omegaconf", "h5py", "hydra", "hydra.utils", "albumentations", "albumentations.pytorch",
                 "albumentations.pytorch.transforms"):
        if name not in sys.modules:
            try:
                importlib.import_module(name)
            except Exception:
                sys.modules[name] = ref_import._Anything(name)
    return importlib.import_module("siclib.models.optimization.ransac")


def main():
    ransac = reference_solver()
    data, f, g = rg.render(POSES, H, W, NOISE, seed=SEED)
    gen = torch.Generator().manual_seed(SEED)
    B = len(POSES)
    xs, ys = torch.randint(0, W, (B, N, 3), generator=gen), torch.randint(0, H, (B, N, 3), generator=gen)
    solver = types.SimpleNamespace(solver=ransac.MinimalSolver())
    pp = torch.tensor([H / 2.0, W / 2.0]).expand(B, 2)
    pos, neg = ransac.RPFSolver.solve_rpf(solver, data, xs, ys, pp)
    out = os.path.join(HERE, "rpf_reference.npz")
    np.savez_compressed(out, poses=np.array(POSES, np.float64), noise=NOISE, up_field=data["up_field"].numpy(),
                        latitude_field=data["latitude_field"].numpy(), samples=torch.stack([xs, ys], -1).numpy().astype(np.int16),
                        rpf_pos=pos.numpy().astype(np.float32), rpf_neg=neg.numpy().astype(np.float32))
    print(out, os.path.getsize(out), "bytes; finite rows", int(torch.isfinite(pos).all(-1).sum()), int(torch.isfinite(neg).all(-1).sum()))


if __name__ == "__main__":
    main()
