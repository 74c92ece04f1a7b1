"""Writes tests/golden/field_loss_reference.npz: what the reference's UpDecoder.calculate_losses and
LatitudeDecoder.calculate_losses (siclib/models/decoders/up_decoder.py, latitude_decoder.py) return on recorded inputs, and what
autograd makes of them.  Data only: float32 predictions, targets and confidences of 3 x 12 x 20 pixels whose residuals span
1e-4 .. 0.3 across the columns (Huber and Cauchy see both regimes), and for every loss type and each of three modes -- a
confidence with use_uncertainty_loss on ("conf_on"), with it off ("conf_off"), no confidence ("noconf") -- the reference's
float32 losses (3,) and the gradient of sum(GOUT * loss) with respect to the predictions.  The gradients of "conf_off" are
recorded as one flag per loss type: whether they equal those of "noconf" bit for bit (they do: the reference ignores the
confidence then).

Runs where a checkout of the reference is available (oracle/ref_import.py says where); the test that reads the file,
tests/test_field_loss_abi.py, does not need one.  The decoders' modules pull in omegaconf and friends at import time; the two
functions touch none of them, so placeholder modules stand in where they are missing.

    python tests/golden/make_golden_field_loss.py
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

B, H, W, SEED = 3, 12, 20, 31
GOUT = (0.5, -2.0, 1.25)
TYPES = {"up": ("l1", "l2", "dot", "cauchy", "huber"), "latitude": ("l1", "l2", "cauchy", "huber")}
MODES = ("conf_on", "conf_off", "noconf")


def reference_decoders():
    ref_import.load()
    for name in ("omegaconf", "h5py", "hydra", "hydra.utils", "albumentations", "albumentations.pytorch",
                 "albumentations.pytorch.transforms"):
        if name not in sys.modules:
            try:
                importlib.import_module(name)
            except Exception:
                sys.modules[name] = ref_import._Anything(name)
    up = importlib.import_module("siclib.models.decoders.up_decoder")
    lat = importlib.import_module("siclib.models.decoders.latitude_decoder")
    return {"up": up.UpDecoder.calculate_losses, "latitude": lat.LatitudeDecoder.calculate_losses}


def inputs():
    """Recorded inputs, float32: targets (unit up vectors, latitudes in +-1.2), predictions = targets + residuals of magnitude
    1e-4 .. 0.3 (log-spaced over the columns, random signs and a random factor in 0.5 .. 1), confidences in 0.01 .. 0.99."""
    g = torch.Generator().manual_seed(SEED)
    rand = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)  # noqa: E731
    ang = rand(B, H, W) * 2 * np.pi
    t = {"up": torch.stack([torch.cos(ang), torch.sin(ang)], 1), "latitude": (rand(B, 1, H, W) - 0.5) * 2.4}
    mag = torch.logspace(-4, np.log10(0.3), W, dtype=torch.float64)
    out = {}
    for k, C in (("up", 2), ("latitude", 1)):
        res = mag * (0.5 + 0.5 * rand(B, C, H, W)) * torch.where(rand(B, C, H, W) < 0.5, -1.0, 1.0)
        out[f"{k}_target"] = t[k].float()
        out[f"{k}_pred"] = (t[k] + res).float()
        out[f"{k}_conf"] = (0.01 + 0.98 * rand(B, H, W)).float()
    return out


def main():
    fns, data = reference_decoders(), inputs()
    rec = {k: v.numpy() for k, v in data.items()}
    rec["grad_output"] = np.array(GOUT, np.float32)
    gout = torch.tensor(GOUT)
    for field, kinds in TYPES.items():
        for kind in kinds:
            grads = {}
            for mode in MODES:
                self = types.SimpleNamespace(loss_type=kind, use_uncertainty_loss=mode == "conf_on", loss_weight=1.0,
                                             conf=types.SimpleNamespace(loss_type=kind))
                pred = data[f"{field}_pred"].clone().requires_grad_(True)
                conf = None if mode == "noconf" else data[f"{field}_conf"]
                loss = fns[field](self, pred, data[f"{field}_target"], conf)[f"{field}-{kind}-loss"]
                assert loss.dtype == torch.float32 and loss.shape == (B,)
                (gout * loss).sum().backward()
                rec[f"{field}/{kind}/{mode}/loss"] = loss.detach().numpy()
                grads[mode] = pred.grad.numpy()
            rec[f"{field}/{kind}/conf_on/grad"], rec[f"{field}/{kind}/noconf/grad"] = grads["conf_on"], grads["noconf"]
            rec[f"{field}/{kind}/conf_off/grad_equals_noconf"] = np.array(grads["conf_off"].tobytes() == grads["noconf"].tobytes())
    out = os.path.join(HERE, "field_loss_reference.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes,", len(rec), "arrays")


if __name__ == "__main__":
    main()
