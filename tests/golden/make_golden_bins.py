"""Writes tests/golden/bins_reference.npz: what the reference's classification-bin arithmetic
(siclib/models/utils/perspective_encoding.py: encode_up_bin, decode_up_bin, encode_bin_latitude, decode_bin_latitude) returns on
recorded inputs.  Data only, for 73 / 180 bins (the original PerspectiveFields heads) and a tiny 5 / 7 case:

    up_logits, lat_logits       seeded logits (2, Ku, 5, 7) and (2, Kl, 5, 7) with the planted pixels of tests/bins_gate.py
    up_field, latitude          the reference's decodes of their argmax
    planted_up, planted_lat     the planted logit vectors alone, one per kind, with the reference's outputs for them
    enc_up_in, enc_up_bins      up vectors (2, 1, n) -- bin centres, the half-way directions, the wrap, the zero vector, random
                                ones -- and the reference's bins (its float result turned back into the index)
    enc_lat_in, enc_lat_bins    latitudes (n,) -- every class edge, its two float32 neighbours, the ends, random ones -- and bins

Runs where a checkout of the reference is available (oracle/ref_import.py says where); the test that reads the file,
tests/test_pack_bins_abi.py, needs neither.  siclib pulls in omegaconf, h5py, hydra and albumentations at import time; the
arithmetic touches none of them, so placeholder modules stand in where they are missing.

    python tests/golden/make_golden_bins.py
"""
import importlib
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import ref_import  # noqa: E402
import bins_gate as bg  # noqa: E402

CASES = {"": (73, 180, 31), "tiny_": (5, 7, 47)}      # prefix of the keys: (up bins, latitude classes, seed)


def reference_encoding():
    ref_import.load()
    for name in ("omegaconf", "h5py", "hydra", "hydra.utils", "albumentations", "albumentations.pytorch",
                 "albumentations.pytorch.transforms"):
        if name not in sys.modules:
            try:
                importlib.import_module(name)
            except Exception:
                sys.modules[name] = ref_import._Anything(name)
    return importlib.import_module("siclib.models.utils.perspective_encoding")


def encoder_inputs(Ku: int, Kl: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    step = 360 / (Ku - 1)
    k = torch.arange(Ku - 1, dtype=torch.float32)
    deg = torch.cat([k * step - 180, (k + 0.5) * step - 180, torch.rand(64, generator=g) * 360 - 180])
    rad = deg / 180 * math.pi
    vec = torch.stack([torch.cos(rad), torch.sin(rad)])
    special = torch.tensor([[0.0, -1.0, -1.0, 1.0, 0.0, -0.0, 3.0, -1.0], [0.0, 0.0, -0.0, 0.0, 1.0, -2.0, 0.0, -1e-8]])
    vec = torch.cat([vec, special], 1)[:, None, :]                                   # (2, 1, n)
    edges = torch.arange(-90, 90, 180 / Kl)
    e = edges / 180 * math.pi
    lat = torch.cat([e, torch.nextafter(e, torch.full_like(e, 9.0)), torch.nextafter(e, torch.full_like(e, -9.0)),
                     torch.tensor([-math.pi / 2, math.pi / 2, -2.0, 2.0, 0.0]), (torch.rand(64, generator=g) - 0.5) * math.pi])
    return vec.contiguous(), lat.contiguous()


def main():
    pe = reference_encoding()
    out = {"kinds": np.array(bg.KINDS)}
    for prefix, (Ku, Kl, seed) in CASES.items():
        up, lat, where = bg.head_logits(2, Ku, Kl, 5, 7, seed, rounds=2)
        pu, pl = bg.planted(Ku, seed + 1), bg.planted(Kl, seed + 2)
        vec, lats = encoder_inputs(Ku, Kl, seed + 3)
        enc_up = pe.encode_up_bin(vec, Ku)                   # (2, h, w) -> (h, w): deg2rad of the index, a float
        out.update({
            prefix + "up_logits": up.numpy(), prefix + "lat_logits": lat.numpy(),
            prefix + "planted_at": np.array(where, np.int16),
            prefix + "up_field": pe.decode_up_bin(up.argmax(1), Ku).numpy(),
            prefix + "latitude": pe.decode_bin_latitude(lat.argmax(1), Kl).numpy(),
            prefix + "planted_up": pu.numpy(), prefix + "planted_lat": pl.numpy(),
            prefix + "planted_up_field": pe.decode_up_bin(pu[:, :, None, None].argmax(1), Ku).numpy()[:, :, 0, 0],
            prefix + "planted_latitude": pe.decode_bin_latitude(pl.argmax(1), Kl).numpy(),
            prefix + "enc_up_in": vec.numpy(),
            prefix + "enc_up_bins": torch.round(enc_up * 180 / math.pi).to(torch.int16).numpy(),
            prefix + "enc_lat_in": lats.numpy(),
            prefix + "enc_lat_bins": pe.encode_bin_latitude(lats, Kl).to(torch.int16).numpy()})
        assert out[prefix + "up_field"].dtype == np.float32 and out[prefix + "latitude"].dtype == np.float32
    path = os.path.join(HERE, "bins_reference.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
