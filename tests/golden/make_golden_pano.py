"""Generate tests/golden/golden_pano.npz: the REFERENCE's own Camera.get_img_from_pano outputs (CPU, float32).

Run in the build container only (needs the reference checkout; the GPU box does not have it):

    python tests/golden/make_golden_pano.py

Inputs: one 256 x 512 x 3 panorama stored as uint8 (the tests read it as value / 255 in float32), and per model 8 cameras of
24 x 32 with distortion drawn across the model's range, roll / pitch within +-0.5 rad and 8 yaws spread over [-pi, pi).
Outputs per model: the rendering without resize_factor and with one that mixes bicubic (scale >= 1) and area (< 1)."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402

MODELS = ("pinhole", "simple_radial", "radial", "simple_divisional")
DIST = {"pinhole": (0.0, 0.0), "simple_radial": (-0.5, 0.5), "radial": (-0.5, 0.5), "simple_divisional": (-2.0, 2.0)}
N, H, W, HP, WP = 8, 24, 32, 256, 512
RESIZE = [0.2, 0.35, 0.5, 0.8, 1.0, 1.5, 0.3, 2.0]


def inputs(model, seed):
    g = torch.Generator().manual_seed(seed)
    f = (0.5 + 0.7 * torch.rand(N, generator=g)) * W
    lo, hi = DIST[model]
    k1 = lo + (hi - lo) * torch.rand(N, generator=g)
    k2 = (lo + (hi - lo) * torch.rand(N, generator=g)) * (model == "radial")
    cams = torch.stack([torch.full((N,), float(W)), torch.full((N,), float(H)), f, f * 1.02,
                        W / 2 + 2 * torch.rand(N, generator=g) - 1, H / 2 + 2 * torch.rand(N, generator=g) - 1, k1, k2], -1)
    rp = torch.rand(N, 2, generator=g) - 0.5
    yaws = torch.linspace(-math.pi, math.pi, N + 1)[:N] + 0.2 * torch.rand(N, generator=g)
    return cams, rp, yaws


def main():
    ref = ref_import.load()
    g = torch.Generator().manual_seed(2024)
    y = torch.linspace(0, 1, HP)[:, None]
    x = torch.linspace(0, 1, WP)[None, :]
    smooth = torch.stack([torch.sin(6.28 * (3 * x + 2 * y) + c) for c in (0.0, 1.0, 2.0)]) * 0.35 + 0.5
    pano_u8 = (255 * (0.7 * smooth + 0.3 * torch.rand(3, HP, WP, generator=g))).round().clamp(0, 255).to(torch.uint8)
    pano = pano_u8.to(torch.float32) / 255
    out = {"pano_u8": pano_u8.numpy(), "resize": np.array(RESIZE, np.float32)}
    with torch.no_grad():
        for i, model in enumerate(MODELS):
            cams, rp, yaws = inputs(model, 100 + i)
            cam = ref.camera.camera_models[model](cams)
            grav = ref.gravity.Gravity.from_rp(rp[:, 0], rp[:, 1])
            out[f"{model}_cams"], out[f"{model}_rp"], out[f"{model}_yaws"] = cams.numpy(), rp.numpy(), yaws.numpy()
            out[f"{model}_plain"] = cam.get_img_from_pano(pano, grav, yaws).numpy()
            out[f"{model}_resize"] = cam.get_img_from_pano(pano, grav, yaws, torch.tensor(RESIZE)).numpy()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden_pano.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
