"""GPU: Camera.undistort_image on the HIP path (gclm_undistort_image) against the torch composition it replaces.

The torch side is the reference's composition at its best: the sampling grid is built ONCE per camera, outside the timed
window, and only F.grid_sample(bilinear, zeros, align_corners=True) of the whole batch is timed.  The HIP side is one
gclm_undistort_image launch into a preallocated destination (kernel + launch), and the public method (which also allocates
its output).  Times are hipEvent means over --steps calls after --warmup; effective bytes per second count the minimum
traffic, the source read once and the destination written once: 4 C (Hin Win + H W) B bytes.

    python scripts/undistort_bench.py [--batches 1,16,64] [--models simple_radial,simple_divisional] [--steps 50]
Prints one JSON line per (model, B, path).  Run once per library (GCLM_LIB_PATH) to compare builds in one session."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from torch.nn import functional as F  # noqa: E402

from geocalib_amd import _lib, camera_models  # noqa: E402
from geocalib_amd._call import raw_stream as _raw_stream  # noqa: E402

K1 = {"simple_radial": -0.3, "radial": -0.3, "simple_divisional": -0.8, "pinhole": 0.0}


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps * 1e-3      # seconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--models", default="simple_radial,simple_divisional")
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("undistort_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    H, W, C = args.height, args.width, args.channels
    lib = _lib.load()
    for model in args.models.split(","):
        data = torch.tensor([[W, H, 0.8 * W, 0.8 * W, W / 2 + 3.3, H / 2 - 2.1, K1[model], 0.0]], device=dev)
        cam = camera_models[model](data)
        for B in (int(b) for b in args.batches.split(",")):
            img = torch.rand(B, C, H, W, device=dev)
            dst = torch.empty_like(img)
            nbytes = 4 * C * (H * W + H * W) * B
            mid = _lib.CAMERA_MODEL_IDS[model]

            def kernel():
                rc = lib.gclm_undistort_image(mid, data.data_ptr(), 1, img.data_ptr(), B, C, H, W, H, W, dst.data_ptr(),
                                              _raw_stream(dev))
                assert rc == 0, rc

            rows = [("hip_kernel", timed(kernel, args.steps, args.warmup)),
                    ("hip_method", timed(lambda: cam.undistort_image(img), args.steps, args.warmup))]
            if not args.skip_torch:
                x, y = torch.meshgrid(torch.arange(0, W), torch.arange(0, H), indexing="xy")
                coords = torch.stack((x, y), dim=-1).reshape(-1, 2).to(dev, torch.float32)
                p2d, _ = cam.world2image(cam.pinhole().image2world(coords)[0])
                grid = 2.0 * p2d.reshape(1, H, W, 2) / torch.tensor([W - 1, H - 1], device=dev) - 1
                gridB = grid.expand(B, -1, -1, -1)
                rows.append(("torch_grid_sample", timed(lambda: F.grid_sample(img, gridB, align_corners=True),
                                                        args.steps, args.warmup)))
                diff = (F.grid_sample(img, gridB, align_corners=True) - cam.undistort_image(img)).abs().max().item()
            else:
                diff = None
            for path, t in rows:
                print(json.dumps({"model": model, "B": B, "C": C, "H": H, "W": W, "path": path, "ms": round(t * 1e3, 4),
                                  "TBps": round(nbytes / t / 1e12, 3), "max_abs_diff_vs_torch": diff,
                                  "lib": os.path.basename(_lib.LIB_PATH)}), flush=True)
            del img, dst


if __name__ == "__main__":
    main()
