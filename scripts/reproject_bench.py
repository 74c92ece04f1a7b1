"""GPU: Camera.reproject_image on the HIP path (gclm_reproject_image) against what it replaces.

Per (source model, rotation, B) on the same device tensors, at 1080 x 1920, C = 3 by default:
  hip_kernel        one gclm_reproject_image launch into a preallocated destination, no mask (kernel + launch)
  hip_kernel_mask   the same with the (B, H, W) uint8 mask written
  hip_method        the public method (allocates its output, reads the two cameras' sizes from the device once)
  torch_path        the full torch composition of the same definition (camera._reproject_torch)
  grid_sample       F.grid_sample alone on a precomputed grid: the floor of any torch path
  undistort_kernel  identity rotation only: one gclm_undistort_image launch at the same shapes
Rotations: "identity" (NULL, to the source's pinhole), "roll25" (a 25 deg roll removed), "level" ((-40, 30) deg levelled).
Times are hipEvent means over --steps calls after --warmup; TBps counts the algorithmic traffic, one read and one write of the
image (2 x 4 B C H W bytes), over that time.  max_abs_diff is the kernel's output against the torch composition's.

    python scripts/reproject_bench.py [--shape 1080x1920] [--batches 1,16,64] [--models pinhole,simple_radial,simple_divisional]
                                      [--run 1]
Prints one JSON line per (model, rotation, B, path); profiles/reproject_bench.jsonl holds two calls (--run 1, --run 2)."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from torch.nn import functional as F  # noqa: E402

from geocalib_amd import Gravity, _lib, camera as camera_module, camera_models  # noqa: E402
from geocalib_amd._call import raw_stream as _raw_stream  # noqa: E402

K1 = {"simple_radial": -0.2, "radial": -0.2, "simple_divisional": -0.8, "pinhole": 0.0}


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


def rotation(kind, dev):
    if kind == "identity":
        return None
    roll, pitch, level = (25.0, 0.0, False) if kind == "roll25" else (-40.0, 30.0, True)
    g = Gravity.from_rp(torch.tensor([math.radians(roll)]), torch.tensor([math.radians(pitch)]))
    R_t = Gravity.from_rp(torch.zeros(1), torch.zeros(1) if level else g.pitch).R
    return (R_t @ g.R.transpose(-1, -2)).to(dev).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1080x1920", help="HxW")
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--models", default="pinhole,simple_radial,simple_divisional")
    ap.add_argument("--rotations", default="identity,roll25,level")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--torch-steps", type=int, default=5)
    ap.add_argument("--run", type=int, default=1, help="a label for the lines of this call (the spread is taken between calls)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("reproject_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    H, W = (int(v) for v in args.shape.split("x"))
    C = args.channels
    for model in args.models.split(","):
        data = torch.tensor([[W, H, 0.8 * W, 0.81 * W, W / 2 + 3.3, H / 2 - 2.1, K1[model], 0.0]], device=dev)
        pin = torch.cat([data[:, :6], torch.zeros_like(data[:, 6:])], -1)
        cam, mid = camera_models[model](data), _lib.CAMERA_MODEL_IDS[model]
        for B in (int(b) for b in args.batches.split(",")):
            img = torch.rand(B, C, H, W, device=dev)
            dst = torch.empty_like(img)
            mask = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
            nbytes = 2 * 4 * B * C * H * W
            for kind in args.rotations.split(","):
                rot = rotation(kind, dev)

                def kernel(valid=None):
                    rc = lib.gclm_reproject_image(mid, data.data_ptr(), 0, pin.data_ptr(), 1, None if rot is None else rot.data_ptr(),
                                                  1, img.data_ptr(), B, C, H, W, H, W, H, W, dst.data_ptr(), valid, _raw_stream(dev))
                    assert rc == 0, rc

                def torch_path():
                    return camera_module._reproject_torch(model, data, "pinhole", pin, rot, img, (H, W), (H, W))[0]

                rows = [("hip_kernel", timed(kernel, args.steps, args.warmup)),
                        ("hip_kernel_mask", timed(lambda: kernel(mask.data_ptr()), args.steps, args.warmup)),
                        ("hip_method", timed(lambda: cam.reproject_image(img, rotation=rot), args.steps, args.warmup)),
                        ("torch_path", timed(torch_path, args.torch_steps, 1))]
                kernel()
                ref = torch_path()
                diff = (dst - ref).abs().max().item()
                del ref
                grid = camera_module._reproject_grid(model, data, "pinhole", pin, rot, img.shape, (H, W), (H, W))[0].contiguous()
                rows.append(("grid_sample", timed(lambda: F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros",
                                                                        align_corners=True), args.torch_steps, 1)))
                del grid
                if kind == "identity":
                    def undistort():
                        rc = lib.gclm_undistort_image(mid, data.data_ptr(), 1, img.data_ptr(), B, C, H, W, H, W, dst.data_ptr(),
                                                      _raw_stream(dev))
                        assert rc == 0, rc
                    rows.append(("undistort_kernel", timed(undistort, args.steps, args.warmup)))
                for path, t in rows:
                    print(json.dumps({"run": args.run, "model": model, "rotation": kind, "B": B, "C": C, "H": H, "W": W, "path": path,
                                      "ms": round(t * 1e3, 4), "TBps": round(nbytes / t / 1e12, 3), "max_abs_diff_vs_torch": diff}),
                          flush=True)
            del img, dst, mask
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
