"""GPU: get_perspective_field on the HIP path (gclm_perspective_fields) against the torch composition it replaces.

Four timings on the same device tensors: one gclm_perspective_fields launch into preallocated outputs (kernel + launch), the
public get_perspective_field (which also allocates its outputs and reads the camera size once), today's torch path (up and
latitude compositions, float32, same cameras), and `zero_()` of one buffer that holds both outputs -- a same-process store
ceiling for the 12 bytes per pixel the kernel writes.  Times are hipEvent means over --steps calls after --warmup.

    python scripts/perspective_bench.py [--shapes 480x640:1,480x640:64,480x640:1024,1080x1920:1]
                                        [--models pinhole,simple_divisional] [--steps 50]
Prints one JSON line per (model, shape, B, path).  Run once per library (GCLM_LIB_PATH) to compare builds in one session."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from geocalib_amd import Gravity, _lib, camera_models, perspective_fields as pf  # noqa: E402
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
    ap.add_argument("--shapes", default="480x640:1,480x640:64,480x640:1024,1080x1920:1", help="HxW:B,...")
    ap.add_argument("--models", default="pinhole,simple_divisional")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--torch-steps", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perspective_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    g = torch.Generator().manual_seed(0)
    for model in args.models.split(","):
        for spec in args.shapes.split(","):
            hw, B = spec.split(":")
            H, W = (int(v) for v in hw.split("x"))
            B = int(B)
            f = 0.8 * W * (1 + 0.2 * torch.rand(B, generator=g))
            data = torch.stack([torch.full((B,), float(W)), torch.full((B,), float(H)), f, f * 1.01,
                                W / 2 + 3.3 + torch.zeros(B), H / 2 - 2.1 + torch.zeros(B), torch.full((B,), K1[model]),
                                torch.zeros(B)], -1).to(dev)
            cam = camera_models[model](data)
            roll, pitch = (torch.rand(B, generator=g) - 0.5), (torch.rand(B, generator=g) - 0.5)
            grav = Gravity.from_rp(roll, pitch).to(dev)
            gd = grav._data.contiguous()
            buf = torch.empty(3 * B * H * W, device=dev)
            up, lat = buf[:2 * B * H * W], buf[2 * B * H * W:]
            mid = _lib.CAMERA_MODEL_IDS[model]
            nbytes = 12 * B * H * W

            def kernel():
                rc = lib.gclm_perspective_fields(mid, data.data_ptr(), gd.data_ptr(), B, H, W, 1, up.data_ptr(), lat.data_ptr(),
                                                 _raw_stream(dev))
                assert rc == 0, rc

            rows = [("hip_kernel", timed(kernel, args.steps, args.warmup)),
                    ("hip_method", timed(lambda: pf.get_perspective_field(cam, grav), args.steps, args.warmup)),
                    ("zero_ceiling", timed(buf.zero_, args.steps, args.warmup))]
            diff = None
            if not args.skip_torch:
                def torch_path():
                    return (pf._up_field_torch(cam, grav, H, W, True), pf._latitude_field_torch(cam, grav, H, W))

                rows.append(("torch_path", timed(torch_path, args.torch_steps, 1)))
                kernel()
                tu, tl = torch_path()
                diff = max((up.view(B, H, W, 2) - tu).abs().max().item(), (lat.view(B, H, W, 1) - tl).abs().max().item())
                del tu, tl
            for path, t in rows:
                print(json.dumps({"model": model, "B": B, "H": H, "W": W, "path": path, "ms": round(t * 1e3, 4),
                                  "TBps": round(nbytes / t / 1e12, 3), "max_abs_diff_vs_torch": diff,
                                  "lib": os.path.basename(_lib.LIB_PATH)}), flush=True)
            del buf, up, lat
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
