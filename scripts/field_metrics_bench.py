"""GPU: metrics.perspective_field_metrics on the HIP path (gclm_field_errors) against the composition it replaces.

Timings on the same device tensors, hipEvent means over --steps calls after --warmup, one timed region per row:
    hip_kernel        gclm_field_errors into preallocated statistics and workspace: both fields, both confidences, no maps
    hip_kernel_noconf ... without the confidences          hip_kernel_maps   ... with both per-pixel error maps
    hip_method        the public perspective_field_metrics (allocates its outputs and the workspace)
    baseline          what a caller composes without the kernel: the HIP get_perspective_field, then the torch metrics as the
                      reference writes them (metrics._field_metrics_torch)
    variant_kernel    hip_kernel of a second build of the library (--variant-lib: e.g. one made with
                      -DGCLM_METRICS_MAX_PX=2, two pixels per lane at most), in the same process on the same tensors
TBps is bytes READ (20 B per pixel with both confidences, 12 without) over time, to set against the 8 TB/s peak.

    python scripts/field_metrics_bench.py [--shapes 480x640:1024,480x640:16] [--models pinhole,simple_divisional]
                                          [--steps 30] [--variant-lib PATH]
Prints one JSON line per (model, shape, B, path)."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from geocalib_amd import Gravity, _lib, camera_models, metrics, perspective_fields as pf  # noqa: E402
from geocalib_amd._call import raw_stream as _raw_stream  # noqa: E402

K1 = {"simple_radial": -0.3, "radial": -0.3, "simple_divisional": -0.8, "pinhole": 0.0}
THRESHOLDS = (1, 3, 5, 10)


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


def bind(path):
    """A second build of the library, bound like the first (for --variant-lib)."""
    lib = ctypes.CDLL(path)
    for name in ("gclm_field_errors", "gclm_field_errors_workspace"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._SIGNATURES[name]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="480x640:1024,480x640:16", help="HxW:B,...")
    ap.add_argument("--models", default="pinhole,simple_divisional")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--baseline-steps", type=int, default=3)
    ap.add_argument("--variant-lib", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("field_metrics_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    variant = bind(args.variant_lib) if args.variant_lib else None
    g = torch.Generator().manual_seed(0)
    thr = (ctypes.c_float * len(THRESHOLDS))(*(float(t) for t in THRESHOLDS))
    for model in args.models.split(","):
        for spec in args.shapes.split(","):
            hw, B = spec.split(":")
            H, W = (int(v) for v in hw.split("x"))
            B = int(B)
            f = 0.8 * W * (1 + 0.2 * torch.rand(B, generator=g))
            data = torch.stack([torch.full((B,), float(W)), torch.full((B,), float(H)), f, f * 1.01,
                                W / 2 + 3.3 + torch.zeros(B), H / 2 - 2.1 + torch.zeros(B), torch.full((B,), K1[model]),
                                torch.zeros(B)], -1).to(dev)
            roll, pitch = (torch.rand(B, generator=g) - 0.5), (torch.rand(B, generator=g) - 0.5)
            cam, grav = camera_models[model](data), Gravity.from_rp(roll, pitch).to(dev)
            # predictions: the fields of a calibration 3 degrees and 5 % off
            moved = data.clone()
            moved[:, 2:4] *= 1.05
            up, lat = pf.get_perspective_field(camera_models[model](moved), Gravity.from_rp(roll + 0.05, pitch - 0.05).to(dev))
            pred = {"up_field": up.contiguous(), "latitude_field": lat.contiguous(),
                    "up_confidence": torch.rand(B, H, W, device=dev), "latitude_confidence": torch.rand(B, H, W, device=dev)}
            del up, lat
            gd = grav._data.contiguous()
            ws_bytes = lib.gclm_field_errors_workspace(B, H, W, len(THRESHOLDS))
            ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
            stats = torch.empty(B, 2 * (2 + len(THRESHOLDS)), device=dev)
            maps = torch.empty(2, B, H, W, device=dev)
            mid, p = _lib.CAMERA_MODEL_IDS[model], {k: v.data_ptr() for k, v in pred.items()}

            def kernel(which=lib, conf=True, with_maps=False):
                rc = which.gclm_field_errors(mid, data.data_ptr(), gd.data_ptr(), B, H, W, p["up_field"], p["latitude_field"],
                                             p["up_confidence"] if conf else None, p["latitude_confidence"] if conf else None,
                                             len(THRESHOLDS), thr, ws.data_ptr(), ws_bytes, stats.data_ptr(),
                                             maps[0].data_ptr() if with_maps else None, maps[1].data_ptr() if with_maps else None,
                                             _raw_stream(dev))
                assert rc == 0, rc

            px = B * H * W
            rows = [("hip_kernel", timed(kernel, args.steps, args.warmup), 20 * px),
                    ("hip_kernel_noconf", timed(lambda: kernel(conf=False), args.steps, args.warmup), 12 * px),
                    ("hip_kernel_maps", timed(lambda: kernel(with_maps=True), args.steps, args.warmup), 20 * px),
                    ("hip_method", timed(lambda: metrics.perspective_field_metrics(pred, cam, grav), args.steps, args.warmup), 20 * px)]
            if variant is not None:
                rows.append(("variant_kernel", timed(lambda: kernel(variant), args.steps, args.warmup), 20 * px))
                rows.append(("hip_kernel_again", timed(kernel, args.steps, args.warmup), 20 * px))
            base = timed(lambda: metrics._field_metrics_torch(pred, cam, grav, list(THRESHOLDS), False), args.baseline_steps, 1)
            rows.append(("baseline", base, 20 * px))
            hip = metrics.perspective_field_metrics(pred, cam, grav)
            ref = metrics._field_metrics_torch(pred, cam, grav, list(THRESHOLDS), False)
            diff = max((hip[k] - ref[k]).abs().max().item() for k in hip)
            for path, t, nbytes in rows:
                print(json.dumps({"model": model, "B": B, "H": H, "W": W, "path": path, "ms": round(t * 1e3, 4),
                                  "read_TBps": round(nbytes / t / 1e12, 3), "of_8TBps_peak": round(nbytes / t / 8e12, 3),
                                  "baseline_over_this": round(base / t, 2), "max_abs_diff_vs_baseline": diff,
                                  "lib": os.path.basename(args.variant_lib if path == "variant_kernel" else _lib.LIB_PATH)}),
                      flush=True)
            del pred, ws, stats, maps
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
