"""GPU: losses.perspective_field_loss on the HIP path (gclm_field_loss, gclm_field_loss_grad) against what a caller composes
without it, and against the read ceiling.

Per (model, B) at one image size, both fields with both confidences, everything in ONE process on the same device tensors,
the paths alternating within each of --rounds rounds; a row reports the median of the rounds' hipEvent means:
    hip_forward       gclm_field_loss into a preallocated output and workspace            (reads 20 B per pixel)
    hip_backward      gclm_field_loss_grad into preallocated gradient planes               (reads 20, writes 12 B per pixel)
    hip_both          the public perspective_field_loss on leaves, then perspective_total.sum().backward(): the two kernels
                      plus the autograd.Function, the scale and the allocations
    base_forward      the composition at the parent of this feature: get_perspective_field (one HIP launch, both targets
                      written to memory), then the reference's torch formulas (losses.field_loss) on leaves
    base_both         ... then perspective_total.sum().backward() through autograd;  base_backward = base_both - base_forward
    read_probe        gclm_read_probe on the five input planes: the project's yardstick for a streaming kernel
    variant_backward  hip_backward of a second build of the library (--variant-lib: e.g. one made with
                      -DGCLM_FIELD_LOSS_NT_STORES=1, nontemporal stores of the gradient planes), on the same tensors
TBps counts the bytes each HIP path must move (above) over its time, to set against the 8 TB/s peak.

    python scripts/field_loss_bench.py [--shape 480x640] [--batches 16,64,1024] [--models pinhole,simple_divisional]
                                       [--loss l1] [--rounds 5] [--variant-lib PATH] [--out profiles/field_loss.jsonl]
Appends one JSON line per (model, B, path) to --out and prints it."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from geocalib_amd import Gravity, _lib, camera_models, losses, perspective_fields as pf  # noqa: E402
from geocalib_amd._call import raw_stream  # noqa: E402

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
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="480x640")
    ap.add_argument("--batches", default="16,64,1024")
    ap.add_argument("--models", default="pinhole,simple_divisional")
    ap.add_argument("--loss", default="l1")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--variant-lib", default=None)
    ap.add_argument("--run", default="", help="a label written into every row (e.g. which of two runs)")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "field_loss.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("field_loss_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    variant = None
    if args.variant_lib:
        variant = ctypes.CDLL(args.variant_lib)
        variant.gclm_field_loss_grad.restype, variant.gclm_field_loss_grad.argtypes = _lib._SIGNATURES["gclm_field_loss_grad"]
    H, W = (int(v) for v in args.shape.split("x"))
    kind = _lib.FIELD_LOSS_IDS[args.loss]
    g = torch.Generator().manual_seed(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for model in args.models.split(","):
        for B in (int(b) for b in args.batches.split(",")):
            f = 0.8 * W * (1 + 0.2 * torch.rand(B, generator=g))
            data = torch.stack([torch.full((B,), float(W)), torch.full((B,), float(H)), f, f * 1.01, W / 2 + 3.3 + torch.zeros(B),
                                H / 2 - 2.1 + torch.zeros(B), torch.full((B,), K1[model]), torch.zeros(B)], -1).to(dev)
            roll, pitch = (torch.rand(B, generator=g) - 0.5), (torch.rand(B, generator=g) - 0.5)
            cam, grav = camera_models[model](data), Gravity.from_rp(roll, pitch).to(dev)
            moved = data.clone()                 # predictions: the fields of a calibration 3 degrees and 5 % off
            moved[:, 2:4] *= 1.05
            up, lat = pf.get_perspective_field(camera_models[model](moved), Gravity.from_rp(roll + 0.05, pitch - 0.05).to(dev))
            pred = {"up_field": up.contiguous().requires_grad_(True), "latitude_field": lat.contiguous().requires_grad_(True),
                    "up_confidence": torch.rand(B, H, W, device=dev), "latitude_confidence": torch.rand(B, H, W, device=dev)}
            del up, lat
            gd, px = grav._data.contiguous(), B * H * W
            ws_bytes = lib.gclm_field_loss_workspace(B, H, W)
            ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
            out, scale = torch.empty(B, 4, device=dev), torch.full((B, 2), 1.0 / px, device=dev)
            g_up, g_lat = torch.empty_like(pred["up_field"]), torch.empty_like(pred["latitude_field"])
            mid, p = _lib.CAMERA_MODEL_IDS[model], {k: v.data_ptr() for k, v in pred.items()}
            shared = (mid, data.data_ptr(), gd.data_ptr(), B, H, W, p["up_field"], p["latitude_field"], p["up_confidence"],
                      p["latitude_confidence"], kind, kind)
            planes = (ctypes.c_void_p * 5)(p["up_field"], p["up_field"] + 4 * px, p["latitude_field"], p["up_confidence"],
                                           p["latitude_confidence"])

            def hip_forward():
                assert lib.gclm_field_loss(*shared, ws.data_ptr(), ws_bytes, out.data_ptr(), raw_stream(dev)) == 0

            def hip_backward(which=lib):
                assert which.gclm_field_loss_grad(*shared, scale.data_ptr(), g_up.data_ptr(), g_lat.data_ptr(), raw_stream(dev)) == 0

            def both(fn):
                def run():
                    pred["up_field"].grad = pred["latitude_field"].grad = None
                    fn()["perspective_total"].sum().backward()
                return run

            def base_forward():
                up_t, lat_t = pf.get_perspective_field(cam, grav)
                l_up = losses.field_loss(pred["up_field"], up_t, pred["up_confidence"], args.loss)
                l_lat = losses.field_loss(pred["latitude_field"], lat_t, pred["latitude_confidence"], args.loss)
                return {"up_total": l_up, "latitude_total": l_lat, "perspective_total": l_up + l_lat}

            def probe():
                assert lib.gclm_read_probe(planes, 5, px, raw_stream(dev)) == 0

            hip_public = lambda: losses.perspective_field_loss(pred, cam, grav, args.loss, args.loss)  # noqa: E731
            paths = {"hip_forward": (hip_forward, 20, 20 * px), "hip_backward": (hip_backward, 20, 32 * px),
                     "hip_both": (both(hip_public), 10, 52 * px), "base_forward": (base_forward, 3, None),
                     "base_both": (both(base_forward), 3, None), "read_probe": (probe, 20, 20 * px)}
            if variant is not None:
                paths["variant_backward"] = (lambda: hip_backward(variant), 20, 32 * px)
            times = {k: [] for k in paths}
            for _ in range(args.rounds):         # alternated: the paths share whatever else the box is doing
                for k, (fn, steps, _) in paths.items():
                    times[k].append(timed(fn, steps, 2))
            med = {k: statistics.median(v) for k, v in times.items()}
            med["base_backward"] = med["base_both"] - med["base_forward"]
            # the two paths compute the same thing
            a, b = hip_public(), base_forward()
            diff = max(((a[k] - b[k]).abs() / b[k].abs().clamp(min=1e-30)).max().item() for k in b)
            for k, t in med.items():
                nbytes = paths[k][2] if k in paths else None
                against = {"hip_forward": "base_forward", "hip_backward": "base_backward", "hip_both": "base_both",
                           "variant_backward": "hip_backward"}.get(k)
                row = {"model": model, "B": B, "H": H, "W": W, "loss": args.loss, "path": k, "ms": round(t * 1e3, 4),
                       "rounds_ms": [round(v * 1e3, 4) for v in times.get(k, [])], "run": args.run}
                if nbytes:
                    row.update(TBps=round(nbytes / t / 1e12, 3), of_8TBps_peak=round(nbytes / t / 8e12, 3))
                if against:
                    row["hip_backward_over_this" if k == "variant_backward" else "baseline_over_this"] = round(med[against] / t, 3)
                if k == "variant_backward":
                    row["lib"] = os.path.basename(args.variant_lib)
                if k == "hip_forward":
                    row["read_probe_over_this"] = round(med["read_probe"] / t, 3)
                    row["max_rel_diff_vs_baseline"] = diff
                print(json.dumps(row), flush=True)
                with open(args.out, "a") as fh:
                    fh.write(json.dumps(row) + "\n")
            del pred, ws, out, g_up, g_lat
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
