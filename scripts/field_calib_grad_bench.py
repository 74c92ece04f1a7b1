"""GPU: the gradients of losses.perspective_field_loss with respect to the camera and the gravity on the HIP path
(`calibration_grad=True`: gclm_field_loss_param_grad) against the route the same call takes without the keyword -- the torch
composition, which is what the parent of this feature does for a calibration that requires grad -- and against the read ceiling.

Per (model, B) at one image size, both fields with both confidences, everything in ONE process on the same device tensors,
the paths alternating within each of --rounds rounds; a row reports the median of the rounds' hipEvent means:
    hip_param_grad   gclm_field_loss_param_grad into preallocated outputs and workspace: the new backward alone
                     (reads 20 B per pixel, writes 72 B per tile); two pixels per lane (W even, aligned planes)
    hip_param_grad_px1
                     the same call on copies of the planes 4 bytes off their alignment, which the launcher walks at one
                     pixel per lane: what the wider instantiation buys
    hip_both         perspective_field_loss(..., calibration_grad=True) on camera and gravity leaves, then
                     perspective_total.sum().backward(): gclm_field_loss, gclm_field_loss_param_grad, the autograd.Function,
                     the scale and the allocations
    base_both        the same call without the keyword on the same tensors: get_perspective_field's torch composition, the
                     reference's loss formulas, autograd backwards
    read_probe       gclm_read_probe on the five planes the kernel reads: the project's yardstick for a streaming kernel
TBps counts the bytes the HIP path must move over its time, to set against the 8 TB/s peak.

    python scripts/field_calib_grad_bench.py [--shape 480x640] [--batches 16,1024] [--models pinhole,simple_divisional]
                                             [--loss l1] [--rounds 3] [--out profiles/field_calib_grad.jsonl]
Appends one JSON line per (model, B, path) to --out and prints it; every row names the host it ran on."""
import argparse
import ctypes
import json
import os
import socket
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
    ap.add_argument("--batches", default="16,1024")
    ap.add_argument("--models", default="pinhole,simple_divisional")
    ap.add_argument("--loss", default="l1")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-base", action="store_true", help="leave the torch composition out (it keeps tens of GB alive at B = 1024)")
    ap.add_argument("--run", default="", help="a label written into every row")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "field_calib_grad.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("field_calib_grad_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    lib = _lib.load()
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
            gd = Gravity.from_rp(roll, pitch).to(dev)._data.contiguous()
            moved = data.clone()                 # predictions: the fields of a calibration 3 degrees and 5 % off
            moved[:, 2:4] *= 1.05
            up, lat = pf.get_perspective_field(camera_models[model](moved), Gravity.from_rp(roll + 0.05, pitch - 0.05).to(dev))
            pred = {"up_field": up.contiguous(), "latitude_field": lat.contiguous(),
                    "up_confidence": torch.rand(B, H, W, device=dev), "latitude_confidence": torch.rand(B, H, W, device=dev)}
            del up, lat
            cam_leaf, grav_leaf = data.clone().requires_grad_(True), gd.clone().requires_grad_(True)
            cam, grav = camera_models[model](cam_leaf), Gravity(gd)
            cam._data, grav._data = cam_leaf, grav_leaf
            px = B * H * W
            ws_bytes = lib.gclm_field_param_grad_workspace(B, H, W)
            ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
            scale = torch.full((B, 2), 1.0 / (H * W), device=dev)
            g_cam, g_grav = torch.empty(B, 8, device=dev), torch.empty(B, 3, device=dev)
            mid, p = _lib.CAMERA_MODEL_IDS[model], {k: v.data_ptr() for k, v in pred.items()}
            shared = (mid, data.data_ptr(), gd.data_ptr(), B, H, W, p["up_field"], p["latitude_field"], p["up_confidence"],
                      p["latitude_confidence"], kind, kind)
            planes = (ctypes.c_void_p * 5)(p["up_field"], p["up_field"] + 4 * px, p["latitude_field"], p["up_confidence"],
                                           p["latitude_confidence"])

            def hip_param_grad(args=shared):
                assert lib.gclm_field_loss_param_grad(*args, scale.data_ptr(), ws.data_ptr(), ws_bytes, g_cam.data_ptr(),
                                                      g_grav.data_ptr(), raw_stream(dev)) == 0

            def shifted(floats):                 # the same planes `floats` floats past an aligned address, and the call's arguments
                keep = {}
                for k, v in pred.items():
                    flat = torch.empty(v.numel() + floats, device=dev)
                    flat[floats:].copy_(v.reshape(-1))
                    keep[k] = flat
                q = {k: v.data_ptr() + 4 * floats for k, v in keep.items()}
                return keep, shared[:6] + (q["up_field"], q["latitude_field"], q["up_confidence"], q["latitude_confidence"]) + shared[10:]

            def both(flag):
                def run():
                    cam_leaf.grad = grav_leaf.grad = None
                    losses.perspective_field_loss(pred, cam, grav, args.loss, args.loss, calibration_grad=flag)["perspective_total"].sum().backward()
                return run

            def probe():
                assert lib.gclm_read_probe(planes, 5, px, raw_stream(dev)) == 0

            big = B >= 256
            paths = {"hip_param_grad": (hip_param_grad, 20, 20 * px), "hip_both": (both(True), 10, 40 * px), "read_probe": (probe, 20, 20 * px)}
            if W % 2 == 0:
                keep1, args1 = shifted(1)
                paths["hip_param_grad_px1"] = (lambda: hip_param_grad(args1), 20, 20 * px)
            if not args.no_base:
                paths["base_both"] = (both(False), 1 if big else 3, None)
            times = {k: [] for k in paths}
            for _ in range(args.rounds):         # alternated: the paths share whatever else the box is doing
                for k, (fn, steps, _) in paths.items():
                    times[k].append(timed(fn, steps, 1 if k == "base_both" and big else 2))
            med = {k: statistics.median(v) for k, v in times.items()}
            # the two routes compute the same thing
            diff = None
            if not args.no_base:
                both(True)()
                hip = torch.cat([cam_leaf.grad, grav_leaf.grad], 1)
                both(False)()
                base = torch.cat([cam_leaf.grad, grav_leaf.grad], 1)
                diff = ((hip - base).abs().amax(0) / base.abs().amax(0).clamp(min=1e-30)).max().item()
            for k, t in med.items():
                nbytes = paths[k][2]
                row = {"model": model, "B": B, "H": H, "W": W, "loss": args.loss, "path": k, "ms": round(t * 1e3, 4),
                       "rounds_ms": [round(v * 1e3, 4) for v in times[k]], "run": args.run, "host": socket.gethostname()}
                if nbytes:
                    row.update(TBps=round(nbytes / t / 1e12, 3), of_8TBps_peak=round(nbytes / t / 8e12, 3))
                if k == "hip_both" and "base_both" in med:
                    row.update(baseline_over_this=round(med["base_both"] / t, 3), max_rel_diff_vs_baseline=diff)
                if k.startswith("hip_param_grad"):
                    row["read_probe_over_this"] = round(med["read_probe"] / t, 3)
                print(json.dumps(row), flush=True)
                with open(args.out, "a") as fh:
                    fh.write(json.dumps(row) + "\n")
            del pred, ws, cam, grav, cam_leaf, grav_leaf, paths
            keep1 = None
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
