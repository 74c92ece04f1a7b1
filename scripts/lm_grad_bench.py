"""GPU: the differentiable LM solve (lm_grad.py) -- what the step record costs the forward, and what the backward costs.

Per (model, B) at one image size, both fields with both confidences, 10 fixed LM steps, everything in ONE process on the same
device tensors, the paths alternating within each of --rounds rounds; a row reports the median of the rounds' hipEvent means:
    forward_plain     LMOptimizer.calibrate_fields: gclm_calibrate_ex, the entry point of the parent commit
    forward_recorded  lm_grad.recorded_solve: gclm_calibrate_recorded into a preallocated-per-call record
    backward          gclm_lm_backward on that record into preallocated gradient planes (all four), num_steps steps
    read_probe        gclm_read_probe over the five input planes: what ONE step of either pass must at least read (20 B/px;
                      a backward step also reads and writes the four gradient planes, 20 + 40 B/px from its second step on)
    python scripts/lm_grad_bench.py [--shape 480x640] [--batches 16,1024] [--models pinhole,simple_radial] [--steps 10]
                                    [--rounds 5] [--out profiles/lm_grad.jsonl] [--accuracy]
Appends one JSON line per (model, B, path) to --out and prints it.

--accuracy adds the rows of the gradient gate: per case of tests/golden/lm_grad_reference.npz and per input, the error of the HIP
gradients and of the reference's own float32 gradients against its float64 ones, per image, and their ratio -- the figures
tests/test_lm_grad.py asserts on, computed by that module's own functions (`--batches ""` writes these rows alone)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from geocalib_amd import LMOptimizer, _lib, lm_grad  # noqa: E402
from geocalib_amd._call import raw_stream  # noqa: E402
from geocalib_amd.synth import synth_fields  # noqa: E402


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


def accuracy_rows(root):
    sys.path.insert(0, os.path.join(root, "tests"))
    import numpy as np
    import test_lm_grad as T
    ref = np.load(os.path.join(root, "tests", "golden", "lm_grad_reference.npz"))
    rows = []
    for name in T.ALL_CASES:
        _, grads = T.run_grad(ref, name)
        for k, g in grads.items():
            g64 = torch.from_numpy(ref[f"{name}/grad64/{k}"])
            own = T.per_image_err(torch.from_numpy(ref[f"{name}/grad32/{k}"]).double(), g64)
            err = T.per_image_err(g.detach().cpu().double(), g64)
            rows.append({"bench": "lm_grad_accuracy", "case": name, "input": k, "hip_err": [float(f"{v:.3e}") for v in err.tolist()],
                         "reference_float32_err": [float(f"{v:.3e}") for v in own.tolist()],
                         "ratio": [round(v, 2) for v in (err / own).tolist()]})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="480x640")
    ap.add_argument("--batches", default="16,1024")
    ap.add_argument("--models", default="pinhole,simple_radial")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--run", default="", help="a label written into every row")
    ap.add_argument("--accuracy", action="store_true", help="add the rows of the gradient gate (tests/test_lm_grad.py)")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "lm_grad.jsonl"))
    args = ap.parse_args()
    H, W = (int(v) for v in args.shape.split("x"))
    dev = torch.device("cuda:0")
    lib = _lib.load()
    rows = []
    for model in args.models.split(","):
        for B in (int(b) for b in args.batches.split(",") if b):
            data, _, _ = synth_fields(model, B, H, W, dev, seed=5)
            conf = {"camera_model": model, "num_steps": args.steps, "early_stop": False}
            opt = LMOptimizer(conf).train()
            opt.overlap_streams = 1                    # one call on one stream on both sides: separable durations
            px = B * H * W
            _, _, _, record = lm_grad.recorded_solve(opt, data)
            info = opt._last_raw[2]
            g_cam, g_grav = torch.ones(B, 8, device=dev), torch.ones(B, 3, device=dev)
            outs = [torch.empty_like(data[k]) for k in ("up_field", "latitude_field", "up_confidence", "latitude_confidence")]
            ws_bytes = lib.gclm_lm_backward_workspace(B, H, W)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            p = {k: v.data_ptr() for k, v in data.items()}
            planes = (ctypes.c_void_p * 5)(p["up_field"], p["up_field"] + 4 * px, p["latitude_field"], p["up_confidence"],
                                           p["latitude_confidence"])

            def forward_plain():
                opt.calibrate_fields(data)

            def forward_recorded():
                lm_grad.recorded_solve(opt, data)

            def backward():
                assert lib.gclm_lm_backward(_lib.CAMERA_MODEL_IDS[model], p["up_field"], p["latitude_field"], p["up_confidence"],
                                            p["latitude_confidence"], B, H, W, record.data_ptr(), args.steps, 0, info.data_ptr(),
                                            1e-2, 1e-2, 1, 1, int(model != "pinhole"), g_cam.data_ptr(), g_grav.data_ptr(),
                                            *(t.data_ptr() for t in outs), ws.data_ptr(), ws_bytes, raw_stream(dev)) == 0

            def probe():
                assert lib.gclm_read_probe(planes, 5, px, raw_stream(dev)) == 0

            reps = 3 if B >= 256 else 10
            paths = {"forward_plain": (forward_plain, reps), "forward_recorded": (forward_recorded, reps),
                     "backward": (backward, reps), "read_probe": (probe, 20)}
            times = {k: [] for k in paths}
            for _ in range(args.rounds):
                for k, (fn, n) in paths.items():
                    times[k].append(timed(fn, n, 1))
            med = {k: statistics.median(v) for k, v in times.items()}
            for k, t in med.items():
                row = {"bench": "lm_grad", "model": model, "B": B, "H": H, "W": W, "steps": args.steps, "path": k,
                       "ms": round(t * 1e3, 4), "rounds": args.rounds, "run": args.run}
                if k == "forward_recorded":
                    row["vs_forward_plain"] = round(t / med["forward_plain"], 4)
                if k == "backward":
                    row["vs_forward_plain"] = round(t / med["forward_plain"], 3)
                    row["vs_read_probe_per_step"] = round(t / args.steps / med["read_probe"], 2)
                rows.append(row)
                print(json.dumps(row), flush=True)
    if args.accuracy:
        rows += accuracy_rows(root)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
