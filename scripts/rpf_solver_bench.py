"""GPU: the three-pixel minimal solver (gclm_rpf_hypotheses) and RPFSolver.forward around it.

There is nothing in earlier versions of the package to compare the solve with; the yardstick is the torch composition of the
same definition (ransac._solve_torch) on the same device tensors in the same process.  Timings are hipEvent means over
--steps calls after --warmup, one timed region per row:
    hip_kernel     gclm_rpf_hypotheses into preallocated rows, the samples drawn in the kernel
    hip_method     the public solve_rpf (allocates its outputs, wraps them)
    torch_solve    ransac._solve_torch on float32 device tensors, the samples given (the draw is not timed)
    rank           metrics.rank_calibrations on the rows of the solve (gclm_hypothesis_scores)
    forward        RPFSolver.forward: solve, rank, winner, the winner's inlier maps
`rank_share_of_forward` is rank over forward; `valid_share` the share of the 2 N rows that are valid (the rest score 0 in the
ranking: what compacting them away could save).

    python scripts/rpf_solver_bench.py [--size 320x320] [--batches 1,16] [--samples 256,1000] [--steps 50] [--out FILE]
Prints one JSON line per (B, N, path); --out appends them to a file as well."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from geocalib_amd import Gravity, Pinhole, RPFSolver, _lib, metrics, ransac, solve_rpf  # noqa: E402
from geocalib_amd import perspective_fields as pf  # noqa: E402
from geocalib_amd._call import raw_stream  # noqa: E402


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
    ap.add_argument("--size", default="320x320", help="HxW")
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--samples", default="256,1000")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--noise", type=float, default=0.02)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rpf_solver_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    H, W = (int(v) for v in args.size.split("x"))
    g = torch.Generator().manual_seed(0)
    sink = open(args.out, "a") if args.out else None
    for B in (int(v) for v in args.batches.split(",")):
        vfov = torch.deg2rad(40 + 50 * torch.rand(B, generator=g))
        f = H / 2 / torch.tan(vfov / 2)
        cam = torch.stack([torch.full((B,), float(W)), torch.full((B,), float(H)), f, f, torch.full((B,), W / 2), torch.full((B,), H / 2),
                           torch.zeros(B), torch.zeros(B)], -1).to(dev)
        roll, pitch = (torch.rand(B, generator=g) - 0.5) * 1.4, (torch.rand(B, generator=g) - 0.5) * 1.4
        grav = Gravity.from_rp(roll, pitch).to(dev)
        up, lat = pf.get_perspective_field(Pinhole(cam), grav)
        up = torch.nn.functional.normalize(up + args.noise * torch.randn(up.shape, device=dev), dim=1).contiguous()
        lat = (lat + args.noise * torch.randn(lat.shape, device=dev)).clamp(-math.pi / 2 + 1e-3, math.pi / 2 - 1e-3).contiguous()
        pred = {"up_field": up, "latitude_field": lat, "up_confidence": torch.rand(B, H, W, device=dev),
                "latitude_confidence": torch.rand(B, H, W, device=dev)}
        for N in (int(v) for v in args.samples.split(",")):
            rows_c, rows_g = torch.empty(B, 2 * N, 8, device=dev), torch.empty(B, 2 * N, 3, device=dev)
            used = torch.empty(B, N, 3, 2, dtype=torch.int32, device=dev)
            stream = raw_stream(dev)

            def kernel():
                rc = lib.gclm_rpf_hypotheses(up.data_ptr(), lat.data_ptr(), None, None, 7, 0, B, N, H, W, rows_c.data_ptr(), rows_g.data_ptr(),
                                             used.data_ptr(), stream)
                assert rc == 0, rc

            kernel()
            hyp = solve_rpf(pred, n=N, seed=7)
            torch.cuda.synchronize()
            assert torch.equal(hyp["samples"], used)
            solver = RPFSolver({"n_iter": N, "seed": 7})
            t = {"hip_kernel": timed(kernel, 4 * args.steps, args.warmup),
                 "hip_method": timed(lambda: solve_rpf(pred, n=N, seed=7), args.steps, args.warmup),
                 "torch_solve": timed(lambda: ransac._solve_torch(up, lat, None, used), args.steps, args.warmup),
                 "rank": timed(lambda: metrics.rank_calibrations(pred, hyp["cameras"], hyp["gravities"]), args.steps, args.warmup),
                 "forward": timed(lambda: solver(pred), args.steps, args.warmup)}
            t["hip_kernel_again"] = timed(kernel, 4 * args.steps, args.warmup)          # the spread of the first row
            # both solves on the same pixels: how far apart their valid rows and their winners are
            tc, tg = ransac._solve_torch(up, lat, None, used)
            both = ~tc[..., 2].isnan() & hyp["valid"]
            out = solver(pred)
            ferr = (out["camera_opt"]._data[:, 2] / cam[:, 2] - 1).abs().max().item()
            ang = torch.rad2deg(torch.acos((out["gravity_opt"]._data * grav._data).sum(-1).clamp(-1, 1))).max().item()
            for path, sec in t.items():
                line = json.dumps({"B": B, "N": N, "H": H, "W": W, "noise": args.noise, "path": path, "us": round(sec * 1e6, 2),
                                   "torch_solve_over_this": round(t["torch_solve"] / sec, 2),
                                   "rank_share_of_forward": round(t["rank"] / t["forward"], 3),
                                   "valid_share": round(hyp["valid"].float().mean().item(), 3),
                                   "validity_mismatch_vs_torch": round((~tc[..., 2].isnan() != hyp["valid"]).float().mean().item(), 5),
                                   "rows_valid_on_both": int(both.sum()), "winner_focal_rel_err": round(ferr, 4),
                                   "winner_gravity_err_deg": round(ang, 3), "device": torch.cuda.get_device_name(0)})
                print(line, flush=True)
                if sink:
                    sink.write(line + "\n")
                    sink.flush()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
