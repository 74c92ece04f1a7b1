"""GPU: fields.pack_fields with a graph (gclm_pack_fields_ex / gclm_pack_fields_typed forward, gclm_pack_fields_backward)
against the eager torch lines it replaces in a training step.

Per (dtype, B) at one image size, both confidences, everything in ONE process on the same device tensors, the paths
alternating within each of --rounds rounds; a row reports the median of the rounds' hipEvent means and their range:
    hip_forward / hip_backward / hip_both        pack_fields on raws that require grad; torch.autograd.grad of its four outputs
                                                 under fixed incoming gradients (retain_graph: only the raws are kept); both
    eager_forward / eager_backward / eager_both  the reference's four lines (F.normalize, asin(clamp(tanh)), two sigmoids) on the
                                                 same raws -- on `.float()` of them for 16-bit raws, which is what hands a
                                                 float32 solve its fields -- and autograd's backward of them
    entry_backward                               gclm_pack_fields_backward alone, into preallocated planes (no autograd, no
                                                 allocation): what the kernel takes
    variant_backward                             the same call of a second build of the library (--variant-lib: e.g. one made
                                                 with -DGCLM_PACK_BWD_NT_STORES, non-temporal stores of the raw gradients)
    entry_backward_read / variant_backward_read  either call followed by gclm_read_probe over the raw gradients it wrote: the
                                                 pass together with a kernel that reads its output next, as autograd's does
and one row per (dtype, B) with the peak device memory of one forward + backward of each chain above what the raws, the
incoming gradients and the results occupy.
    python scripts/pack_fields_grad_bench.py [--shape 480x640] [--batches 16,64,1024] [--dtypes float32,bfloat16]
                                             [--rounds 5] [--variant-lib PATH] [--out profiles/pack_fields_grad.jsonl]
Appends one JSON line per row to --out and prints it.  Bytes per pixel: float32 raws 40 forward (20 read, 20 written) and 60
backward (20 raws, 20 incoming gradients, 20 raw gradients); 16-bit raws 30 and 40."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from geocalib_amd import _lib  # noqa: E402
from geocalib_amd._call import raw_stream  # noqa: E402
from geocalib_amd.fields import pack_fields  # noqa: E402

KEYS = ("up_field", "latitude_field", "up_confidence", "latitude_confidence")


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


def eager_lines(up_raw, lat_raw, ulc, llc):
    up_raw, lat_raw, ulc, llc = (t.float() for t in (up_raw, lat_raw, ulc, llc))
    return (F.normalize(up_raw, dim=1), torch.asin(torch.clamp(torch.tanh(lat_raw), -1 + 1e-5, 1 - 1e-5)), torch.sigmoid(ulc),
            torch.sigmoid(llc))


def hip_lines(up_raw, lat_raw, ulc, llc):
    out = pack_fields(up_raw, lat_raw, ulc, llc)
    return tuple(out[k] for k in KEYS)


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="480x640")
    ap.add_argument("--batches", default="16,64,1024")
    ap.add_argument("--dtypes", default="float32,bfloat16")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--variant-lib", default=None)
    ap.add_argument("--run", default="", help="a label written into every row")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "pack_fields_grad.jsonl"))
    args = ap.parse_args()
    H, W = (int(v) for v in args.shape.split("x"))
    dev = torch.device("cuda:0")
    lib = _lib.load()
    variant = None
    if args.variant_lib:
        variant = ctypes.CDLL(args.variant_lib)
        variant.gclm_pack_fields_backward.restype, variant.gclm_pack_fields_backward.argtypes = _lib._SIGNATURES["gclm_pack_fields_backward"]
    rows = []
    for dtype_name in args.dtypes.split(","):
        dtype = getattr(torch, dtype_name)
        fwd_bytes, bwd_bytes = (40, 60) if dtype is torch.float32 else (30, 40)
        for B in (int(b) for b in args.batches.split(",") if b):
            px = B * H * W
            g = torch.Generator(device=dev).manual_seed(B)
            raws = [torch.randn(s, generator=g, device=dev).to(dtype).requires_grad_(True)
                    for s in ((B, 2, H, W), (B, 1, H, W), (B, H, W), (B, 1, H, W))]
            grads = [torch.randn(s, generator=g, device=dev) for s in ((B, 2, H, W), (B, 1, H, W), (B, H, W), (B, H, W))]
            eager_grads = [grads[0], grads[1], grads[2], grads[3].view(B, 1, H, W)]
            d = [torch.empty_like(t) for t in raws]
            held = {"hip": hip_lines(*raws), "eager": eager_lines(*raws)}
            p = [t.data_ptr() for t in raws]
            gp, dp = [t.data_ptr() for t in grads], [t.data_ptr() for t in d]

            def forward(fn):
                return lambda: fn(*raws)

            def backward(which, gs):
                return lambda: torch.autograd.grad(held[which], raws, gs, retain_graph=True)

            def both(fn, gs):
                return lambda: torch.autograd.grad(fn(*raws), raws, gs)

            def entry(library):
                def call():
                    assert library.gclm_pack_fields_backward(_lib.LOGIT_DTYPE_IDS[dtype_name], p[0], p[2], p[1], p[3], B, H, W, gp[0],
                                                             gp[2], gp[1], gp[3], dp[0], dp[2], dp[1], dp[3], raw_stream(dev)) == 0
                return call

            d_floats = d[1].numel() * d[1].element_size() // 4            # one plane of raw gradients, counted in floats
            d_planes = (ctypes.c_void_p * 5)(dp[0], dp[0] + 4 * d_floats, dp[1], dp[2], dp[3])

            def then_read(call):
                def run():
                    call()
                    assert lib.gclm_read_probe(d_planes, 5, d_floats, raw_stream(dev)) == 0
                return run

            reps = 5 if B >= 256 else 20
            paths = {"hip_forward": forward(hip_lines), "hip_backward": backward("hip", grads), "hip_both": both(hip_lines, grads),
                     "eager_forward": forward(eager_lines), "eager_backward": backward("eager", eager_grads),
                     "eager_both": both(eager_lines, eager_grads), "entry_backward": entry(lib)}
            paths["entry_backward_read"] = then_read(entry(lib))
            if variant is not None:
                paths["variant_backward"] = entry(variant)
                paths["variant_backward_read"] = then_read(entry(variant))
            times = {k: [] for k in paths}
            for _ in range(args.rounds):
                for k, fn in paths.items():
                    times[k].append(timed(fn, reps, 2))
            med = {k: statistics.median(v) for k, v in times.items()}
            for k, t in med.items():
                row = {"bench": "pack_fields_grad", "dtype": dtype_name, "B": B, "H": H, "W": W, "path": k, "ms": round(t * 1e3, 4),
                       "ms_range": [round(min(times[k]) * 1e3, 4), round(max(times[k]) * 1e3, 4)], "rounds": args.rounds,
                       "calls_per_round": reps, "run": args.run}
                if k in ("hip_forward", "hip_backward", "entry_backward", "variant_backward"):      # (the _read paths move more)
                    row["bytes_per_px"] = fwd_bytes if k == "hip_forward" else bwd_bytes
                    row["TB_per_s"] = round(row["bytes_per_px"] * px / t * 1e-12, 3)
                if k.startswith("hip_"):
                    row["eager_over_this"] = round(med["eager_" + k[4:]] / t, 2)
                if k == "hip_backward":
                    row["over_hip_forward"] = round(t / med["hip_forward"], 3)
                if k.startswith("variant_"):
                    row["product_over_this"] = round(med[k.replace("variant_", "entry_")] / t, 4)
                    row["lib"] = os.path.basename(args.variant_lib)
                rows.append(row)
                print(json.dumps(row), flush=True)
            # peak memory of one forward + backward, above what is alive before it (raws, incoming gradients, held graphs)
            del held
            peaks = {}
            for name, fn, gs in (("hip", hip_lines, grads), ("eager", eager_lines, eager_grads)):
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                got = torch.autograd.grad(fn(*raws), raws, gs)
                torch.cuda.synchronize()
                peaks[name] = torch.cuda.max_memory_allocated() - base
                del got
            row = {"bench": "pack_fields_grad_memory", "dtype": dtype_name, "B": B, "H": H, "W": W,
                   "hip_peak_MB": round(peaks["hip"] / 2 ** 20, 1), "eager_peak_MB": round(peaks["eager"] / 2 ** 20, 1),
                   "bytes_per_px": {k: round(v / px, 1) for k, v in peaks.items()}, "eager_over_hip": round(peaks["eager"] / peaks["hip"], 2),
                   "run": args.run}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del raws, grads, eager_grads, d
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
