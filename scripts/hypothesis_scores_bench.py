"""GPU: gclm_hypothesis_scores (metrics.rank_calibrations on the HIP path) against the best composition the package offered
before it.

Timings on the same device tensors, hipEvent means over --steps calls after --warmup, one timed region per row:
    hip_kernel         gclm_hypothesis_scores into preallocated scores, best and workspace: both fields, both confidences
    hip_method         the public rank_calibrations (allocates its outputs and the workspace, gathers the winners)
    baseline_repeat    fields.field_errors(return_errors=True) on the fields repeated per hypothesis, in chunks of hypotheses
                       that keep the copies under --chunk-bytes, then torch's ((e < t) * conf).sum per field
    baseline_calls     N calls of fields.field_errors(return_errors=True) on the fields as they are, one per hypothesis, and the
                       same torch pass
    variant_kernel     hip_kernel of a second build of the library (--variant-lib, repeatable: e.g. builds with
                       -DGCLM_HYPOTHESIS_CHUNK=8 / 32), in the same process on the same tensors
`baseline_over_this` is the faster of the two baselines over the row's time.  ns_per_px_hyp is time per (pixel x hypothesis);
valu_per_px_hyp counts the VALU instructions of the kernel's hypothesis loop in the code object (llvm-objdump; both sides of
every branch, so an upper bound of what a lane issues) per pixel, and valu_rate is that count x pixels x hypotheses / time
against the 39.3 T lane-operations/s of 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz.

    python scripts/hypothesis_scores_bench.py [--size 320x320] [--batches 1,16] [--hypotheses 16,256,2000]
                                              [--models pinhole,simple_divisional] [--steps 30] [--variant-lib PATH ...]
Prints one JSON line per (model, B, N, path)."""
import argparse
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from geocalib_amd import Gravity, _lib, camera_models, fields, metrics, perspective_fields as pf  # noqa: E402
from geocalib_amd._call import raw_stream as _raw_stream  # noqa: E402

K1 = {"simple_radial": -0.3, "radial": -0.3, "simple_divisional": -0.8, "pinhole": 0.0}
LLVM = "/opt/rocm/lib/llvm/bin"
PEAK_LANE_OPS = 256 * 4 * 16 * 2.4e9


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
    for name in ("gclm_hypothesis_scores", "gclm_hypothesis_scores_workspace"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._SIGNATURES[name]
    return lib


def loop_valu(lib_path, model_id, px):
    """VALU instructions of hypothesis_kernel<model_id, px>'s hypothesis loop (the widest backward branch of the kernel) in
    the library's gfx950 code object; None where the LLVM tools are missing."""
    if not os.path.exists(f"{LLVM}/llvm-objdump"):
        return None
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(lib_path, os.path.join(tmp, "lib.so"))        # (the code objects are extracted next to the input)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", "lib.so"], cwd=tmp, check=True, capture_output=True)
        for f in sorted(os.listdir(tmp)):
            if "amdgcn" not in f:
                continue
            text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", f], cwd=tmp, check=True, capture_output=True, text=True).stdout
            m = re.search(r"^[0-9a-f]+ <(\S*hypothesis_kernelILi%dELi%dE\S*)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)" % (model_id, px), text, re.S | re.M)
            if not m:
                continue
            ins = []                             # (address, mnemonic, branch target or None)
            for line in m.group(2).splitlines():
                a = re.search(r"^\s*(\S+).*//\s*([0-9A-Fa-f]{12}):", line)
                if not a:
                    continue
                t = re.search(r"<\S+\+0x([0-9a-fA-F]+)>\s*$", line)
                ins.append((int(a.group(2), 16), a.group(1), None if t is None else t.group(1)))
            base = ins[0][0]
            loops = [(addr - (base + int(t, 16)), base + int(t, 16), addr) for addr, op, t in ins
                     if t is not None and "branch" in op and base + int(t, 16) < addr]
            if not loops:
                return None
            _, lo, hi = max(loops)
            return sum(1 for addr, op, _ in ins if lo <= addr <= hi and op.startswith("v_"))
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="320x320", help="HxW")
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--hypotheses", default="16,256,2000")
    ap.add_argument("--models", default="pinhole,simple_divisional")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--baseline-steps", type=int, default=3)
    ap.add_argument("--chunk-bytes", type=float, default=4e9, help="most bytes of repeated fields and error maps of one baseline chunk")
    ap.add_argument("--variant-lib", action="append", default=[])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hypothesis_scores_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    variants = [(os.path.basename(path), bind(path)) for path in args.variant_lib]
    H, W = (int(v) for v in args.size.split("x"))
    g = torch.Generator().manual_seed(0)
    t_up = t_lat = 1.0
    for model in args.models.split(","):
        mid = _lib.CAMERA_MODEL_IDS[model]
        px = 4 if W % 4 == 0 else 2 if W % 2 == 0 else 1                       # (torch's planes are 16-byte aligned)
        valu = {p: loop_valu(p, mid, px) for p in [_lib.LIB_PATH] + args.variant_lib}
        valu = {p: None if v is None else round(v / px, 1) for p, v in valu.items()}
        for B in (int(v) for v in args.batches.split(",")):
            f = 0.8 * W * (1 + 0.2 * torch.rand(B, generator=g))
            data = torch.stack([torch.full((B,), float(W)), torch.full((B,), float(H)), f, f * 1.01,
                                W / 2 + 3.3 + torch.zeros(B), H / 2 - 2.1 + torch.zeros(B), torch.full((B,), K1[model]),
                                torch.zeros(B)], -1).to(dev)
            roll, pitch = (torch.rand(B, generator=g) - 0.5), (torch.rand(B, generator=g) - 0.5)
            # predictions: the fields of the calibration itself; hypotheses: that calibration moved by up to +-6 degrees and +-10 %
            up, lat = pf.get_perspective_field(camera_models[model](data), Gravity.from_rp(roll, pitch).to(dev))
            pred = {"up_field": up.contiguous(), "latitude_field": lat.contiguous(),
                    "up_confidence": torch.rand(B, H, W, device=dev), "latitude_confidence": torch.rand(B, H, W, device=dev)}
            del up, lat
            for N in (int(v) for v in args.hypotheses.split(",")):
                s = (torch.rand(B, N, generator=g) - 0.5) * 2
                hc = data[:, None].repeat(1, N, 1)
                hc[..., 2:4] *= (1 + 0.1 * s.to(dev))[..., None]
                hg = Gravity.from_rp(roll[:, None] + 0.1 * s, pitch[:, None] - 0.1 * s.flip(1))._data.to(dev).contiguous()
                cam, grav = camera_models[model](hc), Gravity(hg)
                scores = torch.empty(B, N, 3, device=dev)
                best = torch.empty(B, dtype=torch.int32, device=dev)
                p = {k: v.data_ptr() for k, v in pred.items()}

                def kernel(which=lib):
                    ws_bytes = which.gclm_hypothesis_scores_workspace(B, N, H, W)
                    if kernel.ws is None or kernel.ws.numel() * 4 < ws_bytes:
                        kernel.ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
                    rc = which.gclm_hypothesis_scores(mid, hc.data_ptr(), hg.data_ptr(), B, N, H, W, p["up_field"], p["latitude_field"],
                                                      p["up_confidence"], p["latitude_confidence"], None, t_up, t_lat, 1.0, 1.0,
                                                      kernel.ws.data_ptr(), kernel.ws.numel() * 4, scores.data_ptr(), best.data_ptr(),
                                                      _raw_stream(dev))
                    assert rc == 0, rc
                kernel.ws = None

                def torch_pass(ue, le, k):
                    su = ((ue.view(B, k, H, W) < t_up).float() * pred["up_confidence"][:, None]).sum((2, 3))
                    sl = ((le.view(B, k, H, W) < t_lat).float() * pred["latitude_confidence"][:, None]).sum((2, 3))
                    return su, sl

                step = max(1, min(N, int(args.chunk_bytes // (B * H * W * 4 * 5))))      # 3 repeated planes + 2 error maps

                def baseline_repeat():
                    parts = []
                    for n0 in range(0, N, step):
                        k = min(step, N - n0)
                        u = pred["up_field"][:, None].expand(B, k, 2, H, W).reshape(B * k, 2, H, W)
                        la = pred["latitude_field"][:, None].expand(B, k, 1, H, W).reshape(B * k, 1, H, W)
                        _, ue, le = fields.field_errors(model, hc[:, n0:n0 + k].reshape(B * k, 8), hg[:, n0:n0 + k].reshape(B * k, 3),
                                                        u, la, None, None, (), return_errors=True)
                        parts.append(torch_pass(ue, le, k))
                    su, sl = torch.cat([a for a, _ in parts], 1), torch.cat([b for _, b in parts], 1)
                    return su, sl, (su + sl).argmax(1)

                def baseline_calls():
                    parts = []
                    for n in range(N):
                        _, ue, le = fields.field_errors(model, hc[:, n], hg[:, n], pred["up_field"], pred["latitude_field"], None, None,
                                                        (), return_errors=True)
                        parts.append(torch_pass(ue, le, 1))
                    su, sl = torch.cat([a for a, _ in parts], 1), torch.cat([b for _, b in parts], 1)
                    return su, sl, (su + sl).argmax(1)

                rows = [("hip_kernel", timed(kernel, args.steps, args.warmup), _lib.LIB_PATH)]
                for name, vlib in variants:
                    rows.append((f"variant_kernel:{name}", timed(lambda: kernel(vlib), args.steps, args.warmup), name))
                if variants:
                    rows.append(("hip_kernel_again", timed(kernel, args.steps, args.warmup), _lib.LIB_PATH))
                rows.append(("hip_method", timed(lambda: metrics.rank_calibrations(pred, cam, grav), args.steps, args.warmup), _lib.LIB_PATH))
                bases = {"baseline_repeat": timed(baseline_repeat, args.baseline_steps, 1),
                         "baseline_calls": timed(baseline_calls, args.baseline_steps, 1)}
                rows += [(k, v, _lib.LIB_PATH) for k, v in bases.items()]
                base = min(bases.values())
                kernel()
                su, sl, bb = baseline_repeat()
                torch.cuda.synchronize()
                diff = max((su - scores[..., 0]).abs().max().item(), (sl - scores[..., 1]).abs().max().item())
                same_best = int((bb == best.long()).sum())
                pxh = B * N * H * W
                for path, t, which in rows:
                    v = valu.get(next((q for q in [_lib.LIB_PATH] + args.variant_lib if os.path.basename(q) == os.path.basename(which)),
                                      _lib.LIB_PATH)) if "kernel" in path or path == "hip_method" else None
                    print(json.dumps({"model": model, "B": B, "N": N, "H": H, "W": W, "path": path, "ms": round(t * 1e3, 4),
                                      "ns_per_px_hyp": round(t / pxh * 1e9, 6), "valu_per_px_hyp": v,
                                      "valu_rate_of_peak": None if v is None else round(v * pxh / t / PEAK_LANE_OPS, 3),
                                      "baseline_over_this": round(base / t, 2), "baseline_chunk": step,
                                      "max_abs_score_diff_vs_baseline": diff, "same_best": f"{same_best}/{B}",
                                      "lib": os.path.basename(which)}), flush=True)
                del scores, best, hc, hg
                kernel.ws = None
                torch.cuda.empty_cache()
            del pred
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
