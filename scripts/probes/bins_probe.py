"""GPU box: the classification-head epilogue (gclm_pack_fields_bins behind fields.pack_fields_from_logits) at B = 64, 73 + 180
bins, 320 x 480, for float32 and bfloat16 logits, timed with HIP events against two things on the SAME tensors in the same
process: the eager torch composition of the definition (perspective_encoding.fields_from_logits: two argmax, two table gathers,
a permute) and gclm_read_probe over the same logit buffers (16-byte non-temporal loads and nothing else: the read ceiling of that
allocation).  One child process per dtype, under a time limit; inside it every timing has its own deadline, polled on its end
event, and a timing that misses it ends the process (exit status 124) -- nothing more is started on the device after that, here
or in the parent.  Prints one JSON line.

usage: python scripts/probes/bins_probe.py [--json OUT] [--batch 64] [--iters 10]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
H, W, KU, KL = 320, 480, 73, 180
DEADLINE_S = 60.0          # per timing
CHILD_LIMIT_S = 400.0      # per dtype: allocation, three timings, the comparison


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn, iters, what):
    """Mean milliseconds of `fn` over `iters` calls between two events, after three warm-up calls; the process ends if the
    end event has not arrived by the deadline."""
    import torch
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    end = time.monotonic() + DEADLINE_S
    while not e1.query():
        if time.monotonic() > end:
            print(f"bins_probe: {what} missed its deadline of {DEADLINE_S} s", flush=True)
            os._exit(124)
        time.sleep(0.002)
    return e0.elapsed_time(e1) / iters


def child(dtype_name, B, iters):
    import torch
    from geocalib_amd import _call, _lib, perspective_encoding as pe
    from geocalib_amd.fields import pack_fields_from_logits
    dev, dtype = torch.device("cuda:0"), getattr(torch, dtype_name)
    g = torch.Generator(device=dev).manual_seed(1)
    up = torch.empty((B, KU, H, W), dtype=dtype, device=dev)
    lat = torch.empty((B, KL, H, W), dtype=dtype, device=dev)
    for t in (up, lat):                                  # image by image: no float32 copy of the whole batch
        for b in range(B):
            t[b] = torch.randn(t.shape[1:], device=dev, generator=g).to(dtype)
    out = {}
    ms = timed(lambda: out.update(pack_fields_from_logits(up, lat)), iters, "the launch")
    eager = {}
    ms_eager = timed(lambda: eager.update(zip(("up_field", "latitude_field"), pe.fields_from_logits(up, lat))), max(iters // 3, 2),
                     "the eager composition")
    lib, stream = _lib.load(), _call.raw_stream(dev)

    def read():
        for t in (up, lat):
            _lib.check(lib.gclm_read_probe((_lib.C.c_void_p * 1)(t.data_ptr()), 1, t.numel() * t.element_size() // 4, stream), None,
                       "gclm_read_probe")
    ms_read = timed(read, iters, "the read probe")
    same = all(torch.equal(out[k], eager[k]) for k in eager)
    nbytes = (up.numel() + lat.numel()) * up.element_size()
    print(json.dumps({"dtype": dtype_name, "kernel_ms": round(ms, 4), "eager_torch_ms": round(ms_eager, 4),
                      "read_probe_ms": round(ms_read, 4), "eager_over_kernel": round(ms_eager / ms, 2),
                      "fraction_of_read_ceiling": round(ms_read / ms, 4), "logit_bytes": nbytes,
                      "logit_TB_per_s": round(nbytes / ms / 1e9, 3), "read_probe_TB_per_s": round(nbytes / ms_read / 1e9, 3),
                      "equals_eager": bool(same)}), flush=True)


def main():
    B, iters = arg("--batch", 64), arg("--iters", 10)
    if "--child" in sys.argv:
        return child(sys.argv[sys.argv.index("--child") + 1], B, iters)
    rows = []
    for dtype_name in ("float32", "bfloat16"):
        r = subprocess.run(["timeout", "-k", "10", str(int(CHILD_LIMIT_S)), sys.executable, os.path.abspath(__file__), "--child", dtype_name,
                            "--batch", str(B), "--iters", str(iters)], capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            print(r.stdout[-2000:])
            sys.exit(f"bins_probe: the {dtype_name} run ended with status {r.returncode}; nothing more is started")
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps({"probe": "bins_probe", "what": "gclm_pack_fields_bins, no confidences, no sixth plane; mean over "
                       f"{iters} calls between HIP events; the eager composition and gclm_read_probe on the same tensors in the same process",
                       "B": B, "h": H, "w": W, "up_bins": KU, "lat_bins": KL, "rows": rows})
    print(line)
    if "--json" in sys.argv:
        out = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
