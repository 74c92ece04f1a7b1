"""Same-allocation A/B of the packed confidence plane (include/gclm.h: gclm_set_conf_pack) on the flagship workload.

The placement of the input planes moves the pinhole solve by up to 8 % between processes, so the plane is judged inside ONE
process on ONE allocation: the fields are made once, and the solve runs with mode 0 / TEST / 0 (TEST = -1, the built-in rule,
unless --mode says 1), each block timed wall-clock over --solves solves and with the library's HIP-event sweep timing.

usage: python scripts/conf_pack_ab.py [--batch 1024] [--solves 10] [--mode -1|1] [--out profiles/conf_pack_ab.json]
       python scripts/conf_pack_ab.py --crossover 110,128,192,256,384,512 [--out profiles/conf_pack_crossover.json]
--crossover: mode 0 / 1 / 0 at each batch size of 640x480; reports the smallest batch from which the packed solve is >= 5 %
faster than the mean of its two unpacked neighbours (gclm_api.hip: GCLM_CONF_PACK_MIN_PIXELS, the built-in rule's threshold,
is kept well above it: DESIGN.md 9.4)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def block(lib, opt, h, data, mode, solves):
    from geocalib_amd import _lib
    opt.conf_pack = {-1: None, 0: False, 1: True}[mode]
    for _ in range(2):
        opt(data)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(solves):
        opt(data)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / solves * 1e3
    lib.gclm_set_timing(h.ptr, 1)
    for _ in range(solves):
        opt(data)
    torch.cuda.synchronize()
    n, ms = C.c_int(0), C.c_float(0)
    _lib.check(lib.gclm_last_pass_timing(h.ptr, C.byref(n), C.byref(ms)), h.ptr, "gclm_last_pass_timing")
    lib.gclm_set_timing(h.ptr, 0)
    return {"mode": mode, "solve_ms": wall, "sweeps_ms_per_solve": ms.value / solves, "sweeps_per_solve": n.value / solves,
            "plane_bytes": int(lib.gclm_conf_pack_bytes(h.ptr))}


def ab(lib, dev, B, H, W, steps, solves, mode, seed):
    from geocalib_amd import LMOptimizer
    from geocalib_amd.synth import synth_fields
    data, _, _ = synth_fields("pinhole", B, H, W, dev, seed=seed)
    opt = LMOptimizer({"camera_model": "pinhole", "num_steps": steps, "early_stop": False}).eval()
    opt.overlap_streams = 1
    h = opt._handle(dev)
    blocks = [block(lib, opt, h, data, m, solves) for m in (0, mode, 0)]
    base = 0.5 * (blocks[0]["solve_ms"] + blocks[2]["solve_ms"])
    base_sw = 0.5 * (blocks[0]["sweeps_ms_per_solve"] + blocks[2]["sweeps_ms_per_solve"])
    res = {"batch": B, "height": H, "width": W, "lm_steps": steps, "solves_per_block": solves, "blocks": blocks,
           "gain_solve": base / blocks[1]["solve_ms"] - 1, "gain_sweeps": base_sw / blocks[1]["sweeps_ms_per_solve"] - 1,
           "images_per_s": {"unpacked": B / base * 1e3, "test": B / blocks[1]["solve_ms"] * 1e3}}
    del data, opt
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--lm-steps", type=int, default=20)
    ap.add_argument("--solves", type=int, default=10)
    ap.add_argument("--mode", type=int, default=-1, choices=[-1, 1])
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--crossover", default=None, help="comma-separated batch sizes")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from geocalib_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    if args.crossover:
        rows = [ab(lib, dev, int(b), args.height, args.width, args.lm_steps, args.solves, 1, args.seed) for b in args.crossover.split(",")]
        for r in rows:
            print(f"B {r['batch']}: solve {r['gain_solve'] * 100:+.1f} %, sweeps {r['gain_sweeps'] * 100:+.1f} %", flush=True)
        ok = [r["batch"] for r in rows if r["gain_solve"] >= 0.05]
        first = next((b for i, b in enumerate(r["batch"] for r in rows) if all(x["gain_solve"] >= 0.05 for x in rows[i:])), None)
        res = {"what": "mode 0 / 1 / 0 per batch size, one allocation each", "rows": rows, "batches_with_5_percent": ok,
               "crossover_batch": first, "crossover_pixels": None if first is None else first * args.height * args.width}
    else:
        res = ab(lib, dev, args.batch, args.height, args.width, args.lm_steps, args.solves, args.mode, args.seed)
        print(f"B {res['batch']}: mode {args.mode} against mode 0: solve {res['gain_solve'] * 100:+.1f} %, sweeps {res['gain_sweeps'] * 100:+.1f} %")
    out = args.out or os.path.join(ROOT, "profiles", "conf_pack_crossover.json" if args.crossover else "conf_pack_ab.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("rows", "blocks")}))


if __name__ == "__main__":
    main()
