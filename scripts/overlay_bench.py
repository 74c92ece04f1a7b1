"""Kernel time of viz.draw_perspective_fields (gclm_draw_fields_u8) on uint8 channels_last C = 3 frames, by HIP events, warm,
against what a caller without it can do on the device for the TINT ALONE: HIP get_perspective_field, then the torch palette
gather and blend (the comparator does strictly less work: no lines, no arrows, nearest palette bin).

    python scripts/overlay_bench.py [--out profiles/overlay_bench.jsonl] [--reps 20]

One JSON line per (size, B, variant): us per frame, GB/s of 2 B H W C bytes, and the ratio comparator / kernel."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geocalib_amd import Gravity, _lib, camera_models, viz  # noqa: E402
from geocalib_amd.perspective_fields import get_perspective_field  # noqa: E402


def timed(fn, reps):
    """Median milliseconds per call of `fn` over `reps` event-timed windows after three warm-up runs; a window holds as many
    calls as fill about 20 ms, so that a 10 us kernel is not a measurement of the event pair."""
    def window(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    inner = max(1, min(1000, int(20.0 / max(window(3), 1e-3))))
    return sorted(window(inner) for _ in range(reps))[reps // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--model", default="simple_radial")
    ap.add_argument("--quick", action="store_true", help="B = 16 only (A/B of two builds of the library, GCLM_LIB_PATH)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for H, W in ((480, 640), (1080, 1920)):
        for B in ((16,) if args.quick else (1, 16, 64)):
            g = torch.Generator().manual_seed(B)
            img = torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8).to(dev).contiguous(memory_format=torch.channels_last)
            f = 0.8 * W
            cams = torch.tensor([[W, H, f, f, W / 2, H / 2, 0.05, 0.0]], dtype=torch.float32, device=dev).expand(B, -1).contiguous()
            cam = camera_models[args.model](cams)
            grav = Gravity.from_rp(torch.full((B,), 0.1, device=dev), torch.full((B,), 0.2, device=dev))
            conf = torch.rand((B, H, W), generator=g).to(dev)
            pal = viz.resolve_palette("seismic", dev)
            heat = torch.flip(pal, (0,))
            pal_f = pal.float()

            def comparator():
                _, lat = get_perspective_field(cam, grav, use_up=False)                  # (B, 1, H, W) radians
                idx = ((lat[:, 0] * (180 / torch.pi) + 90) * (256 / 180)).long().clamp_(0, 255)
                col = pal_f[idx].permute(0, 3, 1, 2)
                return (img.float() * 0.6 + col * 0.4).round_().clamp_(0, 255).to(torch.uint8)

            variants = {
                "all layers": lambda: viz.draw_perspective_fields(img, cam, grav, horizon=True, up=True, confidence=conf, palette=pal,
                                                                  heat_palette=heat),
                "tint alone": lambda: viz.draw_perspective_fields(img, cam, grav, contours=False, palette=pal),
                "contours alone": lambda: viz.draw_perspective_fields(img, cam, grav, tint=False, palette=pal),
                "horizon alone": lambda: viz.draw_perspective_fields(img, cam, grav, tint=False, contours=False, horizon=True),
                "arrows alone": lambda: viz.draw_perspective_fields(img, cam, grav, tint=False, contours=False, up=True),
                "heat alone": lambda: viz.draw_perspective_fields(img, cam, grav, tint=False, contours=False, confidence=conf,
                                                                  heat_palette=heat),
                "no layer (copy)": lambda: viz.draw_perspective_fields(img, cam, grav, tint=False, contours=False),
                "torch tint comparator": comparator,
            }
            ms = {name: timed(fn, args.reps) for name, fn in variants.items()}
            for name, t in ms.items():
                lines.append({"what": "overlay_bench", "lib": os.path.basename(_lib.LIB_PATH), "model": args.model, "H": H, "W": W, "B": B, "variant": name,
                              "us_per_frame": round(1e3 * t / B, 2), "GBps": round(2 * B * H * W * 3 / (t * 1e-3) / 1e9, 1),
                              "comparator_over_this": round(ms["torch tint comparator"] / t, 2)})
                print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
