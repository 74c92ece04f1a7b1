"""GPU: Camera.reproject_image on uint8 images (gclm_reproject_image_u8) against what a caller with a byte frame had to do
before it: convert to float32, run gclm_reproject_image, round and convert back.

Per (rotation, B) on the same device tensors, simple_radial source to its pinhole, 1080 x 1920, C = 3 by default; the
candidates ALTERNATE inside one process (every round times each of them once, the median over the rounds is reported):
  baseline_planar       img.float(), gclm_reproject_image, .round().clamp(0, 255).to(torch.uint8)
  baseline_interleaved  the same from a channels_last frame: the planar copy first
  float_kernel          the float kernel of the baseline alone, preallocated destination
  u8_kernel_planar      one gclm_reproject_image_u8 launch, interleaved = 0, preallocated destination
  u8_kernel_interleaved the same with interleaved = 1
  u8_method_planar      the public method on a contiguous uint8 image (allocates its output, reads the cameras' sizes once)
  u8_method_interleaved the public method on a channels_last uint8 image
  u8_c4_dwords          interleaved, C = 4, both images on a 4-byte boundary: a tap is one dword load, a pixel one dword store
  u8_c4_bytes           the same call on buffers one byte off the boundary: the byte path of the same kernel
Rotations: "identity" (NULL), "roll25" (a 25 deg roll removed), "level" ((-40, 30) deg levelled), as scripts/reproject_bench.py.
Times are hipEvent means over --steps calls, after --warmup calls of every candidate; GBps counts the byte image's algorithmic
traffic, one read and one write (2 B C H W bytes), over that time.

    python scripts/u8_image_bench.py [--shape 1080x1920] [--batches 1,16,64] [--rotations identity,roll25,level] [--run 1]
Prints one JSON line per (rotation, B, path); profiles/u8_image.jsonl holds the calls made (--run 1, --run 2, ...)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from geocalib_amd import _lib, camera_models  # noqa: E402
from geocalib_amd._call import raw_stream  # noqa: E402
from reproject_bench import rotation  # noqa: E402


def timed_once(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps          # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1080x1920", help="HxW")
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--model", default="simple_radial")
    ap.add_argument("--rotations", default="identity,roll25,level")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--run", type=int, default=1, help="a label for the lines of this call (the spread is taken between calls)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("u8_image_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    H, W = (int(v) for v in args.shape.split("x"))
    C, model = args.channels, args.model
    data = torch.tensor([[W, H, 0.8 * W, 0.81 * W, W / 2 + 3.3, H / 2 - 2.1, -0.2, 0.0]], device=dev)
    pin = torch.cat([data[:, :6], torch.zeros_like(data[:, 6:])], -1)
    cam, mid = camera_models[model](data), _lib.CAMERA_MODEL_IDS[model]
    for B in (int(b) for b in args.batches.split(",")):
        img = torch.randint(0, 256, (B, C, H, W), dtype=torch.uint8, device=dev)
        img_cl = img.contiguous(memory_format=torch.channels_last)
        dst, dst_cl = torch.empty_like(img), torch.empty_like(img_cl)
        fimg = img.float()
        fdst = torch.empty_like(fimg)
        n4 = B * 4 * H * W
        src4, dst4 = (torch.randint(0, 256, (n4 + 4,), dtype=torch.uint8, device=dev) for _ in range(2))
        for kind in args.rotations.split(","):
            rot = rotation(kind, dev)
            rp = None if rot is None else rot.data_ptr()

            def float_kernel(src=fimg):
                rc = lib.gclm_reproject_image(mid, data.data_ptr(), 0, pin.data_ptr(), 1, rp, 1, src.data_ptr(), B, C, H, W, H, W, H, W,
                                              fdst.data_ptr(), None, raw_stream(dev))
                assert rc == 0, rc

            def baseline(frame):
                float_kernel(frame.contiguous().float())
                return fdst.round().clamp(0, 255).to(torch.uint8)

            def u8_kernel(src, out, interleaved, channels=C):
                rc = lib.gclm_reproject_image_u8(mid, data.data_ptr(), 0, pin.data_ptr(), 1, rp, 1, src.data_ptr(), B, channels, H, W,
                                                 H, W, H, W, interleaved, out.data_ptr(), None, raw_stream(dev))
                assert rc == 0, rc

            paths = [("baseline_planar", lambda: baseline(img)), ("baseline_interleaved", lambda: baseline(img_cl)),
                     ("float_kernel", float_kernel), ("u8_kernel_planar", lambda: u8_kernel(img, dst, 0)),
                     ("u8_kernel_interleaved", lambda: u8_kernel(img_cl, dst_cl, 1)),
                     ("u8_method_planar", lambda: cam.reproject_image(img, rotation=rot)),
                     ("u8_method_interleaved", lambda: cam.reproject_image(img_cl, rotation=rot)),
                     ("u8_c4_dwords", lambda: u8_kernel(src4, dst4, 1, 4)), ("u8_c4_bytes", lambda: u8_kernel(src4[1:], dst4[1:], 1, 4))]
            for _, fn in paths:
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            ms = {name: [] for name, _ in paths}
            for _ in range(args.rounds):
                for name, fn in paths:
                    ms[name].append(timed_once(fn, args.steps))
            # the candidates computed the same image: the byte call against the rounded float kernel, and layout against layout
            u8_kernel(img, dst, 0)
            u8_kernel(img_cl, dst_cl, 1)
            off_float = (dst.int() - baseline(img).int()).abs().max().item()
            off_layout = (dst.int() - dst_cl.int()).abs().max().item()
            for name, _ in paths:
                t = statistics.median(ms[name])
                channels = 4 if name.startswith("u8_c4") else C
                print(json.dumps({"run": args.run, "model": model, "rotation": kind, "B": B, "C": channels, "H": H, "W": W, "path": name,
                                  "ms": round(t, 4), "ms_min": round(min(ms[name]), 4), "ms_max": round(max(ms[name]), 4),
                                  "GBps": round(2 * B * channels * H * W / t / 1e6, 1), "max_byte_diff_vs_rounded_float": off_float,
                                  "max_byte_diff_between_layouts": off_layout}), flush=True)
        del img, img_cl, dst, dst_cl, fimg, fdst, src4, dst4
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
