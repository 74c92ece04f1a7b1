"""GPU: Camera.get_img_from_pano on the HIP path (gclm_render_from_pano) against the torch composition it replaces.

Rows per (panorama, n, resize):
  hip_kernel         one gclm_render_from_pano launch into a preallocated destination (kernel + launch)
  hip_method         the public method (rotations, the one size read, output allocation, and with --resize the resize)
  torch_grid_sample  F.grid_sample of the n images alone, the sampling grid built once outside the timed window
  torch_reference    the reference's whole composition: pixel grid, image2world, normalize, bearings @ gravity.R @ R_yaw,
                     two atan2, a norm, the grid affine and one grid_sample per image (and with --resize, the resize)
  resize_only        (with --resize) the bicubic / area resize of the panorama and its clamp, as the method runs it
Times are hipEvent means over --steps calls after --warmup.  "out_GBps" counts the destination written once, 4 C H W n
bytes (the panorama is gathered, so its traffic depends on the view).

    python scripts/pano_bench.py [--batches 1,16,64] [--panos 2048x4096,4096x8192] [--resize 1.0] [--steps 30]
Prints one JSON line per row.  Run once per library (GCLM_LIB_PATH) to compare builds in one session."""
import argparse
import ctypes
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from torch.nn import functional as F  # noqa: E402

from geocalib_amd import _lib, camera_models  # noqa: E402
from geocalib_amd.gravity import Gravity  # noqa: E402
from geocalib_amd._call import raw_stream as _raw_stream  # noqa: E402
from geocalib_amd.utils import rad2rotmat  # noqa: E402


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


def resized(pano, cam, h, rf):
    """The method's resize: one per distinct target shape (here one, every image shares the camera)."""
    Hp, Wp = pano.shape[-2:]
    scale = torch.pi / float(cam.vfov[0]) * float(h) / Hp * torch.tensor(rf, dtype=torch.float32)
    shape = (int(Hp * scale), int(Wp * scale))
    out = F.interpolate(pano, size=shape, mode="bicubic" if scale >= 1 else "area")
    return out.clamp(pano.min(), pano.max())


def torch_reference(cam, grav, yaws, pano, h, w, rf):
    """The reference's composition with this package's camera ops (camera.py:414-514 of the reference), which resizes the
    panorama once per image."""
    n = yaws.shape[0]
    srcs = [pano if rf is None else resized(pano, cam, h, rf) for _ in range(n)]
    uv1, _ = cam.image2world(cam.pixel_coordinates())
    b = cam.pixel_bearing_many(uv1) @ grav.R @ rad2rotmat(yaws.new_zeros(n), yaws.new_zeros(n), yaws)
    lon = torch.atan2(b[..., 0], b[..., 2])
    lat = torch.atan2(b[..., 1], torch.norm(b[..., [0, 2]], dim=-1))
    out = []
    for i, src in enumerate(srcs):
        Hs, Ws = src.shape[-2:]
        nx = (lon[i] + math.pi) / (2 * math.pi) * (Ws - 1.0)
        ny = (lat[i] + math.pi / 2) / math.pi * (Hs - 1.0)
        grid = torch.stack((nx.reshape(1, h, w), ny.reshape(1, h, w)), -1)
        grid = 2.0 * grid / torch.tensor([Ws - 1, Hs - 1], device=grid.device, dtype=grid.dtype) - 1
        out.append(F.grid_sample(src, grid, align_corners=True))
    return torch.cat(out, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--panos", default="2048x4096,4096x8192")
    ap.add_argument("--model", default="simple_radial")
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--resize", type=float, default=None, help="resize_factor of every image (default: no resize)")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pano_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    H, W, C, rf = args.height, args.width, args.channels, args.resize
    lib = _lib.load()
    mid = _lib.CAMERA_MODEL_IDS[args.model]
    data = torch.tensor([[W, H, 0.8 * W, 0.8 * W, W / 2 + 3.3, H / 2 - 2.1, -0.1, 0.0]], device=dev)
    cam = camera_models[args.model](data)
    for spec in args.panos.split(","):
        Hp, Wp = (int(v) for v in spec.split("x"))
        pano = torch.rand(1, C, Hp, Wp, device=dev)
        for n in (int(b) for b in args.batches.split(",")):
            yaws = torch.linspace(-math.pi, math.pi, n + 1, device=dev)[:n]
            grav = Gravity.from_rp(torch.full((1,), 0.05, device=dev), torch.full((1,), 0.2, device=dev))
            rot = (grav.R.reshape(-1, 3, 3) @ rad2rotmat(yaws.new_zeros(n), yaws.new_zeros(n), yaws)).contiguous()
            src = pano if rf is None else resized(pano, cam, H, rf)
            srcs = (ctypes.c_void_p * n)(*([src.data_ptr()] * n))
            hw = (ctypes.c_int * (2 * n))(*(list(src.shape[-2:]) * n))
            dst = torch.empty(n, C, H, W, device=dev)

            def kernel():
                r = lib.gclm_render_from_pano(mid, data.data_ptr(), 1, rot.data_ptr(), srcs, hw, n, C, H, W, dst.data_ptr(),
                                              _raw_stream(dev))
                assert r == 0, r

            rows = [("hip_kernel", timed(kernel, args.steps, args.warmup)),
                    ("hip_method", timed(lambda: cam.get_img_from_pano(pano[0], grav, yaws, rf), args.steps, args.warmup))]
            diff = None
            if rf is not None:
                rows.append(("resize_only", timed(lambda: resized(pano, cam, H, rf), args.steps, args.warmup)))
            if not args.skip_torch:
                uv1, _ = cam.image2world(cam.pixel_coordinates())
                b = cam.pixel_bearing_many(uv1) @ rot
                lon, lat = torch.atan2(b[..., 0], b[..., 2]), torch.atan2(b[..., 1], torch.norm(b[..., [0, 2]], dim=-1))
                grid = torch.stack((lon / math.pi, 2 * lat / math.pi), -1).reshape(n, H, W, 2)
                srcn = src.expand(n, -1, -1, -1)
                rows.append(("torch_grid_sample", timed(lambda: F.grid_sample(srcn, grid, align_corners=True),
                                                        args.steps, args.warmup)))
                rows.append(("torch_reference", timed(lambda: torch_reference(cam, grav, yaws, pano, H, W, rf),
                                                      max(3, args.steps // 3), 2)))
                diff = (torch_reference(cam, grav, yaws, pano, H, W, rf) - cam.get_img_from_pano(pano[0], grav, yaws, rf))
                diff = diff.abs().max().item()
            total = dict(rows)
            for path, t in rows:
                line = {"model": args.model, "pano": f"{Hp}x{Wp}", "n": n, "C": C, "H": H, "W": W, "resize": rf, "path": path,
                        "ms": round(t * 1e3, 4), "out_GBps": round(4 * C * H * W * n / t / 1e9, 1),
                        "max_abs_diff_vs_torch": diff, "lib": os.path.basename(_lib.LIB_PATH)}
                if path == "resize_only":
                    line["share_of_hip_method"] = round(t / total["hip_method"], 3)
                print(json.dumps(line), flush=True)
            del dst, src


if __name__ == "__main__":
    main()
