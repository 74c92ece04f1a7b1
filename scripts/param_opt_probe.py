"""GPU: PerspectiveParamOpt on the HIP path (gclm_param_opt) -- what one pass costs against the read probe, what a whole
default-conf solve costs, and what the composition it replaces costs.

Rows (one JSON object each, all in one process on the same device tensors; noisy pinhole fields, sigma 0.02):
    pass          gclm_param_opt_cost at B images of H x W: pose records, the pass over the three planes, the per-image sums
                  (three launches), hipEvent mean over --steps calls after --warmup
    read_probe    gclm_read_probe on the same three planes (12 B per pixel): the project's yardstick for a streaming kernel
    solve         PerspectiveParamOpt(default_conf) on the whole batch, host clock around a call that ends in a synchronise,
                  with poll_every 16 (the default) and 0 (all max_steps steps enqueued, no host synchronisation)
    solve_one     the same at B = 1: two launches per step, launch-bound
    torch_one     the reference's loop on one image on the device: the torch composition of get_perspective_field under
                  autograd, torch.optim.Adam, ReduceLROnPlateau and the two .item() round trips per step (baseline, not target)
A one-launch step (the last workgroup of an image doing its update) is not built; the row `one_launch_step` says so.

    python scripts/param_opt_probe.py [--shape 480x640] [--batch 1024] [--steps 20] [--out profiles/param_opt_probe.json]"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from geocalib_amd import Gravity, PerspectiveParamOpt, Pinhole, _lib, perspective_fields as pf  # noqa: E402
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


def wall(fn, repeats):
    """Host seconds of fn() followed by a synchronise: (best, all)."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts), ts, out


def make_fields(B, H, W, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    roll, pitch = (torch.rand(B, generator=g) - 0.5) * 1.2, (torch.rand(B, generator=g) - 0.5) * 1.2
    vfov = torch.deg2rad(40 + 50 * torch.rand(B, generator=g))
    size = torch.ones(B)
    cam = Pinhole.from_dict({"height": size * H, "width": size * W, "vfov": vfov}).to(dev)
    up, lat = pf.get_perspective_field(cam, Gravity.from_rp(roll, pitch).to(dev))
    gen = torch.Generator(device=dev).manual_seed(seed)
    up = torch.nn.functional.normalize(up + 0.02 * torch.randn(up.shape, device=dev, generator=gen), dim=1)
    lat = (lat + 0.02 * torch.randn(lat.shape, device=dev, generator=gen)).clamp(-math.pi / 2 + 1e-3, math.pi / 2 - 1e-3)
    return {"up_field": up.contiguous(), "latitude_field": lat.contiguous()}, torch.stack([roll, pitch, vfov], -1).to(dev)


def torch_reference_loop(data, conf):
    """The reference's optimize() on one image, from the same initial estimate, composed of torch ops on the device."""
    init = PerspectiveParamOpt({"max_steps": 1})(data)["initial"][0]
    H, W = data["latitude_field"].shape[-2:]
    params = [torch.nn.Parameter(init[k:k + 1].clone()) for k in range(3)]
    opt = torch.optim.Adam(params, lr=conf["lr"])
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", patience=3)
    size, window, steps = torch.ones(1, device=init.device), [], 0
    for _ in range(conf["max_steps"]):
        opt.zero_grad()
        cam = Pinhole.from_dict({"height": size * H, "width": size * W, "vfov": params[2]})
        up, lat = pf.get_perspective_field(cam, Gravity.from_rp(params[0], params[1]))
        lat_loss = (lat - data["latitude_field"]).abs().squeeze(1)
        up_loss = torch.acos(torch.clip(torch.nn.functional.cosine_similarity(up, data["up_field"], dim=1), -1 + 1e-7, 1 - 1e-7))
        loss = torch.mean(conf["lamb"] * lat_loss + (1 - conf["lamb"]) * up_loss)
        loss.backward()
        opt.step()
        sched.step(loss)
        steps += 1
        if loss.item() <= conf["abs_tol"]:
            break
        if len(window) < conf["patience"]:
            window.append(loss.item())
        elif abs(loss.item() - window[0]) < conf["rel_tol"]:
            break
        else:
            window = (window + [loss.item()])[-conf["patience"]:]
    return torch.cat([p.detach() for p in params]), steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="480x640")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "param_opt_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("param_opt_probe.py needs a GPU")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    H, W = (int(v) for v in args.shape.split("x"))
    B = args.batch
    data, truth = make_fields(B, H, W, dev)
    up, lat = data["up_field"], data["latitude_field"]
    px = B * H * W
    rows = []

    def emit(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    # the pass against the read probe
    ws_bytes = lib.gclm_param_opt_workspace(B, H, W)
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    out = torch.empty(B, 8, device=dev)
    rpv = (truth + torch.tensor([0.05, -0.04, 0.06], device=dev)).contiguous()

    def one_pass():
        assert lib.gclm_param_opt_cost(up.data_ptr(), lat.data_ptr(), rpv.data_ptr(), B, H, W, ws.data_ptr(), ws_bytes, out.data_ptr(),
                                       raw_stream(dev)) == 0

    planes = (ctypes.c_void_p * 3)(up.data_ptr(), up.data_ptr() + 4 * px, lat.data_ptr())

    def probe():
        assert lib.gclm_read_probe(planes, 3, px, raw_stream(dev)) == 0

    for rep in range(args.repeats):          # alternated: the two share whatever else the box is doing
        t_pass, t_probe = timed(one_pass, args.steps, args.warmup), timed(probe, args.steps, args.warmup)
        emit(path="pass", B=B, H=H, W=W, repeat=rep, ms=round(t_pass * 1e3, 4), read_TBps=round(12 * px / t_pass / 1e12, 3),
             of_read_probe=round(t_probe / t_pass, 3))
        emit(path="read_probe", B=B, H=H, W=W, repeat=rep, ms=round(t_probe * 1e3, 4), read_TBps=round(12 * px / t_probe / 1e12, 3))

    # whole solves
    for poll in (16, 0):
        opt = PerspectiveParamOpt({"poll_every": poll})
        best, ts, res = wall(lambda: opt(data), args.repeats)
        steps = res["steps"].float()
        miss = torch.rad2deg((res["rpv"] - truth).abs()).max(0).values
        emit(path="solve", B=B, H=H, W=W, poll_every=poll, s=round(best, 4), all_s=[round(t, 4) for t in ts], images_per_s=round(B / best, 1),
             converged=int(res["converged"].sum()), steps_mean=round(steps.mean().item(), 1), steps_max=int(steps.max()),
             worst_miss_deg=[round(v, 4) for v in miss.tolist()])
    one = {k: v[:1].contiguous() for k, v in data.items()}
    for poll in (16, 0):
        opt = PerspectiveParamOpt({"poll_every": poll})
        best, ts, res = wall(lambda: opt(one), args.repeats)
        emit(path="solve_one", B=1, H=H, W=W, poll_every=poll, ms=round(best * 1e3, 3), all_ms=[round(t * 1e3, 3) for t in ts],
             steps=int(res["steps"][0]), us_per_step_enqueued=round(best * 1e6 / (int(res["steps"][0]) if poll else 1000), 2))
    emit(path="one_launch_step", built=False, note="the step stays two launches (pass, per-image sums and update); not measured")

    # the composition it replaces, one image
    conf = {k: PerspectiveParamOpt.default_conf[k] for k in ("max_steps", "lr", "patience", "abs_tol", "rel_tol", "lamb")}
    t0 = time.perf_counter()
    ref, ref_steps = torch_reference_loop(one, conf)
    torch.cuda.synchronize()
    t_ref = time.perf_counter() - t0
    hip = PerspectiveParamOpt({})(one)
    emit(path="torch_one", B=1, H=H, W=W, s=round(t_ref, 3), steps=ref_steps, ms_per_step=round(t_ref * 1e3 / ref_steps, 3),
         hip_steps=int(hip["steps"][0]), max_abs_diff_deg=round(torch.rad2deg((ref - hip["rpv"][0]).abs().max()).item(), 5))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=0)


if __name__ == "__main__":
    main()
