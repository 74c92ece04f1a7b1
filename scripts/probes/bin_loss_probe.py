"""GPU box: the classification heads' loss (gclm_bin_loss / gclm_bin_loss_grad behind losses.perspective_bin_loss) at 73 + 180
bins, 320 x 480, B = 16 and 64, float32 and bfloat16 logits, with both confidences, timed with HIP events against two things on
the SAME tensors in the same process: gclm_read_probe over the buffers each pass moves (forward: the logits; backward: the
logits and the gradients -- the probe reads where the pass writes, 16-byte non-temporal loads and nothing else) and the eager
torch composition of the definition (get_perspective_field + the encoders + F.cross_entropy with the weighting, and autograd's
backward).  Peak memory of both, over what the inputs hold.  One child process per (B, dtype), under a time limit; inside it
every timing has its own deadline, polled on its end event, and a timing that misses it ends the process (exit status 124) --
nothing more is started on the device after that, here or in the parent.  Appends one JSON line per row.

usage: python scripts/probes/bin_loss_probe.py [--jsonl OUT] [--iters 10] [--batches 16,64]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
H, W, KU, KL = 320, 480, 73, 180
DEADLINE_S = 60.0          # per timing
CHILD_LIMIT_S = 300.0      # per (B, dtype)


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn, iters, what):
    """Mean milliseconds of `fn` over `iters` calls between two events, after two warm-up calls; the process ends if the end
    event has not arrived by the deadline."""
    import torch
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    end = time.monotonic() + DEADLINE_S
    while not e1.query():
        if time.monotonic() > end:
            print(f"bin_loss_probe: {what} missed its deadline of {DEADLINE_S} s", flush=True)
            os._exit(124)
        time.sleep(0.002)
    return e0.elapsed_time(e1) / iters


def child(dtype_name, B, iters):
    import math
    import torch
    import torch.nn.functional as F
    from geocalib_amd import Gravity, _call, _lib, fields, losses
    from geocalib_amd.camera import camera_models
    dev, dtype = torch.device("cuda:0"), getattr(torch, dtype_name)
    g = torch.Generator(device=dev).manual_seed(1)
    up = torch.empty((B, KU, H, W), dtype=dtype, device=dev)
    lat = torch.empty((B, KL, H, W), dtype=dtype, device=dev)
    for t in (up, lat):                                  # image by image: no float32 copy of the whole batch
        for b in range(B):
            t[b] = (3 * torch.randn(t.shape[1:], device=dev, generator=g)).to(dtype)
    conf = torch.rand((2, B, H, W), device=dev, generator=g) * 0.9 + 0.1
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(B, device=dev, generator=g)  # noqa: E731
    roll, pitch, vfov = u(-0.6, 0.6), u(-0.5, 0.5), u(0.5, 1.4)
    f, one = H / 2 / torch.tan(vfov / 2), torch.ones(B, device=dev)
    cam = torch.stack([W * one, H * one, f, f, W / 2 * one, H / 2 * one, u(-0.15, 0.15), 0 * one], -1).contiguous()
    grav = torch.stack([-torch.sin(roll) * torch.cos(pitch), -torch.cos(roll) * torch.cos(pitch), torch.sin(pitch)], -1).contiguous()
    camera, gravity = camera_models["simple_radial"](cam), Gravity(grav)
    gravity._data = grav
    inputs_bytes = torch.cuda.memory_allocated()

    # ---- the two kernels alone
    state = {}
    ms_fwd = timed(lambda: state.update(zip(("out", "lse", "bins"), fields.bin_loss("simple_radial", cam, grav, up, lat, conf[0], conf[1]))),
                   iters, "the forward")
    scale = (1.0 / state["out"][:, 1::3]).contiguous()
    ms_bwd = timed(lambda: state.update(zip(("g_up", "g_lat"), fields.bin_loss_grad(scale, state["lse"], state["bins"], up, lat, conf[0], conf[1]))),
                   iters, "the backward")
    lib, stream = _lib.load(), _call.raw_stream(dev)

    def read(tensors):
        for t in tensors:
            _lib.check(lib.gclm_read_probe((_lib.C.c_void_p * 1)(t.data_ptr()), 1, t.numel() * t.element_size() // 4, stream), None,
                       "gclm_read_probe")
    ms_read_fwd = timed(lambda: read((up, lat)), iters, "the read probe over the logits")
    ms_read_bwd = timed(lambda: read((up, lat, state["g_up"], state["g_lat"])), iters, "the read probe over the logits and the gradients")
    hip_loss = (state["out"][:, 0] / state["out"][:, 1] + state["out"][:, 3] / state["out"][:, 4]).double().cpu()
    g_up_hip = state["g_up"][0, :, ::37, ::41].double().cpu()
    state.clear()

    # ---- the public call, forward + backward, and its peak memory
    def public():
        zu, zl = up.detach().requires_grad_(True), lat.detach().requires_grad_(True)
        out = losses.perspective_bin_loss({"up_logits": zu, "latitude_logits": zl, "up_confidence": conf[0], "latitude_confidence": conf[1]},
                                          camera, gravity)
        out["perspective_total"].sum().backward()
        return out, zu.grad
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ms_public = timed(public, iters, "the public call")
    peak_hip = torch.cuda.max_memory_allocated() - inputs_bytes

    # ---- the eager composition on the same tensors
    from geocalib_amd import perspective_encoding as pe

    def eager():
        zu, zl = up.detach().requires_grad_(True), lat.detach().requires_grad_(True)
        t_up, t_lat = losses.perspective_target_bins(camera, gravity, KU, KL)
        total = 0
        for z, t, c in ((zu, t_up, conf[0]), (zl, t_lat, conf[1])):
            ce = F.cross_entropy(z.float(), t, reduction="none")
            total = total + (ce * c).sum((1, 2)) / c.sum((1, 2))
        total.sum().backward()
        return total.detach(), zu.grad
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ms_eager = timed(eager, max(iters // 3, 2), "the eager composition")
    peak_eager = torch.cuda.max_memory_allocated() - inputs_bytes
    eager_loss, eager_g_up = eager()
    rel = ((hip_loss - eager_loss.double().cpu()).abs() / eager_loss.double().cpu().abs()).max().item()
    gdiff = (g_up_hip - eager_g_up[0, :, ::37, ::41].double().cpu()).abs().max().item() / max(g_up_hip.abs().max().item(), 1e-300)
    nbytes = (up.numel() + lat.numel()) * up.element_size()
    r4 = lambda v: round(v, 4)  # noqa: E731
    print(json.dumps({"probe": "bin_loss_probe", "B": B, "h": H, "w": W, "up_bins": KU, "lat_bins": KL, "dtype": dtype_name, "iters": iters,
                      "forward_ms": r4(ms_fwd), "backward_ms": r4(ms_bwd), "read_probe_logits_ms": r4(ms_read_fwd),
                      "read_probe_logits_and_gradients_ms": r4(ms_read_bwd), "forward_over_read": r4(ms_fwd / ms_read_fwd),
                      "backward_over_read": r4(ms_bwd / ms_read_bwd), "public_forward_backward_ms": r4(ms_public),
                      "eager_forward_backward_ms": r4(ms_eager), "eager_over_public": round(ms_eager / ms_public, 2),
                      "logit_bytes": nbytes, "forward_TB_per_s": round(nbytes / ms_fwd / 1e9, 3),
                      "backward_TB_per_s": round(2 * nbytes / ms_bwd / 1e9, 3), "peak_bytes_public": peak_hip, "peak_bytes_eager": peak_eager,
                      "loss_rel_diff_to_eager": rel, "grad_maxnorm_diff_to_eager": gdiff, "nan": bool(math.isnan(rel))}), flush=True)


def main():
    iters = arg("--iters", 10)
    if "--child" in sys.argv:
        return child(sys.argv[sys.argv.index("--child") + 1], arg("--batch", 16), iters)
    out = arg("--jsonl", "")
    for B in (int(v) for v in arg("--batches", "16,64").split(",")):
        for dtype_name in ("float32", "bfloat16"):
            r = subprocess.run(["timeout", "-k", "10", str(int(CHILD_LIMIT_S)), sys.executable, os.path.abspath(__file__), "--child", dtype_name,
                                "--batch", str(B), "--iters", str(iters)], capture_output=True, text=True)
            sys.stderr.write(r.stderr[-2000:])
            if r.returncode != 0:
                print(r.stdout[-2000:])
                sys.exit(f"bin_loss_probe: the B = {B} {dtype_name} run ended with status {r.returncode}; nothing more is started")
            line = r.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            if out:
                os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
                with open(out, "a") as fh:
                    fh.write(line + "\n")


if __name__ == "__main__":
    main()
