"""gclm_solve_recorded, gclm_calibrate_recorded, gclm_lm_backward and gclm_lm_backward_workspace at the C ABI: declared, exported,
bound; gclm_lm_backward refuses invalid arguments before any HIP call (fake device addresses, never dereferenced); the
workspace size; the record's layout constants; the kernels' resource usage (no scratch); and, on the GPU, the stage gate of
the backward -- the adjoint of ONE LM step against float64 autograd of lm_grad.lm_unrolled_torch -- and the canary check of
the planes and the workspace the call must not write.

The stage gate.  A record row is made by the recorded HIP solve of one step from a given state theta with a given damping
lambda; gclm_lm_backward then runs on that row with a given adjoint of the step's result.  The yardstick is float64 autograd
of lm_unrolled_torch(num_steps=1, init=theta, detach_init=False) from the same theta and lambda, so no trajectory is involved:
only the adjoint of a step.  A record of one row yields the step's input gradients (the first step's state adjoint is never
formed: the initial estimate takes none); a record of two rows, each from a state of its own, carries the state adjoint of
row 1 into row 0, whose input gradients are linear in it -- that checks the sum of d phi / d theta and the adjoint of [+].

States.  `normal`: the fixture's confidences, lambda = 0.1, a state near the fixture's solution; no lambda H_jj near its
clamp.  `clamp`: the confidences times 1e-7, so that H_jj is 1e-8 .. 1e-5 and the lambda that puts the 1e-6 clamp into the
widest gap of the sorted H_jj (their geometric mean; the gap is asserted to be at least 4x, so no rounding moves a column
across) is of order 1: columns on both sides of the clamp, and a damping term as large as the rest of phi, so a wrong mask
moves the gradients by O(1).  Every state is asserted to have up and latitude pixels on both sides of the Huber threshold and
none within 1e-4 of it (a pixel that changes sides between float32 and float64 changes rho'').

The bound is not taken from the code under test.  Per input, the unit is the larger of (a) the error of the SAME torch
composition run in float32 against its float64 run -- the yardstick's own float32 error, as the end-to-end gate uses the
reference's -- and (b) cond(A) x 2^-23 of the damped system A = H + D: the record holds A's words in float32, so v = A^-1
delta-bar is not determined more finely than that by any arithmetic downstream.  The gate is 4 units, the multiple the issue
starts from, in the norm of the end-to-end gate (per image: max-norm of the difference over max-norm of the float64 gradient).
Measured on an MI355X: 32 ratios (2 models x 2 states x {one row, two rows} x 4 inputs), at most 1.14, median 0.53."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from geocalib_amd import LMOptimizer, _lib, lm_grad
from geocalib_amd.camera import camera_models
from abi_harness import HEADER, assert_declared_exported_and_bound
from test_lm_grad_oracle import INPUTS, case_data, ref  # noqa: F401

F, I = "const float*", "int"
SOLVE = ["gclm_handle*", F, F, F, F, I, I, I, "float*", "float*", "float*", "float*", "void*"]
CALIBRATE = ["gclm_handle*", F, F, F, F, I, I, I, F, F, F, F, I, "float*", "float*", "float*", "float*", "void*"]
BACKWARD = [I, F, F, F, F, I, I, I, F, I, I, F, "float", "float", I, I, I, F, F, "float*", "float*", "float*", "float*", "void*",
            "size_t", "void*"]


def test_entry_points_are_declared_exported_and_bound():
    assert_declared_exported_and_bound("gclm_solve_recorded", SOLVE)
    assert_declared_exported_and_bound("gclm_calibrate_recorded", CALIBRATE)
    assert_declared_exported_and_bound("gclm_lm_backward", BACKWARD)
    assert assert_declared_exported_and_bound("gclm_lm_backward_workspace", [I] * 3, ret="size_t") == [C.c_int] * 3
    header = open(HEADER).read()
    changelog = header[header.index("ABI version:"):header.index("#define GCLM_VERSION")]
    assert all(n in changelog for n in ("gclm_solve_recorded", "gclm_calibrate_recorded", "gclm_lm_backward", "gclm_lm_backward_workspace"))
    assert f"#define GCLM_LM_RECORD_STRIDE {_lib.LM_RECORD_STRIDE}\n" in header
    R = lm_grad.RECORD
    for name, at in (("CAMERA", R["camera"].start), ("GRAVITY", R["gravity"].start), ("LAMBDA", R["lambda"]), ("DELTA", R["delta"].start),
                     ("FAILED", R["failed"]), ("EXECUTED", R["executed"]), ("SYSTEM", R["system"].start)):
        assert f"#define GCLM_LM_RECORD_{name} {at}\n" in header, name
    assert R["system"].stop == _lib.LM_RECORD_STRIDE


UP, LAT, UPC, LATC, REC, INFO = 0x4000000, 0x8000000, 0xC000000, 0x10000000, 0x14000000, 0x18000000
GCAM, GGRAV, GUP, GLAT, GUPC, GLATC, WS = 0x1C000000, 0x1D000000, 0x40000000, 0x50000000, 0x58000000, 0x60000000, 0x70000000
PX = 2 * 48 * 64 * 4
OK = dict(model=1, up=UP, lat=LAT, upc=UPC, latc=LATC, B=2, H=48, W=64, rec=REC, steps=10, early=1, info=INFO, us=1e-2, ls=1e-2,
          gcam=GCAM, ggrav=GGRAV, gup=GUP, glat=GLAT, gupc=GUPC, glatc=GLATC, ws=WS, ws_bytes=1 << 24)
BAD = [("radial", dict(model=2)), ("simple_divisional", dict(model=3)), ("model -1", dict(model=-1)), ("NULL latitude", dict(lat=None)),
       ("NULL record", dict(rec=None)), ("NULL camera gradient", dict(gcam=None)), ("NULL gravity gradient", dict(ggrav=None)),
       ("NULL workspace", dict(ws=None)), ("early stop without info", dict(info=None)), ("0 steps", dict(steps=0)),
       ("257 steps", dict(steps=257)), ("up scale 0", dict(us=0.0)), ("latitude scale NaN", dict(ls=float("nan"))),
       ("up gradient without up", dict(up=None, upc=None, gupc=None)), ("up confidence gradient without up", dict(up=None, gup=None)),
       ("up confidence gradient without the confidence", dict(upc=None)),
       ("latitude confidence gradient without the confidence", dict(latc=None)), ("B = 0", dict(B=0)), ("B > 65535", dict(B=65536)),
       ("H = 0", dict(H=0)), ("W = 0", dict(W=0)), ("workspace too small", dict(ws_bytes=1024)),
       ("workspace misaligned", dict(ws=WS + 4)), ("latitude misaligned", dict(lat=LAT + 2)), ("record misaligned", dict(rec=REC + 1)),
       ("up gradient misaligned", dict(gup=GUP + 2)), ("up gradient is up", dict(gup=UP)),
       ("latitude gradient overlaps the latitude", dict(glat=LAT + PX - 4)), ("confidence gradient overlaps the record", dict(gupc=REC - 4)),
       ("workspace overlaps the camera gradient", dict(ws=GCAM - 64)), ("the gradients overlap", dict(glatc=GLAT + PX - 4)),
       ("gradient overlaps the workspace", dict(glat=WS + 256))]


def _backward(a):
    return _lib.load().gclm_lm_backward(a["model"], a["up"], a["lat"], a["upc"], a["latc"], a["B"], a["H"], a["W"], a["rec"], a["steps"],
                                        a["early"], a["info"], a["us"], a["ls"], 1, 1, 1, a["gcam"], a["ggrav"], a["gup"], a["glat"],
                                        a["gupc"], a["glatc"], a["ws"], a["ws_bytes"], None)


@pytest.mark.parametrize("what,change", BAD, ids=[b[0] for b in BAD])
def test_invalid_arguments_are_refused_before_any_hip_call(what, change):
    assert _backward({**OK, **change}) == -3, what


def test_workspace_size_is_monotone_and_zero_for_invalid_sizes():
    ws = _lib.load().gclm_lm_backward_workspace
    assert 0 < ws(2, 48, 64) <= OK["ws_bytes"]
    for B, H, W in ((1, 1, 1), (7, 479, 641), (1024, 480, 640)):
        assert ws(B, H, W) <= ws(B + 1, H, W) and ws(B, H, W) <= ws(B, H + 1, W) <= ws(B, H + 1, W + 1)
    assert ws(1024, 480, 640) < 128 << 20
    for bad in ((0, 48, 64), (65536, 48, 64), (2, 0, 64), (2, 48, 0), (2, 65536, 32768), (2, 2 ** 31 - 1, 1)):
        assert ws(*bad) == 0, bad




def test_backward_kernels_carry_no_scratch(tmp_path):
    """Read from the code objects inside the built library, as tests/test_kernel_audit.py reads the sweeps': the flags are
    the build's own.  Three kernels, each for pinhole and simple_radial."""
    from test_kernel_audit import LLVM, SO, kernel_metadata
    if not (os.path.exists(SO) and os.path.exists(f"{LLVM}/llvm-readelf")):
        pytest.skip("library or LLVM tools missing")
    k = {n: v for n, v in kernel_metadata(tmp_path).items() if "lm_grad_" in n}
    for stem in ("prepare", "pixel", "finish"):
        assert len([n for n in k if f"lm_grad_{stem}_kernel" in n]) == 2, (stem, sorted(k))
    assert not any(v["scratch"] for v in k.values()), k


# ------------------------------------------------------------------------------------------ on the GPU: stage gate, canaries
HUBER = 3e-2          # the noise of the fixture's fields: pixels on both sides of the threshold in every state
GATE = 4.0
FLOAT32_EPS = 2.0 ** -23


def dev():
    return torch.device("cuda:0")


def per_image_err(got, want):
    dims = tuple(range(1, want.dim()))
    return (got - want).abs().amax(dim=dims) / want.abs().amax(dim=dims)


def step_conf(model, lam, steps=1):
    return {"camera_model": model, "num_steps": steps, "early_stop": False, "lambda_": float(lam), "loss_fn": "huber_loss",
            "up_loss_fn_scale": HUBER, "lat_loss_fn_scale": HUBER}


def stage_inputs(ref, model, image, conf_scale):
    """Image `image` of the fixture's 13 x 19 Huber case (ragged tiles both ways), float32 on the CPU; the confidences scaled
    in float32, so every run reads the same float32 words."""
    data = case_data(ref, f"c2/{model}/huber", torch.float32, "cpu", requires_grad=False)
    data = {k: data[k][image:image + 1].clone() for k in INPUTS}
    for k in ("up_confidence", "latitude_confidence"):
        data[k] = data[k] * torch.tensor(conf_scale, dtype=torch.float32)
    return data


def stage_state(ref, model, image, kind):
    """A float32 state (camera row, gravity) off the fixture's solution: `near` by 5 % of the focal length, 0.02 of k1 and
    about 2 degrees of gravity, `far` by 20 %, 0.05 and about 5 degrees."""
    f, dk, dg = {"near": (1.05, 0.02, 0.03), "far": (1.2, 0.05, 0.08)}[kind]
    cam = torch.from_numpy(ref[f"c2/{model}/huber/camera64"][image:image + 1]).float()
    grav = torch.from_numpy(ref[f"c2/{model}/huber/gravity64"][image:image + 1]).float()
    cam[:, 2:4] *= f
    if model != "pinhole":
        cam[:, 6:8] += dk
    grav = torch.nn.functional.normalize(grav + torch.tensor([[dg, -0.5 * dg, dg]]), dim=-1)
    return cam, grav


def oracle_step(model, inputs, cam, grav, lam, dtype, adj_cam, adj_grav):
    """One LM step of lm_unrolled_torch from (cam, grav) with damping `lam`, in `dtype`, and autograd of
    <adj_cam, camera+> + <adj_grav, gravity+>: ({input: gradient}, (gradient of the camera row, of the gravity), out).
    Keys of `inputs` other than the four fields (priors) are passed on as they are: they fix columns and take no gradient."""
    from geocalib_amd.lm_optimizer import _unit_gravity
    data = {k: (v.to(dtype).requires_grad_(True) if k in INPUTS else v) for k, v in inputs.items()}
    c, g = cam.to(dtype).requires_grad_(True), grav.to(dtype).requires_grad_(True)
    out = lm_grad.lm_unrolled_torch(data, step_conf(model, lam), dtype=dtype, init=(camera_models[model](c), _unit_gravity(g)),
                                    detach_init=False)
    loss = (out["camera"]._data * adj_cam.to(dtype)).sum() + (out["gravity"]._data * adj_grav.to(dtype)).sum()
    grads = torch.autograd.grad(loss, [data[k] for k in INPUTS] + [c, g])
    return dict(zip(INPUTS, (t.detach() for t in grads[:4]))), (grads[4].detach(), grads[5].detach()), out


def oracle_chain(model, inputs, rows, adj_cam, adj_grav, dtype):
    """The input gradients of a record of `rows` [(cam, grav, lam), ...]: the last row takes the given adjoint, each earlier
    one the state adjoint of the row after it; summed over the rows."""
    total, adj = None, (adj_cam, adj_grav)
    for cam, grav, lam in reversed(rows):
        grads, adj, _ = oracle_step(model, inputs, cam, grav, lam, dtype, *adj)
        total = grads if total is None else {k: total[k] + grads[k] for k in INPUTS}
    return total


def state_facts(model, inputs, cam, grav, lam):
    """In float64: (H_jj, cond of the damped system, (up, latitude) squared residuals over the squared Huber scale)."""
    out = oracle_step(model, inputs, cam, grav, lam, torch.float64, torch.zeros(1, 8), torch.zeros(1, 3))[2]
    H = out["hessians"][0, 0]
    A = H + torch.diag((H.diagonal() * lam).clamp(min=1e-6))
    from geocalib_amd.lm_optimizer import _unit_gravity
    model_f, _ = lm_grad.fields_and_jacobian(camera_models[model](cam.double()), _unit_gravity(grav.double()),
                                             tuple(inputs["latitude_field"].shape[-2:]))
    up = inputs["up_field"].double().permute(0, 2, 3, 1).reshape(1, -1, 2)
    sl = torch.sin(inputs["latitude_field"].double()).reshape(1, -1)
    x_up = ((up - model_f[..., :2]) ** 2).sum(-1) / HUBER ** 2
    x_lat = (sl - model_f[..., 2]) ** 2 / HUBER ** 2
    return H.diagonal(), torch.linalg.cond(A).item(), (x_up, x_lat)


def clamp_lambda(diag):
    """The damping that puts the 1e-6 clamp of lambda H_jj into the widest gap of the sorted H_jj, and that gap's ratio."""
    d = diag.sort().values
    ratio = d[1:] / d[:-1]
    i = int(ratio.argmax())
    return 1e-6 / float((d[i] * d[i + 1]).sqrt()), float(ratio[i])


def assert_both_huber_sides(xs, what):
    for name, x in zip(("up", "latitude"), xs):
        inl, outl = int((x <= 1).sum()), int((x > 1).sum())
        print(f"{what} {name}: {inl} inliers, {outl} outliers, closest to the threshold {float((x - 1).abs().min()):.2e}")
        assert inl >= 4 and outl >= 4, (what, name, inl, outl)
        assert float((x - 1).abs().min()) >= 1e-4, (what, name)


def hip_row(model, inputs, cam, grav, lam):
    """(optimizer, (1, 1, stride) record, result) of the recorded HIP solve of one step from (cam, grav) with damping `lam`;
    result: the (camera row, gravity) the step arrived at, on the CPU."""
    opt = LMOptimizer(step_conf(model, lam)).train()
    data = {k: v.to(dev()) for k, v in inputs.items()}
    from geocalib_amd.lm_optimizer import _unit_gravity
    init = (camera_models[model](cam.to(dev())), _unit_gravity(grav.to(dev())))      # the words as they are: no re-normalisation
    cam1, grav1, _, record = lm_grad.recorded_solve(opt, data, init=init)
    R = lm_grad.RECORD
    assert float(record[0, 0, R["lambda"]]) == float(np.float32(lam)) and float(record[0, 0, R["executed"]]) == 1.0
    assert float(record[0, 0, R["failed"]]) == 0.0
    return opt, record, (cam1._data.cpu(), grav1._data.cpu())


def row_state(record, i=0):
    """The state and damping the record's row says the step started from: what the oracle starts from."""
    R = lm_grad.RECORD
    r = record[:, i].cpu()
    return r[:, R["camera"]].clone(), r[:, R["gravity"]].clone(), float(r[0, R["lambda"]])


def hip_backward(opt, model, data, record, adj_cam, adj_grav, planes=None, workspace=None):
    """gclm_lm_backward on device tensors; `planes`: {input: caller-owned flat float32 buffer} (default: all four, fresh);
    `workspace`: a caller-owned uint8 buffer at least the required size.  Returns {input: gradient}."""
    from geocalib_amd import _call
    up, lat, upc, latc = (data[k].contiguous() for k in INPUTS)
    B, _, H, W = lat.shape
    if planes is None:
        planes = {k: torch.empty(data[k].numel(), dtype=torch.float32, device=dev()) for k in INPUTS}
    ws_bytes = int(_lib.load().gclm_lm_backward_workspace(B, H, W))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev()) if workspace is None else workspace
    info = torch.zeros((B, _lib.INFO_STRIDE), dtype=torch.float32, device=dev())
    record = record.contiguous()
    P = _call.ptr
    _call.call("gclm_lm_backward", _lib.CAMERA_MODEL_IDS[model], P(up), P(lat), P(upc), P(latc), B, H, W, record.data_ptr(),
               record.shape[1], 0, info.data_ptr(), HUBER, HUBER, int(opt.estimate_gravity), int(opt.estimate_focal),
               int(opt.estimate_dist), adj_cam.data_ptr(), adj_grav.data_ptr(), *(P(planes.get(k)) for k in INPUTS), ws.data_ptr(),
               ws_bytes, _call.raw_stream(dev()), device=dev())
    torch.cuda.synchronize()
    return {k: planes[k].reshape(data[k].shape) for k in INPUTS if k in planes}


def adjoint(model):
    """A fixed adjoint of a step's result: focal lengths, k1 (simple_radial) and gravity, nothing else."""
    cam = torch.zeros(1, 8)
    cam[0, 2], cam[0, 3] = 0.03, -0.05
    if model != "pinhole":
        cam[0, 6] = 0.7
    return cam, torch.tensor([[0.4, -0.2, 0.3]])


def gate(what, got, want64, want32, cond):
    floor = cond * FLOAT32_EPS
    worst = {}
    for k in INPUTS:
        err = per_image_err(got[k].cpu().double(), want64[k]).max().item()
        own = per_image_err(want32[k].double(), want64[k]).max().item()
        worst[k] = err / max(own, floor)
        print(f"{what} {k}: hip err {err:.3e}, torch float32 err {own:.3e}, cond(A) 2^-23 {floor:.3e}, ratio {worst[k]:.2f}")
    assert max(worst.values()) <= GATE, (what, worst)


STATES = {"normal": dict(conf_scale=1.0, image=0, kind="near"), "clamp": dict(conf_scale=1e-7, image=1, kind="far")}


def state_rows(ref, model, which, steps):
    """The inputs of state `which` and `steps` record rows on them: the last from the state itself (lambda 0.1, or the clamp
    lambda), an earlier one from the other kind of state (lambda 1, or its own clamp lambda)."""
    s = STATES[which]
    inputs = stage_inputs(ref, model, s["image"], s["conf_scale"])
    cam, grav = stage_state(ref, model, s["image"], s["kind"])
    lam = 0.1
    if which == "clamp":
        lam, gap = clamp_lambda(state_facts(model, inputs, cam, grav, 0.1)[0])
        assert gap >= 4.0 and 1e-6 <= lam <= 1e2, (lam, gap)
    rows = [(cam, grav, lam)]
    if steps == 2:
        other = "far" if s["kind"] == "near" else "near"
        cam0, grav0 = stage_state(ref, model, s["image"], other)
        lam0 = 1.0 if which == "normal" else clamp_lambda(state_facts(model, inputs, cam0, grav0, 0.1)[0])[0]
        rows.insert(0, (cam0, grav0, lam0))
    return inputs, rows


def hip_rows(model, inputs, rows):
    """The rows through the recorded HIP solve: (optimizer, (1, len(rows), stride) record, the rows as the record has them)."""
    made = [hip_row(model, inputs, *r)[:2] for r in rows]
    record = torch.cat([m[1] for m in made], dim=1).contiguous()
    return made[0][0], record, [row_state(record, i) for i in range(len(rows))]


@pytest.mark.gpu
@pytest.mark.parametrize("steps", [1, 2], ids=["inputs", "state_adjoint"])
@pytest.mark.parametrize("which", ["normal", "clamp"])
@pytest.mark.parametrize("model", ["pinhole", "simple_radial"])
def test_one_backward_step_against_float64_autograd(ref, model, which, steps):
    inputs, rows = state_rows(ref, model, which, steps)
    opt, record, rows = hip_rows(model, inputs, rows)
    conds = []
    for i, (cam, grav, lam) in enumerate(rows):
        diag, cond, xs = state_facts(model, inputs, cam, grav, lam)
        conds.append(cond)
        assert_both_huber_sides(xs, f"{model}/{which}/row{i}")
        clamped = diag * lam <= 1e-6
        print(f"{model}/{which}/row{i}: lambda {lam:.3e}, lambda H_jj {(diag * lam).tolist()}, cond(A) {cond:.3e}")
        assert float(((diag * lam).log() - np.log(1e-6)).abs().min()) >= np.log(2.0), "a lambda H_jj within 2x of the clamp"
        if which == "clamp" and i == len(rows) - 1:
            assert bool(clamped.any()) and not bool(clamped.all()), "a column on each side of the clamp"
    adj_cam, adj_grav = adjoint(model)
    want64 = oracle_chain(model, inputs, rows, adj_cam, adj_grav, torch.float64)
    want32 = oracle_chain(model, inputs, rows, adj_cam, adj_grav, torch.float32)
    data = {k: v.to(dev()) for k, v in inputs.items()}
    got = hip_backward(opt, model, data, record, adj_cam.to(dev()), adj_grav.to(dev()))
    gate(f"{model}/{which}/{steps}", got, want64, want32, max(conds))


@pytest.mark.gpu
def test_a_failed_step_hands_its_adjoint_on_and_adds_nothing(ref):
    """Row 1 starts where row 0 arrived and is marked as a failed Cholesky (the zero step): the gradients of the two-row
    record are those of row 0 alone under the same adjoint -- theta-bar = theta-bar+, nothing for the inputs.  (Only for such a
    chain: the adjoint of the zero step drops the adjoint's component along the gravity, to which the derivatives of the unit
    gravity row 0 arrived at are orthogonal.)  What differs is rounding of the adjoint handed on -- the float32 store of the
    direct term, the float32 norm of the gravity -- which v = A^-1 delta-bar of row 0 amplifies by cond(A) at most: the unit
    and the gate of the stage test."""
    model = "simple_radial"
    inputs, rows = state_rows(ref, model, "normal", 1)
    opt, row0, arrived = hip_row(model, inputs, *stage_state(ref, model, STATES["normal"]["image"], "far"), 1.0)
    _, row1, _ = hip_row(model, inputs, *arrived, 0.1)
    R = lm_grad.RECORD
    assert torch.equal(row1[0, 0, R["gravity"]].cpu(), arrived[1][0])
    record = torch.cat([row0, row1], dim=1).contiguous()
    record[:, 1, R["failed"]] = 1.0
    record[:, 1, R["delta"]] = 0.0
    cond = state_facts(model, inputs, *row_state(record, 0))[1]
    adj_cam, adj_grav = (t.to(dev()) for t in adjoint(model))
    data = {k: v.to(dev()) for k, v in inputs.items()}
    both = hip_backward(opt, model, data, record, adj_cam, adj_grav)
    alone = hip_backward(opt, model, data, record[:, :1], adj_cam, adj_grav)
    for k in INPUTS:
        err = per_image_err(both[k].double(), alone[k].double()).max().item()
        print(f"failed step {k}: {err:.3e} (unit {cond * FLOAT32_EPS:.3e})")
        assert err <= GATE * cond * FLOAT32_EPS, (k, err)


CANARY = -1.2345e30


@pytest.mark.gpu
def test_absent_planes_and_the_workspace_tail_are_never_written(ref):
    """The four gradient planes lie in ONE canary-filled buffer with gaps between them, the workspace in a canary-filled
    buffer longer than the call is told.  Whatever subset of the planes is passed: the planes that are passed hold the bits
    of the run with all four, and every other word -- the planes not passed, the gaps, the tail -- is still the canary."""
    name, model = "c2/simple_radial/huber", "simple_radial"
    from test_lm_grad_oracle import case_conf
    data = case_data(ref, name, torch.float32, dev(), requires_grad=False)
    opt = LMOptimizer(case_conf(ref, name)).train()
    _, _, _, record = lm_grad.recorded_solve(opt, dict(data))
    adj_cam, adj_grav = (torch.from_numpy(ref[f"{name}/{k}"]).float().to(dev()) for k in ("w_cam", "w_grav"))
    gap, at, where = 96, 96, {}
    for k in INPUTS:
        where[k] = slice(at, at + data[k].numel())
        at += data[k].numel() + gap
    B, _, H, W = data["latitude_field"].shape
    ws_bytes, tail = int(_lib.load().gclm_lm_backward_workspace(B, H, W)), 4096

    def run(wanted):
        buf = torch.full((at,), CANARY, dtype=torch.float32, device=dev())
        ws = torch.full((ws_bytes + tail,), 0xA5, dtype=torch.uint8, device=dev())
        out = hip_backward(opt, model, data, record, adj_cam, adj_grav, planes={k: buf[where[k]] for k in wanted}, workspace=ws)
        written = torch.zeros(at, dtype=torch.bool, device=dev())
        for k in wanted:
            written[where[k]] = True
        assert bool((buf[~written] == CANARY).all()), wanted
        assert bool((ws[ws_bytes:] == 0xA5).all()), wanted
        return {k: v.clone() for k, v in out.items()}

    full = run(INPUTS)
    for k in INPUTS:
        assert bool(torch.isfinite(full[k]).all()) and not bool((full[k] == CANARY).any()), k
    for wanted in (("up_field", "latitude_field"), ("up_confidence", "latitude_confidence"), ("latitude_field",), ("up_field",)):
        part = run(wanted)
        assert sorted(part) == sorted(wanted)
        for k in wanted:
            assert torch.equal(part[k].view(torch.int32), full[k].view(torch.int32)), (wanted, k)


@pytest.mark.gpu
def test_results_do_not_depend_on_what_the_workspace_held(ref):
    """gclm_lm_backward on the fixture's 13 x 19 case (ragged tiles both ways, ten recorded steps) with the caller's workspace
    holding 0x00 bytes, 0xFF bytes (NaN patterns), and the records of a call at 3 x 12 x 20: the same bits in all four planes."""
    from test_lm_grad_oracle import case_conf

    def prepared(name):
        data = case_data(ref, name, torch.float32, dev(), requires_grad=False)
        opt = LMOptimizer(case_conf(ref, name)).train()
        record = lm_grad.recorded_solve(opt, dict(data))[3]
        adj = [torch.from_numpy(ref[f"{name}/{k}"]).float().to(dev()) for k in ("w_cam", "w_grav")]
        B, _, H, W = data["latitude_field"].shape
        return (opt, name.split("/")[1], data, record, *adj), int(_lib.load().gclm_lm_backward_workspace(B, H, W))

    (case, need), (other, other_need) = prepared("c2/simple_radial/huber"), prepared("c1/simple_radial/huber")
    ws = torch.empty(max(need, other_need), dtype=torch.uint8, device=dev())
    runs = []
    for fill in (0x00, 0xFF, None):
        if fill is None:
            hip_backward(*other, workspace=ws)
        else:
            ws.fill_(fill)
        runs.append({k: v.clone() for k, v in hip_backward(*case, workspace=ws).items()})
    assert sorted(runs[0]) == sorted(INPUTS)
    for what, run in zip(("0xFF bytes", "another call's records"), runs[1:]):
        for k in INPUTS:
            assert torch.equal(run[k].view(torch.int32), runs[0][k].view(torch.int32)), (what, k)
