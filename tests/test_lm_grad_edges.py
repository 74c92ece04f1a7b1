"""gclm_lm_backward on the GPU where tests/test_lm_grad.py and tests/test_lm_grad_abi.py do not reach: the clamps of
theta [+] delta, the frozen-column plans (with a distortion model: the reference's overlap quirk), the tile walk beyond one
tile column and 32 tile records, and more than one block of the per-image kernel.  The yardsticks, units and gates are those
two files' own, imported, not restated:

  * end to end (frozen columns, tests/golden/lm_grad_frozen_reference.npz): the reference's float64 gradients, in units of
    the reference's own float32 error, ALLOWANCE = 8;
  * stage gate (one LM step from a given state; a record of one row, or of two rows with the state under test LAST, whose
    state adjoint row 0 receives): float64 autograd of lm_unrolled_torch(num_steps=1, init=row state, detach_init=False), in
    units of max(torch float32 run against its float64 run, cond(A) 2^-23), GATE = 4, per-image max-norm ratio.  Every row of
    every state: at least 4 pixels on either side of the Huber threshold in both fields, none within 1e-4 of it, no
    lambda H_jj within 2x of 1e-6, no failed Cholesky.

Stage states added here (Huber scale 3e-2; every record row is made by a real recorded HIP step, none is edited):

  clamp   13 x 19, fields rendered in float64 by the package's torch get_perspective_field from a seeded CPU generator with
          the fixture's noise recipe (0.03 on both fields, 5 % latitude outliers of 0.4 rad, confidences in 0.05 .. 0.95),
          cast to float32 once; seed 11 unless a state says otherwise.  The state starts short of the bound and the data lie
          beyond it, so the step crosses:
            focal_lo  data at vfov 154 deg, state at 148 deg, lambda 0.1   (bound: vfov 150 deg, fy 1.742)
            focal_hi  data at vfov 3 deg,   state at 5.5 deg, lambda 1e-3  (bound: vfov 5 deg, fy 148.9)
            k1_hi     data at k1 +0.85, state at +0.66, lambda 0.01        (bound +0.7)
            k1_lo     data at k1 -0.85, state at -0.66, lambda 0.01        (bound -0.7)
          Asserted, in the float64 oracle AND from the float32 record: fy exp(delta_f) at least 5 % beyond the bound, or
          k1 + delta_k at least 0.05 beyond +-0.7; and that the HIP step arrived exactly on the bound (the bound as float32
          torch's update_focal gives it; +-0.7 in float32).  The clamp zeroes a whole row of the adjoint of [+]: a backward
          that ignored it would move the gradients by O(1).
  frozen  the `normal` state of tests/test_lm_grad_abi.py with priors that hold the state's own focal length and/or gravity:
          simple_radial x {prior_focal, prior_gravity, both}, pinhole x {prior_focal, prior_gravity}.  In the two-row form the
          frozen quantity is the same in both rows (a frozen column does not move between steps).
  tile    `normal`-kind states (the ground truth off by 5 % focal length, 0.02 k1, about 2 degrees; lambda 0.1; row 0 of the
          two-row form: 20 %, 0.05, about 5 degrees, lambda 1) on rendered data of
            67 x 65   2 tile columns, the second one pixel wide; 17 tile rows, the last of 3 rows; 34 tiles, so chains 0 and 1
                      of the finish kernel's 32 take two records each;
            5 x 130   3 tile columns, the last 2 pixels wide; 2 tile rows, the last of one row.
          On these the state adjoint handed from row 1 to row 0 -- the finish kernel's sum over the tile records plus the
          direct term -- is also compared on its own, through what it does to row 0's planes: (planes of the two-row record)
          - (planes of row 1 alone) against the float64 oracle of row 0 under the oracle's own adjoint, same unit and gate.
  The set of stage states holds gravities with g_z of either sign (the pivot branch of gravity_plus): asserted.

More than 64 images (a second block of lm_grad_prepare_kernel, its b >= B guard): 66 images, bit for bit against B = 1."""
import math

import numpy as np
import pytest
import torch

from geocalib_amd import lm_grad
from geocalib_amd.camera import camera_models
from geocalib_amd.gravity import Gravity
from geocalib_amd.perspective_fields import get_perspective_field
from test_lm_grad import ALLOWANCE, gradients_against_reference_float64, recorded_solve_equals_plain_solve, run_grad
from test_lm_grad_abi import (GATE, HUBER, STATES, adjoint, assert_both_huber_sides, dev, gate, hip_backward, hip_row, oracle_chain,
                              oracle_step, row_state, stage_inputs, stage_state, state_facts)
from test_lm_grad_oracle import FROZEN_CASES, INPUTS, ref, ref_frozen  # noqa: F401

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ end to end, frozen columns
@pytest.mark.parametrize("name", FROZEN_CASES)
def test_recorded_solve_equals_plain_solve_frozen_columns(ref_frozen, name):
    recorded_solve_equals_plain_solve(ref_frozen, name)


@pytest.mark.parametrize("name", FROZEN_CASES)
def test_gradients_against_reference_float64_frozen_columns(ref_frozen, name):
    assert ALLOWANCE == 8.0
    gradients_against_reference_float64(ref_frozen, name)


# ------------------------------------------------------------------------------------------ stage gate: rendered data
SEED = 11


def rendered(model, hw, vfov, k1, roll, pitch, seed=SEED):
    """({input: (1, ., h, w) float32}, ground-truth camera row (1, 8) float64, gravity (1, 3) float64): fields of one camera
    rendered in float64 on the CPU, with the noise recipe of tests/golden/make_golden_lm_grad.py, cast to float32 once."""
    h, w = hw
    g = torch.Generator().manual_seed(seed)
    d = {"width": torch.tensor([float(w)]), "height": torch.tensor([float(h)]), "vfov": torch.tensor([vfov])}
    if model != "pinhole":
        d["k1"] = torch.tensor([k1])
    cam = camera_models[model].from_dict(d).double()
    grav = Gravity.from_rp(torch.tensor([roll]), torch.tensor([pitch])).double()
    up, lat = get_perspective_field(cam, grav)
    assert up.dtype is torch.float64 and not up.is_cuda
    up = up + 0.03 * torch.randn(up.shape, generator=g, dtype=torch.float64)
    lat = lat + 0.03 * torch.randn(lat.shape, generator=g, dtype=torch.float64)
    lat = lat + (torch.rand(1, h, w, generator=g) < 0.05)[:, None] * 0.4
    upc = 0.05 + 0.9 * torch.rand(1, h, w, generator=g, dtype=torch.float64)
    latc = 0.05 + 0.9 * torch.rand(1, h, w, generator=g, dtype=torch.float64)
    data = dict(up_field=up, latitude_field=lat, up_confidence=upc, latitude_confidence=latc)
    return {k: v.float() for k, v in data.items()}, cam._data.clone(), grav._data.clone()


def state_at(model, hw, vfov, k1, roll, pitch):
    """A float32 state (camera row, unit gravity); slots 6 and 7 of a simple_radial row are equal, as the solve keeps them."""
    d = {"width": torch.tensor([float(hw[1])]), "height": torch.tensor([float(hw[0])]), "vfov": torch.tensor([vfov])}
    cam = camera_models[model].from_dict(d)._data.double().clone()
    if model != "pinhole":
        cam[:, 6:8] = k1
    grav = Gravity.from_rp(torch.tensor([roll]), torch.tensor([pitch]))._data.double()
    return cam.float(), torch.nn.functional.normalize(grav, dim=-1).float()


def state_off(model, cam, grav, kind):
    """stage_state of tests/test_lm_grad_abi.py, off a given ground truth."""
    f, dk, dg = {"near": (1.05, 0.02, 0.03), "far": (1.2, 0.05, 0.08)}[kind]
    cam, grav = cam.float().clone(), grav.float().clone()
    cam[:, 2:4] *= f
    if model != "pinhole":
        cam[:, 6:8] = cam[:, 6:7] + dk             # slot 7 shadows k1
    return cam, torch.nn.functional.normalize(grav + torch.tensor([[dg, -0.5 * dg, dg]]), dim=-1)


DEG = math.pi / 180
# per clamp state: what the data are rendered at, where the state under test (the LAST row) starts and its lambda, and where
# row 0 of the two-row form starts (lambda 1: a short step that stays inside the bounds)
CLAMPS = {
    "focal_lo": dict(data=dict(vfov=154 * DEG, k1=0.0, roll=0.10, pitch=-0.17), last=dict(vfov=148 * DEG, k1=0.0, roll=0.12, pitch=-0.15),
                     lam=0.1, first=dict(vfov=140 * DEG, k1=0.0, roll=0.07, pitch=-0.20)),
    "focal_hi": dict(data=dict(vfov=3 * DEG, k1=0.0, roll=-0.15, pitch=0.22), last=dict(vfov=5.5 * DEG, k1=0.0, roll=-0.13, pitch=0.20),
                     lam=1e-3, first=dict(vfov=8 * DEG, k1=0.0, roll=-0.18, pitch=0.25)),
    "k1_hi": dict(data=dict(vfov=1.0, k1=0.85, roll=0.10, pitch=-0.17), last=dict(vfov=1.05, k1=0.66, roll=0.12, pitch=-0.15),
                  lam=0.01, first=dict(vfov=1.1, k1=0.55, roll=0.07, pitch=-0.20)),
    "k1_lo": dict(data=dict(vfov=1.0, k1=-0.85, roll=-0.15, pitch=0.22), last=dict(vfov=1.05, k1=-0.66, roll=-0.13, pitch=0.20),
                  lam=0.01, first=dict(vfov=1.1, k1=-0.55, roll=-0.18, pitch=0.25)),
}
# (focal_hi on pinhole alone: at a vfov of 3 degrees k1 is all but unobservable -- H_kk 5e-4, cond(A) 2e5 -- so with k1 free the
# unit cond(A) 2^-23 would be 2e-2, and lambda H_kk lies 2.06x from its clamp)
CLAMP_CASES = [("pinhole", "focal_lo"), ("pinhole", "focal_hi"), ("simple_radial", "focal_lo"), ("simple_radial", "k1_hi"),
               ("simple_radial", "k1_lo")]
CLAMP_HW = (13, 19)


def clamp_rows(model, which, steps):
    s = CLAMPS[which]
    inputs, _, _ = rendered(model, CLAMP_HW, **s["data"])
    rows = [(*state_at(model, CLAMP_HW, **s["last"]), s["lam"])]
    if steps == 2:
        rows.insert(0, (*state_at(model, CLAMP_HW, **s["first"]), 1.0))
    return inputs, rows


def focal_bounds(cam):
    """The bounds of fy for a float32 camera row, as float32 torch's update_focal arrives at them."""
    c = camera_models["pinhole"](cam[:, :6].float())
    return (float(c.update_focal(torch.full((1, 1), -30.0), as_log=True).f[0, 1]),
            float(c.update_focal(torch.full((1, 1), 30.0), as_log=True).f[0, 1]))


def unclamped(which, cam, delta_f, delta_k):
    """(what the step would have arrived at without the clamp, the bound, how far beyond it: a ratio for the focal length,
    a difference for k1; positive = beyond)."""
    lo, hi = focal_bounds(cam)
    if which == "focal_lo":
        pre = float(cam[0, 3]) * math.exp(delta_f)
        return pre, lo, 1 - pre / lo
    if which == "focal_hi":
        pre = float(cam[0, 3]) * math.exp(delta_f)
        return pre, hi, pre / hi - 1
    pre = float(cam[0, 6]) + delta_k
    return (pre, 0.7, pre - 0.7) if which == "k1_hi" else (pre, -0.7, -0.7 - pre)


def assert_clamp_active(what, which, model, inputs, row, record_row, arrived):
    """The last row's step crosses its bound by the asserted margin, in float64 and in the record, and the HIP step arrived on it."""
    cam, grav, lam = row
    out = oracle_step(model, inputs, cam, grav, lam, torch.float64, torch.zeros(1, 8), torch.zeros(1, 3))[2]
    d64 = out["deltas"][0, 0]                       # free columns: d1, d2, focal (, k1)
    d32 = record_row[lm_grad.RECORD["delta"]]       # full size: d1, d2, focal, k1, k2
    margin = 0.05
    for src, df, dk in (("float64 oracle", float(d64[2]), float(d64[3]) if model != "pinhole" else 0.0),
                        ("float32 record", float(d32[2]), float(d32[3]))):
        pre, bound, beyond = unclamped(which, cam, df, dk)
        print(f"{what}: {src}: unclamped {pre:.6g}, bound {bound:.6g}, beyond by {beyond:.3f}")
        assert beyond >= margin, (what, src, pre, bound)
    lo, hi = focal_bounds(cam)
    want = {"focal_lo": lo, "focal_hi": hi, "k1_hi": float(np.float32(0.7)), "k1_lo": float(np.float32(-0.7))}[which]
    got = float(arrived[0][0, 3 if which.startswith("focal") else 6])
    assert got == want, (what, got, want)
    assert float(out["camera"]._data.detach()[0, 3 if which.startswith("focal") else 6]) == pytest.approx(want, rel=1e-6), "the oracle clamps too"
    if model != "pinhole":
        assert float(arrived[0][0, 6]) == float(arrived[0][0, 7])


def run_stage(what, model, inputs, rows, last_row_check=None):
    """The stage gate of tests/test_lm_grad_abi.py on `rows` (the state under test last): every row through the recorded HIP
    solve, the existing conditions on every row, `last_row_check(row, its record row, where the step arrived)`, the gate.
    Returns what the adjoint comparison of the tile states needs."""
    made = [hip_row(model, inputs, *r) for r in rows]
    opt = made[0][0]
    record = torch.cat([m[1] for m in made], dim=1).contiguous()
    assert bool((record[..., lm_grad.RECORD["failed"]] == 0).all())
    rows = [row_state(record, i) for i in range(len(rows))]
    conds = []
    for i, (cam, grav, lam) in enumerate(rows):
        diag, cond, xs = state_facts(model, inputs, cam, grav, lam)
        conds.append(cond)
        assert_both_huber_sides(xs, f"{what}/row{i}")
        print(f"{what}/row{i}: lambda {lam:.3e}, lambda H_jj {(diag * lam).tolist()}, cond(A) {cond:.3e}, g_z {float(grav[0, 2]):+.3f}")
        assert float(((diag * lam).log() - np.log(1e-6)).abs().min()) >= np.log(2.0), "a lambda H_jj within 2x of the clamp"
        if model != "pinhole":
            assert float(cam[0, 6]) == float(cam[0, 7])
    if last_row_check is not None:
        last_row_check(rows[-1], record[0, -1].cpu(), made[-1][2])
    adj_cam, adj_grav = adjoint(model)
    want64 = oracle_chain(model, inputs, rows, adj_cam, adj_grav, torch.float64)
    want32 = oracle_chain(model, inputs, rows, adj_cam, adj_grav, torch.float32)
    data = {k: v.to(dev()) for k, v in inputs.items()}
    got = hip_backward(opt, model, data, record, adj_cam.to(dev()), adj_grav.to(dev()))
    gate(what, got, want64, want32, max(conds))
    return opt, data, record, rows, got, conds


@pytest.mark.parametrize("steps", [1, 2], ids=["inputs", "state_adjoint"])
@pytest.mark.parametrize("model,which", CLAMP_CASES, ids=[f"{m}-{w}" for m, w in CLAMP_CASES])
def test_one_backward_step_with_an_active_clamp(model, which, steps):
    inputs, rows = clamp_rows(model, which, steps)
    what = f"{model}/{which}/{steps}"
    run_stage(what, model, inputs, rows,
              lambda row, record_row, arrived: assert_clamp_active(what, which, model, inputs, row, record_row, arrived))


# ------------------------------------------------------------------------------------------ stage gate: frozen columns
FROZEN = [("simple_radial", ("prior_focal",)), ("simple_radial", ("prior_gravity",)), ("simple_radial", ("prior_focal", "prior_gravity")),
          ("pinhole", ("prior_focal",)), ("pinhole", ("prior_gravity",))]


def frozen_rows(ref, model, priors, steps):
    """The `normal` state with priors that hold its own focal length and / or gravity; row 0 of the two-row form is the `far`
    state with the frozen quantities of the state under test."""
    image = STATES["normal"]["image"]
    inputs = stage_inputs(ref, model, image, 1.0)
    cam, grav = stage_state(ref, model, image, "near")
    if "prior_focal" in priors:
        inputs["prior_focal"] = cam[:, 3].clone()
    if "prior_gravity" in priors:
        inputs["prior_gravity"] = grav.clone()
    rows = [(cam, grav, 0.1)]
    if steps == 2:
        cam0, grav0 = stage_state(ref, model, image, "far")
        if "prior_focal" in priors:
            cam0[:, 2:4] = cam[:, 2:4]
        if "prior_gravity" in priors:
            grav0 = grav.clone()
        rows.insert(0, (cam0, grav0, 1.0))
    return inputs, rows


@pytest.mark.parametrize("steps", [1, 2], ids=["inputs", "state_adjoint"])
@pytest.mark.parametrize("model,priors", FROZEN, ids=[f"{m}-{'+'.join(p)}" for m, p in FROZEN])
def test_one_backward_step_with_frozen_columns(ref, model, priors, steps):
    inputs, rows = frozen_rows(ref, model, priors, steps)
    what = f"{model}/{'+'.join(priors)}/{steps}"

    def frozen_stayed(row, record_row, arrived):
        cam, grav, _ = row          # (a frozen quantity takes the zero step: exp(log f + 0) and a renormalisation, a few ulps)
        if "prior_focal" in priors:
            assert torch.allclose(arrived[0][:, 2:4], cam[:, 2:4], rtol=4e-6, atol=0) and float(record_row[lm_grad.RECORD["delta"]][2]) == 0.0
        if "prior_gravity" in priors:
            assert torch.allclose(arrived[1], grav, rtol=0, atol=4e-7) and not bool(record_row[lm_grad.RECORD["delta"]][:2].any())
        if model != "pinhole":
            assert float(arrived[0][0, 6]) != float(cam[0, 6]), "k1 is free in every plan"

    opt = run_stage(what, model, inputs, rows, frozen_stayed)[0]
    assert (bool(opt.estimate_focal), bool(opt.estimate_gravity)) == ("prior_focal" not in priors, "prior_gravity" not in priors)


# ------------------------------------------------------------------------------------------ stage gate: the tile walk
# the first seed from 11 on at which no pixel of either row lies within 1.5e-4 of the Huber threshold (float64 facts)
TILE_SEEDS = {("pinhole", (67, 65)): 13, ("simple_radial", (67, 65)): 14, ("pinhole", (5, 130)): 11, ("simple_radial", (5, 130)): 11}
TILE_TRUTH = dict(vfov=1.0, k1=0.06, roll=-0.15, pitch=0.22)        # g_z > 0


def tile_rows(model, hw, steps):
    inputs, cam, grav = rendered(model, hw, seed=TILE_SEEDS[model, hw], **TILE_TRUTH)
    rows = [(*state_off(model, cam, grav, "near"), 0.1)]
    if steps == 2:
        rows.insert(0, (*state_off(model, cam, grav, "far"), 1.0))
    return inputs, rows


@pytest.mark.parametrize("steps", [1, 2], ids=["inputs", "state_adjoint"])
@pytest.mark.parametrize("hw", [(67, 65), (5, 130)], ids=["67x65", "5x130"])
@pytest.mark.parametrize("model", ["pinhole", "simple_radial"])
def test_one_backward_step_across_tiles(model, hw, steps):
    inputs, rows = tile_rows(model, hw, steps)
    what = f"{model}/{hw[0]}x{hw[1]}/{steps}"
    opt, data, record, rows, both, conds = run_stage(what, model, inputs, rows)
    if steps == 1:
        return
    # the state adjoint row 1 hands down, through row 0's planes: what the finish kernel summed over the tile records
    adj_cam, adj_grav = adjoint(model)
    alone = hip_backward(opt, model, data, record[:, 1:].contiguous(), adj_cam.to(dev()), adj_grav.to(dev()))
    got = {k: both[k] - alone[k] for k in INPUTS}
    want = {}
    for dtype in (torch.float64, torch.float32):
        handed = oracle_step(model, inputs, *rows[1], dtype, adj_cam, adj_grav)[1]
        want[dtype] = oracle_step(model, inputs, *rows[0], dtype, *handed)[0]
    gate(f"{what}/handed adjoint", got, want[torch.float64], want[torch.float32], max(conds))


def test_the_stage_states_hold_both_signs_of_g_z(ref):
    """The pivot branch of gravity_plus (g_z < 0: v = g_z - |g|, else -sigma / (g_z + |g|)).  The states' gravities are a
    matter of their construction, so this needs no run: the existing `normal` and `clamp` states, the clamp states' last rows
    and the tile states."""
    gz = {}
    for model in ("pinhole", "simple_radial"):
        for name, s in STATES.items():
            gz[f"{model}/{name}"] = float(stage_state(ref, model, s["image"], s["kind"])[1][0, 2])
        for which, s in CLAMPS.items():
            gz[f"{model}/{which}"] = float(state_at(model, CLAMP_HW, **s["last"])[1][0, 2])
        gz[f"{model}/tile"] = float(state_off(model, *rendered(model, (5, 130), **TILE_TRUTH)[1:], "near")[1][0, 2])
    print(gz)
    assert min(gz.values()) < -0.1 and max(gz.values()) > 0.1, gz


# ------------------------------------------------------------------------------------------ more than 64 images
def test_batch_independence_beyond_one_block_of_images(ref):
    """66 images -- image i % 3 of c1/simple_radial/huber with both confidences scaled in float32 by 0.5 + i / 132, so no two
    are equal -- in one differentiable solve: images 0, 63, 64 and 65 get the gradient planes, the camera and the gravity they
    get alone (B = 1), bit for bit.  lm_grad_prepare_kernel runs one thread per image in blocks of 64."""
    name, B = "c1/simple_radial/huber", 66

    def batch(data, wc, wg):
        index = torch.arange(B, device=dev()) % 3
        scale = (0.5 + torch.arange(B, dtype=torch.float32, device=dev()) / 132).reshape(B, 1, 1)
        data = {k: v[index].contiguous() for k, v in data.items()}
        for k in ("up_confidence", "latitude_confidence"):
            data[k] = data[k] * scale.reshape(B, *[1] * (data[k].dim() - 1))
        assert not torch.equal(data["up_confidence"][0], data["up_confidence"][3])
        return data, wc[index], wg[index]

    out, full = run_grad(ref, name, batch=batch)
    assert out["camera"]._data.shape[0] == B and full["up_field"].shape[0] == B
    for i in (0, 63, 64, 65):
        one_out, one = run_grad(ref, name, batch=batch, images=slice(i, i + 1))
        assert torch.equal(one_out["camera"]._data[0], out["camera"]._data[i]), i
        assert torch.equal(one_out["gravity"]._data[0], out["gravity"]._data[i]), i
        for k in INPUTS:
            assert torch.equal(one[k][0], full[k][i]), (i, k)
