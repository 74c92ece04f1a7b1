"""-m gpu: every LM step of the HIP solve, per image, against a float64 oracle step from the SAME state.

For each configuration the solve runs with num_steps = k - 1 and with num_steps = k (same data, same handle knobs); one
float64 oracle step (oracle.solve(..., init=(camera, gravity, lambda))) from the (k - 1)-step state is compared with the
k-step state on every image through tests/test_step_oracle.py:step_gate -- |theta^HIP - theta^f64| <= tau_rel |delta^f64|
+ tau_floor per component (log focal, gravity, distortion).  One damped step is well conditioned (condition number of the
scaled system <= (P + lambda) / lambda), so nothing is amplified and no image is exempt.  The CPU test_step_gate_power
shows that this gate fails every image of a sweep that drops, mirrors or mis-signs one row or column.

Each configuration forces the path it names and asserts it was taken.  Worst measured ratios go to MEASURED."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from conftest import MEASURED
from test_gpu_parity import synth_device, to_np
from test_step_oracle import TAU_FLOOR, TAU_REL, div_k_allowance, step_gate

pytestmark = pytest.mark.gpu

ALL_MODELS = ("pinhole", "simple_radial", "radial", "simple_divisional")
FIXED_K = (1, 2, 3, 10, 20)
ADAPTIVE_K = (1, 2, 3)
COST_RTOL = 2e-6
COV_EPS = 1e-5          # covariance entries: COV_EPS x scaled condition number x sqrt(C_ii C_jj)
# simple_divisional's float32 formulas cancel (camera.py:913).  From k1 = 0 (the first step) its step meets the gate with
# the k allowance of test_step_oracle.div_k_allowance; from the second step on the float32 step itself -- the oracle's as
# much as HIP's -- misses the float64 one by up to ~1000x the gate on focal and gravity, and HIP's final cost by up to
# 1e-4 (12 % on one image of B = 416).  That is a limit of the model in float32, reported rather than built into the gate:
# simple_divisional is held to the step gate at k = 1 and to the initial cost, nothing later.
DIV_STEPS = (1,)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from geocalib_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _fields(model, B, H, W, seed=21, planes="all"):
    from oracle import synth
    data = synth.make_fields(seed, range(B), model, H, W)[0]
    if planes == "four":
        data.pop("up_confidence")
    elif planes == "latitude":
        data = {"latitude_field": data["latitude_field"], "latitude_confidence": data["latitude_confidence"]}
    return data


def _to_dev(data, dev, unaligned=False):
    out = {}
    for k, v in data.items():
        v = np.ascontiguousarray(v)
        if unaligned and v.ndim > 1:                 # a view one float into its allocation: not 16-byte aligned
            flat = torch.empty(v.size + 1, dtype=torch.float32, device=dev)
            flat[1:].copy_(torch.from_numpy(v.reshape(-1)))
            out[k] = flat[1:].view(v.shape)
        else:
            out[k] = torch.from_numpy(v).to(dev)
    return out


def hip_run(dev, conf, data_dev, steps, knobs, init=None):
    """One HIP solve of `steps` steps with the handle knobs forced; returns (cam, grav, info) as numpy and what the handle
    reports about the path it took."""
    from geocalib_amd import Gravity, LMOptimizer, _lib, camera_models
    lib = _lib.load()
    opt = LMOptimizer({**conf, "num_steps": steps, "early_stop": False}).eval()
    opt.row_pairs = knobs.get("row_pairs")
    opt.setup_optimization_and_priors(data_dev, shared_intrinsics=opt.shared_intrinsics)
    h = opt._handle(dev)
    for name, fn in (("slat", lib.gclm_set_slat_plane), ("fused", lib.gclm_set_fused_steps),
                     ("sweep_iters", lib.gclm_set_sweep_iters)):
        if name in knobs:
            _lib.check(fn(h.ptr, int(knobs[name])), h.ptr, name)
    _lib.check(lib.gclm_set_timing(h.ptr, 1), h.ptr, "gclm_set_timing")
    if init is None:
        opt(dict(data_dev))
    else:
        cam = camera_models[conf["camera_model"]](torch.from_numpy(init[0]).to(dev))
        opt.optimize(data_dev, cam, Gravity(torch.from_numpy(init[1]).to(dev)))
    torch.cuda.synchronize()
    assert opt._handle(dev) is h                    # the solve ran on the handle the knobs were set on
    n, ms = C.c_int(0), C.c_float(0)
    _lib.check(lib.gclm_last_pass_timing(h.ptr, C.byref(n), C.byref(ms)), h.ptr, "gclm_last_pass_timing")
    cam, grav, info = (t.cpu().numpy() for t in opt._last_raw)
    lat = data_dev["latitude_field"]
    B, _, H, W = lat.shape
    chunks = C.c_int(0)
    aligned = all(t.data_ptr() % 16 == 0 for t in data_dev.values() if t.dim() > 1)
    rows = C.c_int(0)
    _lib.check(lib.gclm_plan_cut(h.ptr, B, H, W, int(aligned), C.byref(rows), C.byref(chunks)), h.ptr, "gclm_plan_cut")
    return {"cam": cam, "grav": grav, "info": info, "launches": n.value, "slat_bytes": lib.gclm_slat_plane_bytes(h.ptr),
            "chunks": chunks.value, "rows": rows.value}


def _oracle_conf(conf):
    keep = ("camera_model", "shared_intrinsics", "lambda_", "fix_lambda", "use_log_focal", "use_spherical_manifold")
    return {k: conf[k] for k in keep if k in conf}


def _n_params(model, data):
    nd = {"pinhole": 0, "simple_radial": 1, "radial": 2, "simple_divisional": 1}[model]
    return 2 * ("prior_gravity" not in data) + ("prior_focal" not in data) + nd * ("prior_dist" not in data)


def _groups(conf, B):
    if not conf.get("shared_intrinsics"):
        return [np.arange(B)]
    gs = conf.get("group_size") or B
    return [np.arange(g, g + gs) for g in range(0, B, gs)]


def _oracle_step(oracle, conf, data, start, lam, precision, steps=1, training=True):
    """The oracle from the state `start` = (cam, grav), one call per shared-intrinsics group (a group is one arrow-head
    system; the HIP Schur step is checked against its dense solve)."""
    cam, grav = start
    outs = []
    for idx in _groups(conf, len(cam)):
        part = {k: (v[idx] if k not in ("scales",) else v) for k, v in data.items()}
        outs.append(oracle.solve(part, {**_oracle_conf(conf), "num_steps": steps, "early_stop": False}, precision=precision,
                                 training=training, init=(cam[idx], grav[idx], lam[idx])))
    return {k: np.concatenate([o[k] for o in outs]) for k in outs[0] if k != "trace"}


def check_steps(dev, oracle, label, conf, data, knobs=None, ks=FIXED_K, adaptive_ks=ADAPTIVE_K, init=None, unaligned=False,
                expect=None, gate_scale=None):
    """The step-ahead check of one configuration (fixed lambda at every k of `ks`, adaptive lambda at `adaptive_ks`), plus
    the initial / final costs and the covariance at HIP's own final state.  `expect(run)` asserts the path was taken.
    `gate_scale(start, lam)` -> (scale (B,), notes dict): a derived per-image factor on the gate (shared-intrinsics groups,
    tests/shared_gate.py), its notes recorded with the step."""
    knobs = dict(knobs or {})
    model = conf["camera_model"]
    if model == "simple_divisional":
        ks, adaptive_ks = tuple(k for k in ks if k in DIV_STEPS), tuple(k for k in adaptive_ks if k in DIV_STEPS)
    data_dev = _to_dev(data, dev, unaligned)
    P = _n_params(model, data)
    n_images = {}
    for fix in (True, False):
        kset = ks if fix else adaptive_ks
        if not kset:
            continue
        c = {**conf, "fix_lambda": fix}
        runs = {s: hip_run(dev, c, data_dev, s, knobs, init) for s in sorted({k - 1 for k in kset} | set(kset))}
        if expect is not None:
            for s, r in runs.items():
                expect(r, s)
        for k in kset:
            r0, r1 = runs[k - 1], runs[k]
            lam = r0["info"][:, 13].copy()          # the lambda step k uses: the rule's value after step k - 1
            start = (r0["cam"], r0["grav"])
            ref64 = _oracle_step(oracle, c, data, start, lam, "f64")
            extra = None
            if model == "simple_divisional":
                extra = div_k_allowance(model, _oracle_step(oracle, c, data, start, lam, "f32"), ref64)
            scale = 1.0
            if not fix:          # adaptive lambda: the bound on the step's amplification, (P + lambda) / lambda, scales the gate
                scale = ((P + lam) / lam)[:, None]
            notes = {}
            if gate_scale is not None:
                g, notes = gate_scale(start, lam)
                scale = scale * g[:, None]
            ratio = step_gate(model, start, (r1["cam"], r1["grav"]), (ref64["camera"], ref64["gravity"]),
                              TAU_REL * scale, TAU_FLOOR * scale, extra)
            tag = f"step/{label}/{'fix' if fix else 'adaptive'}/k{k}"
            MEASURED[tag] = {"worst_ratio": ratio.max(0).tolist(), "images": int(len(ratio)), **notes}
            n_images[tag] = len(ratio)
            assert np.isfinite(ratio).all() and (ratio <= 1).all(), (tag, ratio.max(0), np.argwhere(ratio > 1)[:8])
            # images whose damped float64 system is not positive definite are exactly those whose HIP step failed
            hip_failed = r1["info"][:, 14] > r0["info"][:, 14]
            assert np.array_equal(hip_failed, ref64["step_failures"] > 0), (tag, hip_failed, ref64["step_failures"])
        # costs at HIP's own states: the initial cost (sweep 1) and the final cost of the longest run, and the covariance
        last = runs[max(kset)]
        at0 = _oracle_step(oracle, c, data, (runs[0]["cam"], runs[0]["grav"]), runs[0]["info"][:, 13], "f64", steps=0)
        e0 = np.abs(last["info"][:, 3] / at0["final_cost"] - 1)
        tag = f"final/{label}/{'fix' if fix else 'adaptive'}"
        if model == "simple_divisional":          # the initial state only (DIV_STEPS)
            MEASURED[tag] = {"initial_cost": float(e0.max())}
            assert (e0 <= COST_RTOL).all(), (tag, e0.max())
            continue
        atK = _oracle_step(oracle, c, data, (last["cam"], last["grav"]), last["info"][:, 13], "f64", steps=0, training=False)
        eK = np.abs(last["info"][:, 6] / atK["final_cost"] - 1)
        Cr = atK["covariance"].astype(np.float64)
        Pc = int(last["info"][0, 12])                 # the covariance keeps the distortion columns under a prior_dist
        assert Cr.shape[1] == Pc, (Cr.shape, Pc)
        Ch = last["info"][:, 16:16 + Pc * Pc].reshape(-1, Pc, Pc).astype(np.float64)
        Hr = np.linalg.inv(Cr)
        d = 1 / np.sqrt(np.abs(np.einsum("bii->bi", Hr)))
        kappa = np.linalg.cond(Hr * d[:, :, None] * d[:, None, :])
        sd = np.sqrt(np.abs(np.einsum("bii->bi", Cr)))
        ecov = (np.abs(Ch - Cr) / (sd[:, :, None] * sd[:, None, :])).max((1, 2)) / kappa
        MEASURED[tag] = {"initial_cost": float(e0.max()), "final_cost": float(eK.max()), "cov_over_kappa": float(ecov.max()),
                         "kappa_max": float(kappa.max())}
        assert (e0 <= COST_RTOL).all() and (eK <= COST_RTOL).all(), (tag, e0.max(), eK.max())
        assert (ecov <= COV_EPS).all(), (tag, ecov.max(), kappa.max())
    return n_images


# ------------------------------------------------------------------ the four models in their three launch forms

SHAPE = (120, 160)


def _expect_slat(on):
    def f(r, steps):
        if steps >= 1:
            assert (r["slat_bytes"] > 0) == on, r["slat_bytes"]
    return f


def _expect_fused(r, steps):
    # the one-launch-per-step path declines the scratch plane even when it is forced on (gclm_api.hip: make_plan), and
    # issues one sweep launch per step plus the final one
    assert r["slat_bytes"] == 0 and r["launches"] == steps + 1, (r["slat_bytes"], r["launches"])


@pytest.mark.parametrize("model", ALL_MODELS)
@pytest.mark.parametrize("form", ["slat_on", "slat_off", "fused_B1", "fused_B4"])
def test_step_parity_launch_forms(dev, oracle, model, form):
    B = 1 if form == "fused_B1" else 4
    data = _fields(model, B, *SHAPE)
    if form.startswith("fused"):
        knobs, expect = {"fused": 1, "slat": 1, "row_pairs": False}, _expect_fused
    else:
        on = form == "slat_on"
        knobs, expect = {"fused": 0, "slat": int(on), "row_pairs": False}, _expect_slat(on)
    check_steps(dev, oracle, f"{model}/{form}", {"camera_model": model}, data, knobs, expect=expect)


# ------------------------------------------------------------------ radial / simple_divisional variants

@pytest.mark.parametrize("model", ["radial", "simple_divisional"])
@pytest.mark.parametrize("variant", ["row_pairs_on", "row_pairs_off", "linear_focal", "explicit_camera", "scales"])
def test_step_parity_radial_variants(dev, oracle, model, variant):
    B = 4
    data = _fields(model, B, *SHAPE)
    conf = {"camera_model": model}
    knobs = {"fused": 0, "row_pairs": variant == "row_pairs_on"}
    init = None
    if variant == "linear_focal":
        conf["use_log_focal"] = False
    if variant == "scales":
        data["scales"] = np.array([1.25, 1.0], np.float32)
    if variant == "explicit_camera":
        # the SHARE = false walk: a principal point off the centre, handed to optimize() (gclm_solve); row pairs forced
        H, W = SHAPE
        cam = np.tile(np.array([W, H, 0.8 * W, 0.8 * W, W / 2 + 7.5, H / 2 - 4.25, 0.0, 0.0], np.float32), (B, 1))
        grav = np.tile(np.array([0.0, -1.0, 0.0], np.float32), (B, 1))
        init, knobs["row_pairs"] = (cam, grav), True
    check_steps(dev, oracle, f"{model}/{variant}", conf, data, knobs, init=init)
    if variant == "explicit_camera":
        # the pair walk ran on the off-centre camera (its sums differ from the one-row walk's in the last bits); that it
        # did not share r2 across the pair is what the step gate above checks
        data_dev = _to_dev(data, dev)
        a = hip_run(dev, {**conf, "fix_lambda": True}, data_dev, 20, knobs, init)
        b = hip_run(dev, {**conf, "fix_lambda": True}, data_dev, 20, {**knobs, "row_pairs": False}, init)
        assert not np.array_equal(a["info"][:, 6], b["info"][:, 6])
    if variant == "row_pairs_on":
        # the row-pair walk was taken: its sums differ from the one-row walk's in the last bits
        data_dev = _to_dev(data, dev)
        a = hip_run(dev, {**conf, "fix_lambda": True}, data_dev, 20, {"fused": 0, "row_pairs": True})
        b = hip_run(dev, {**conf, "fix_lambda": True}, data_dev, 20, {"fused": 0, "row_pairs": False})
        assert not np.array_equal(a["info"][:, 6], b["info"][:, 6])


# ------------------------------------------------------------------ shapes and sweep cuts

SHAPES = {"w318": (96, 318), "unaligned": (96, 128), "h231": (231, 320), "ragged": (230, 324), "strips": (64, 2600),
          "tiny": (6, 8), "iters1": SHAPE, "iters64": (480, 640)}


@pytest.mark.parametrize("model", ["simple_radial", "radial"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_step_parity_shapes(dev, oracle, model, name):
    H, W = SHAPES[name]
    # (the library halves the iterations while a launch has fewer than 2048 workgroups: 64 only takes effect on a batch)
    data = _fields(model, 64 if name == "iters64" else 3, H, W)
    knobs = {}
    if name.startswith("iters"):
        knobs["sweep_iters"] = int(name[5:])

    default = None
    if name.startswith("iters"):          # the knob changed the cut: another number of rows per workgroup chunk
        default = hip_run(dev, {"camera_model": model, "fix_lambda": True}, _to_dev(data, dev), 0, {})["rows"]

    def expect(r, steps):
        if name in ("strips", "ragged", "h231"):
            assert r["chunks"] > 1, r["chunks"]
        if default is not None:
            assert r["rows"] != default, (r["rows"], default)
    check_steps(dev, oracle, f"{model}/{name}", {"camera_model": model}, data, knobs, unaligned=name == "unaligned",
                expect=expect, adaptive_ks=())


# ------------------------------------------------------------------ fewer inputs, priors

@pytest.mark.parametrize("model", ["pinhole", "radial"])
@pytest.mark.parametrize("planes", ["four", "latitude"])
def test_step_parity_fewer_planes(dev, oracle, model, planes):
    data = _fields(model, 3, *SHAPE, planes=planes)

    def expect(r, steps):             # the scratch plane needs all five planes: a sweep over fewer reads latitude itself
        assert r["slat_bytes"] == 0, r["slat_bytes"]
    check_steps(dev, oracle, f"{model}/{planes}", {"camera_model": model}, data, {"slat": 1}, adaptive_ks=(), expect=expect)


@pytest.mark.parametrize("model", ["simple_radial", "radial"])          # PM = 4 and PM = 5
@pytest.mark.parametrize("priors", ["focal", "gravity", "dist", "focal+dist"])
def test_step_parity_priors(dev, oracle, model, priors):
    from oracle import synth
    B = 3
    data = _fields(model, B, *SHAPE)
    gt = [synth.gt_params(21, i, model, *SHAPE) for i in range(B)]
    if "focal" in priors:
        data["prior_focal"] = np.array([1.1 * g[0][3] for g in gt], np.float32)
    if "gravity" in priors:
        data["prior_gravity"] = np.stack([g[1] + [0.02, -0.01, 0.03] for g in gt]).astype(np.float32)
    if "dist" in priors:
        nd = 2 if model == "radial" else 1
        data["prior_dist"] = np.stack([g[0][6:6 + nd] * 0.9 for g in gt]).astype(np.float32)
    P = _n_params(model, data)
    assert 2 <= P <= 4, P
    check_steps(dev, oracle, f"{model}/prior_{priors}", {"camera_model": model}, data, adaptive_ks=())


# ------------------------------------------------------------------ shared intrinsics

@pytest.mark.parametrize("model", ["pinhole", "simple_radial", "radial"])
@pytest.mark.parametrize("groups", ["16", "batch"])
def test_step_parity_shared_intrinsics(dev, oracle, model, groups):
    from oracle import synth
    H, W = 64, 96
    parts = [synth.make_shared_group(21, g, model, H, W)[0] for g in range(2)]
    data = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    conf = {"camera_model": model, "shared_intrinsics": True, "group_size": 16 if groups == "16" else None}
    check_steps(dev, oracle, f"{model}/shared_{groups}", conf, data, adaptive_ks=())


@pytest.mark.parametrize("model", ["pinhole", "simple_radial"])
def test_step_parity_shared_split_two_virtual_ranks(dev, oracle, model):
    """The SharedIntrinsicsSplit protocol: every group's frames dealt to two handles ("ranks") whose Schur partials are
    summed per step (test_gpu_parity.run_virtual_ranks).  Each step of the assembled batch against the float64 dense
    arrow-head step of each group."""
    from test_gpu_parity import run_virtual_ranks
    G, gs, H, W = 4, 8, 48, 64
    data_dev, _, _ = synth_device(model, G * gs, H, W, dev, seed=3, group_size=gs)
    data = {k: v.cpu().numpy() for k, v in data_dev.items()}
    conf = {"camera_model": model, "shared_intrinsics": True, "group_size": gs, "fix_lambda": True}
    frames = torch.arange(G * gs, device=dev)
    sels = [frames[(frames % gs) // (gs // 2) == r] for r in range(2)]
    gofs = [torch.arange(sel.numel(), device=dev, dtype=torch.int32) // (gs // 2) for sel in sels]
    runs = {}
    for steps in sorted({k - 1 for k in FIXED_K} | set(FIXED_K)):
        res = run_virtual_ranks(dev, {**conf, "num_steps": steps, "early_stop": False}, data_dev, sels, gofs, G, H, W)
        cam, grav = np.zeros((G * gs, 8), np.float32), np.zeros((G * gs, 3), np.float32)
        info = np.zeros((G * gs, res[0][2].shape[1]), np.float32)
        for (c, g, i, _), sel in zip(res, sels):
            sel = sel.cpu().numpy()
            cam[sel], grav[sel], info[sel] = c, g, i
        runs[steps] = (cam, grav, info)
    for k in FIXED_K:
        (c0, g0, i0), (c1, g1, _) = runs[k - 1], runs[k]
        ref64 = _oracle_step(oracle, conf, data, (c0, g0), np.full(G * gs, 0.1, np.float32), "f64")
        ratio = step_gate(model, (c0, g0), (c1, g1), (ref64["camera"], ref64["gravity"]))
        tag = f"step/{model}/shared_split/fix/k{k}"
        MEASURED[tag] = {"worst_ratio": ratio.max(0).tolist(), "images": int(len(ratio))}
        assert (ratio <= 1).all(), (tag, ratio.max(0))


# ------------------------------------------------------------------ the library's own choices at batch scale

@pytest.mark.parametrize("model,B", [("radial", 416), ("simple_divisional", 416), ("pinhole", 64), ("simple_radial", 64)])
def test_step_parity_batch_scale(dev, oracle, model, B):
    """Every image of the batch, with every knob left to the library (auto row pairs and the scratch plane for the
    distortion models)."""
    data_dev, _, _ = synth_device(model, B, 480, 640, dev, seed=5)
    data = {k: v.cpu().numpy() for k, v in data_dev.items()}
    del data_dev

    def expect(r, steps):
        assert r["chunks"] > 1
        if model in ("radial", "simple_divisional") and steps >= 1:
            assert r["slat_bytes"] > 0
    n = check_steps(dev, oracle, f"{model}/B{B}", {"camera_model": model}, data, expect=expect)
    assert all(v == B for v in n.values()), n
    if model in ("radial", "simple_divisional"):
        # the library chose row pairs: the forced one-row walk gives other bits
        sub = {k: torch.from_numpy(v).to(dev) for k, v in data.items()}
        a = hip_run(dev, {"camera_model": model, "fix_lambda": True}, sub, 2, {})
        b = hip_run(dev, {"camera_model": model, "fix_lambda": True}, sub, 2, {"row_pairs": False})
        assert not np.array_equal(a["info"][:, 6], b["info"][:, 6])


# ------------------------------------------------------------------ gclm_system over seeded, non-converged states

def _random_states(model, B, H, W, seed):
    rng = np.random.default_rng(seed)
    roll, pitch = np.deg2rad(rng.uniform(-80, 80, B)), np.deg2rad(rng.uniform(-80, 80, B))
    vfov = np.deg2rad(rng.uniform(15, 140, B))
    f = H / 2 / np.tan(vfov / 2)
    lo, hi = {"pinhole": (0, 0), "simple_radial": (-0.69, 0.69), "radial": (-0.69, 0.69),
              "simple_divisional": (-2.95, 2.95)}[model]
    k1 = rng.uniform(lo, hi, B)
    k1[:2] = (lo, hi)                                          # at the clamps (update_dist: +-0.7, +-3)
    k2 = rng.uniform(-0.1, 0.1, B) if model == "radial" else np.zeros(B)
    cx, cy = W / 2 + rng.uniform(-0.1, 0.1, B) * W, H / 2 + rng.uniform(-0.1, 0.1, B) * H
    cam = np.stack([np.full(B, W), np.full(B, H), f, f, cx, cy, k1, k2], 1).astype(np.float32)
    sr, cr, sp, cp = np.sin(roll), np.cos(roll), np.sin(pitch), np.cos(pitch)
    grav = np.stack([-sr * cp, -cr * cp, sp], 1).astype(np.float32)
    return cam, grav


def _ulp_spread(oracle, data, cam, grav, conf, as_rpf, ref):
    """How far the float64 system moves when one input of the float32 state (fx, fy, cx, cy, k1, k2, gravity) moves by one
    float32 ulp, per entry (worst over inputs and both directions).  An entry that a 1-ulp change of the state moves by
    more than the gate cannot be held to it by any float32 evaluation: u = (x - cx) / fx rounds at that level already."""
    spread = {"H": np.zeros_like(ref["H"]), "G": np.zeros_like(ref["G"])}
    for arr, cols in ((cam, range(2, 8)), (grav, range(3))):
        for j in cols:
            for to in (np.inf, -np.inf):
                moved = arr.copy()
                moved[:, j] = np.nextafter(moved[:, j], np.float32(to))
                c2, g2 = (moved, grav) if arr is cam else (cam, moved)
                r = oracle.system(data, c2, g2, conf, as_rpf=as_rpf, precision="f64")
                for k in spread:
                    spread[k] = np.maximum(spread[k], np.abs(r[k] - ref[k]))
    return spread


@pytest.mark.parametrize("model", ALL_MODELS)
@pytest.mark.parametrize("planes", ["all", "four", "latitude"])
@pytest.mark.parametrize("path", ["float4", "scalar", "row_pairs"])
def test_system_at_seeded_states(dev, oracle, model, planes, path):
    """gclm_system against oracle.system(..., precision="f64") at seeded states far from convergence, with the per-entry
    gate of test_gpu_parity.py::test_hip_single_sweep_system and its simple_divisional k rule, in both parametrisations and
    both focal forms.  The float4, scalar (an unaligned view of the same fields) and row-pair paths see the same states.
    At these states (vfov to 140 deg, distortion at its clamps, principal point off centre) some entries are ill-conditioned
    in the state itself: every entry adds twice its 1-ulp input spread (_ulp_spread), which is a property of the state,
    not of any implementation.  (Measured: simple_divisional, four planes, rpf H[0,1] of one image moves by 5.8e-4 of its
    natural scale under a 1-ulp change of the state; the float4 and scalar sweeps agree on it to 1e-7 and sit 4.5e-4 off.)"""
    from geocalib_amd import Gravity, LMOptimizer, camera_models
    if path == "row_pairs" and (model not in ("radial", "simple_divisional") or planes != "all"):
        pytest.skip("the row-pair walk exists for radial / simple_divisional on five planes")
    H, W, B = 96, 128, 8
    data = _fields(model, B, H, W, seed=33, planes=planes)
    cam, grav = _random_states(model, B, H, W, seed=zlib.crc32(f"{model}/{planes}".encode()))
    data_dev = _to_dev(data, dev, unaligned=path == "scalar")
    for log_focal in (True, False):
        for as_rpf in (False, True):
            conf = {"camera_model": model, "use_log_focal": log_focal}
            opt = LMOptimizer(conf).eval()
            opt.row_pairs = path == "row_pairs"
            out = to_np(opt.system(data_dev, camera_models[model](torch.from_numpy(cam).to(dev)),
                                   Gravity(torch.from_numpy(grav).to(dev)), as_rpf=as_rpf))
            ref = oracle.system(data, cam, grav, conf, as_rpf=as_rpf, precision="f64")
            r32 = oracle.system(data, cam, grav, conf, as_rpf=as_rpf, precision="f32")
            ulp = _ulp_spread(oracle, data, cam, grav, conf, as_rpf, ref)
            P = ref["G"].shape[1]
            Hr, Gr = ref["H"], ref["G"]
            d = np.sqrt(np.abs(np.einsum("bii->bi", Hr))) + 1e-30
            cost = (ref["cost_up"] + ref["cost_lat"]) * H * W
            tol = np.full(P, 5e-5)
            if model == "simple_divisional":
                tol[3] = 1e-3            # test_gpu_parity.py: TOL_SYSTEM_DIV_K (camera.py:913)
            nh, ng = d[:, :, None] * d[:, None, :], d * np.sqrt(cost)[:, None]
            ah, ag = 2 * ulp["H"], 2 * ulp["G"]
            if model == "simple_divisional":       # the k rule: the k row / column adds 10x the float32 oracle's spread
                ah[:, 3, :] += 10 * np.abs(r32["H"] - Hr)[:, 3, :]
                ah[:, :, 3] += 10 * np.abs(r32["H"] - Hr)[:, :, 3]
                ag[:, 3] += 10 * np.abs(r32["G"] - Gr)[:, 3]
            eh = ((np.abs(out["H"][:, :P, :P] - Hr) - ah) / nh).max(0)
            eg = ((np.abs(out["G"][:, :P] - Gr) - ag) / ng).max(0)
            tag = f"system_states/{model}/{planes}/{path}/{'rpf' if as_rpf else 'loop'}/{'log' if log_focal else 'lin'}"
            MEASURED[tag] = {"H_rows": eh.max(1).tolist(), "G": eg.tolist()}
            assert (eh < np.maximum(tol[:, None], tol[None, :])).all(), (tag, eh)
            assert (eg < tol).all(), (tag, eg)
            assert np.allclose(out["cost_lat"], ref["cost_lat"], rtol=2e-5), tag
            if "up_field" in data:
                assert np.allclose(out["cost_up"], ref["cost_up"], rtol=2e-5), tag
