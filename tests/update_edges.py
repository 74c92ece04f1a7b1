"""The edge table of the per-image LM update (lambda rule, damped solve, manifold / focal / distortion update, tangent basis
of the new gravity: geocalib_amd/csrc/gclm_device.h), shared by the CPU self-check (test_update_edge_oracle.py), the GPU
test (test_update_edges.py) and the golden generator (golden/make_golden_update_edges.py).  A plain helper module.

Every solve of the rest of the suite starts from gravity (0, -1, 0), f = 0.7 max(h, w), k = 0 and ends within roll, pitch
+-45 deg, vfov 20..90 deg, k1 in [-0.3, 0.1]: the second branch of grav_roll (g.y >= 0), the sigma floor of the Householder
vector, the fov clamps of update_focal, the clamps of update_dist as the result of an UPDATE and the x10 / upper clamp of
the lambda rule are never executed there.  The states below start one LM step in each of those branches: a start
(camera, gravity), a ground truth a few degrees further (the fields are rendered at it, with the noise and confidences of
oracle/synth.py), and the branch the state is there for.  test_update_edge_oracle.py holds every state to its branch in
the float64 oracle, with a margin, so a state cannot quietly turn into a mid-domain case.

`apply_update` / `lambda_rule` restate the update in float64 numpy, with one plausible kernel bug per `mutant`, for the
gate-power test."""
import functools

import numpy as np

H, W = 48, 64                # float4 rows; the update does not depend on the shape
SEED = 47
LAMBDA = 0.1
MODELS = ("pinhole", "simple_radial", "radial", "simple_divisional")
NDIST = {"pinhole": 0, "simple_radial": 1, "radial": 2, "simple_divisional": 1}
FORMS = {"sph_log": {"use_spherical_manifold": True, "use_log_focal": True},
         "rp_lin": {"use_spherical_manifold": False, "use_log_focal": False}}
K_BOUND = {"pinhole": 0.0, "simple_radial": 0.7, "radial": 0.7, "simple_divisional": 3.0}
BOUND_MARGIN = 100           # the float64 unclamped step crosses its bound by this many step gates


def f32_focal_bounds(h):
    """(min, max) focal as the reference computes them in float32 (camera.py:141-142): fov2focal(ones * deg2rad(150), h) and
    fov2focal(ones * deg2rad(5), h) -- deg2rad of a Python number is a double, rounded to float32 by the product with the
    float32 ones; halved, torch.tan, h / 2 / tan in float32.  tests/golden/golden_update_edges.npz holds what the reference's
    own update_focal clamps to in float32, and test_update_edge_oracle.py holds this function to it.
    (Not the same as tan of the float32-arithmetic 5 / 180 * pi: that argument is one ulp larger, its tangent 0.043660946
    instead of 0.043660942, and the bound one ulp smaller at most heights -- 549.69031 instead of 549.69037 at h = 48.)"""
    import torch
    from geocalib_amd.utils import deg2rad, fov2focal
    hh = torch.tensor([float(h)], dtype=torch.float32)
    lo, hi = fov2focal(torch.ones(1) * deg2rad(150), hh), fov2focal(torch.ones(1) * deg2rad(5), hh)
    assert lo.dtype == torch.float32
    return np.float32(lo.item()), np.float32(hi.item())


def f64_focal_bounds(h):
    return h / 2 / np.tan(np.deg2rad(150.0) / 2), h / 2 / np.tan(np.deg2rad(5.0) / 2)


def rp_gravity(roll_deg, pitch_deg):
    r, p = np.deg2rad(roll_deg), np.deg2rad(pitch_deg)
    return np.array([-np.sin(r) * np.cos(p), -np.cos(r) * np.cos(p), np.sin(p)])


def _gravity(spec):
    g = rp_gravity(*spec[1:]) if spec[0] == "rp" else np.array(spec[1:], np.float64)
    return g / np.linalg.norm(g)


def camera_row(model, vfov, k1=0.0, k2=0.0, ratio=1.0, c_off=(0.0, 0.0)):
    fy = H / 2 / np.tan(np.deg2rad(vfov) / 2)
    nd = NDIST[model]
    return np.array([W, H, ratio * fy, fy, W / 2 + c_off[0], H / 2 + c_off[1], k1 if nd else 0.0, k2 if nd == 2 else 0.0])


# ------------------------------------------------------------------ the table

MID = {"vfov": 60.0, "k1": 0.0, "k2": 0.0, "ratio": 1.0}          # the intrinsics of a state that is about gravity: start ...
MID_GT = {"vfov": 55.0, "k1": -0.08, "k2": 0.01, "ratio": 1.0}    # ... and ground truth
RP0, RP0_GT = ("rp", 10.0, -5.0), ("rp", 14.0, -9.0)              # the gravity of a state that is about intrinsics

# The seven gravities: name -> (branch, start, ground truth).  near_pole starts at pitch 89 deg, not 89.9 deg: at 89.9 deg the
# reference's own (roll, pitch) formula, asin(-g.x / (sqrt(1 - g.z^2) + 1e-4)) with sqrt(1 - g.z^2) = 1.7e-3, is
# ill-conditioned in float32 -- the float32 ORACLE's (roll, pitch) step misses the float64 one by 1.3x the gate there (0.06x at
# 89 deg), and its covariance, which is in (roll, pitch) for both forms, by 2.9x the COV_EPS x kappa criterion.  Not a kernel
# matter, so the state was moved rather than a gate widened.  (The spherical update has nothing special at 89.9 deg.)
GRAVITIES = {
    "upside_a": ("gy_pos", ("rp", 140.0, 5.0), ("rp", 135.0, 10.0)),
    "upside_b": ("gy_pos", ("rp", -110.0, 0.0), ("rp", -120.0, 0.0)),
    "up_exact": ("sgn0", ("vec", 0.0, 1.0, 0.0), ("rp", 175.0, 0.0)),
    "cross": ("gy_cross", ("rp", 85.0, 0.0), ("rp", 95.0, 0.0)),
    "pole_pos": ("sigma_floor", ("vec", 0.0, 0.0, 1.0), ("rp", 0.0, 80.0)),
    "pole_neg": ("sigma_floor", ("vec", 0.0, 0.0, -1.0), ("rp", 0.0, -80.0)),
    "near_pole": ("near_pole", ("rp", 0.0, 89.0), ("rp", 0.0, 85.0)),
}
# Where gravity is exactly on the optical axis, the up vector at the principal point is 0 / 0.  With the principal point
# ON a pixel (cx = W / 2, cy = H / 2 here) that one pixel decides the reference's step: its J_vecnorm takes |q| = 1e-6 there
# (misc.py:263-281) and hands the gravity block 1e12 w -- H[0, 0] = 7.5e8 against 3e3 from all other pixels -- so gravity
# "does not move" (|delta| ~ 1e-6).  The sweep's rank-one form of that Jacobian, n n^T / |q| with n = (-u_y, u_x), gives the
# pixel ZERO instead (gclm_pass.hip: norm2_eps and what follows), so HIP does move: measured on the MI355X, pinhole,
# spherical form, two-launch path, HIP's step from g = (0, 0, +-1) misses the float64 oracle's by 61571x / 64750x the gate.
# That is a property of the sweep at one degenerate pixel, not of the update this table is about, and a state whose
# reference step hangs on a 0 / 0 guard cannot gate anything; the pole states therefore keep g = (0, 0, +-1) exactly (the
# sigma floor) with the principal point a fraction of a pixel off the grid, where no pixel has q = 0.  The update at the
# pole is exercised better for it: the step is no longer ~0.
# The pole states are in the spherical form only.  The sigma floor belongs to that form's Householder vector; in the
# (roll, pitch) form gravity on the optical axis is ill-conditioned in float32 by the reference's own formulas (d g / d roll
# = cos(pitch) (...) = 0 up to the rounding of pi / 2: 6e-17 in float64, -4e-8 in float32) -- without the degenerate pixel's
# damping the float32 ORACLE's (roll, pitch) step from the exact pole misses the float64 one by 340x .. 1040x the gate per
# image and by up to 9466x in a shared group.  Not a kernel matter; near_pole (89 deg) is that form's state next to the pole.
POLE_C_OFF = (0.37, -0.21)
POLE_FORMS = ("sph_log",)
EXACT_POLES = ("pole_pos", "pole_neg")       # the covariance is degenerate there (roll sigma ~ 2e4): not compared
UPSIDE = ("upside_a", "upside_b", "up_exact", "cross")


def _intrinsic_states(model):
    """name -> (branch, start intrinsics, ground-truth intrinsics).  The starts sit where the float64 oracle's unclamped
    step crosses the bound by BOUND_MARGIN gates in BOTH forms (test_update_edge_oracle.py checks exactly that); where a
    model does not reach a bound from the common start, its start was moved (FOCAL_STARTS / K_STARTS).  simple_divisional:
      - vfov 149 deg ends at fy = 6.57, short of 6.4308: started at 149.8 deg (149.95 deg in the shared group);
      - at the 5 deg bound it answers a narrower truth with k1 alone (focal step +0.05 px at most), and from k1 = -1, where
        the focal does move, its float32 step is ill-conditioned (float32 oracle at 0.6x the gate per image, 2.1x in the
        shared group): started just outside the bound, at vfov 4.99 deg (4.95 deg in the shared group, whose step moves the
        focal by -1.3 px), which the update has to bring back to the bound;
      - at k1 = +2.99 and vfov 60 deg the k step is 1e-7: started at vfov 8 deg, where it is +0.3.
    radial's shared group reaches k1 = -0.7 from -0.699 (from -0.69 the group's step ends at -0.6966)."""
    lo, hi = FOCAL_STARTS[model]
    lo_gt, hi_gt = FOCAL_TRUTHS[model]
    k0 = khi = {"k1": 0.0, "k2": 0.0}
    out = {}
    for ratio, tag in ((1.0, ""), (1.25, "_ratio")):
        out["fmin" + tag] = ("focal_min", {"vfov": lo, **k0, "ratio": ratio}, {"vfov": lo_gt, **k0, "ratio": ratio})
        out["fmax" + tag] = ("focal_max", {"vfov": hi, **khi, "ratio": ratio}, {"vfov": hi_gt, **khi, "ratio": ratio})
    if model != "pinhole":
        for name, (branch, k_start, k_gt) in K_STARTS[model].items():
            out[name] = (branch, {**MID, **k_start}, {**MID_GT, "k2": 0.0, **k_gt})
    return out


# start vfov at the (150 deg, 5 deg) bounds and the ground truth behind them
FOCAL_STARTS = {"pinhole": (149.0, 5.1), "simple_radial": (149.0, 5.1), "radial": (149.0, 5.1),
                "simple_divisional": (149.8, 4.99)}
FOCAL_TRUTHS = {"pinhole": (165.0, 3.0), "simple_radial": (165.0, 3.0), "radial": (165.0, 3.0),
                "simple_divisional": (165.0, 3.0)}
K_STARTS = {
    "simple_radial": {"kmax": ("k_hi", {"k1": 0.69}, {"k1": 0.9}), "kmin": ("k_lo", {"k1": -0.69}, {"k1": -0.9})},
    "radial": {"kmax": ("k_hi", {"k1": 0.69}, {"k1": 0.9}), "kmin": ("k_lo", {"k1": -0.69}, {"k1": -0.9}),
               "k2max": ("k2_hi", {"k2": 0.69}, {"k2": 0.9})},
    "simple_divisional": {"kmax": ("k_hi", {"k1": 2.99, "vfov": 8.0}, {"k1": 3.5, "vfov": 7.2}), "kmin": ("k_lo", {"k1": -2.99}, {"k1": -3.5})},
}


def states(model, form):
    """The named states of one configuration: dicts with name, branch, cam0 / grav0 (start) and cam_gt / grav_gt."""
    out = []
    for name, (branch, start, gt) in GRAVITIES.items():
        if name in EXACT_POLES and form not in POLE_FORMS:
            continue
        off = POLE_C_OFF if name in EXACT_POLES else (0.0, 0.0)
        out.append({"name": name, "branch": branch, "cam0": camera_row(model, **MID, c_off=off), "grav0": _gravity(start),
                    "cam_gt": camera_row(model, **MID_GT, c_off=off), "grav_gt": _gravity(gt)})
    for name, (branch, start, gt) in _intrinsic_states(model).items():
        out.append({"name": name, "branch": branch, "cam0": camera_row(model, **start), "grav0": _gravity(RP0),
                    "cam_gt": camera_row(model, **gt), "grav_gt": _gravity(RP0_GT)})
    return out


def _noisy_fields(model, cams, gravs, seed, noise=0.02, indices=None):
    """Fields of the given ground truths with the noise, clamps and confidences of oracle/synth.py:make_fields (image i is a
    function of (seed, i))."""
    from oracle import lm_oracle
    up, lat = lm_oracle.render(model, H, W, cams, gravs, precision="f64")
    B = len(cams)
    upc, latc = np.empty((B, H, W), np.float32), np.empty((B, H, W), np.float32)
    for i in range(B):
        rng = np.random.default_rng([seed, i if indices is None else int(indices[i]), 1])
        up[i] += rng.normal(0, noise, up[i].shape).astype(np.float32)
        lat[i] += rng.normal(0, noise, lat[i].shape).astype(np.float32)
        upc[i] = rng.uniform(0, 1, (H, W)).astype(np.float32)
        latc[i] = rng.uniform(0, 1, (H, W)).astype(np.float32)
    up /= np.sqrt((up.astype(np.float64) ** 2).sum(1, keepdims=True)).astype(np.float32)
    lim = np.float32(np.pi / 2 - 1e-3)
    return {"up_field": up, "latitude_field": np.clip(lat, -lim, lim), "up_confidence": upc, "latitude_confidence": latc}


def _pack(model, rows, seed):
    cam_gt = np.stack([s["cam_gt"] for s in rows])
    grav_gt = np.stack([s["grav_gt"] for s in rows])
    return {"names": [s["name"] for s in rows], "branches": [s["branch"] for s in rows],
            "data": _noisy_fields(model, cam_gt, grav_gt, seed),
            "cam0": np.stack([s["cam0"] for s in rows]).astype(np.float32),
            "grav0": np.stack([s["grav0"] for s in rows]).astype(np.float32),
            "lam": np.full(len(rows), LAMBDA, np.float32)}


@functools.lru_cache(maxsize=None)
def batch(model, form):
    """One batch holding every state of (model, form): names, branches, data (the fields), cam0 (B, 8), grav0 (B, 3), lam."""
    return _pack(model, states(model, form), SEED)


@functools.lru_cache(maxsize=None)
def pole_on_grid(model, form):
    """The exact-pole states with the principal point ON a pixel (cx = W / 2, cy = H / 2: what every default estimate
    uses), where HIP and the reference take different steps (POLE_C_OFF above, DESIGN.md "Known deviations").  Returns the
    batch and `masked`: the same fields with the up confidence of the principal-point pixel set to zero.  A float64 oracle
    step on `masked` is the reference's step without that pixel's up term, which is what the sweep computes: its rank-one
    Jacobian gives the pixel no gradient and no Hessian (its up cost stays, which no step depends on)."""
    rows = [{"name": name, "branch": "sigma_floor", "cam0": camera_row(model, **MID), "grav0": _gravity(GRAVITIES[name][1]),
             "cam_gt": camera_row(model, **MID_GT), "grav_gt": _gravity(GRAVITIES[name][2])} for name in EXACT_POLES]
    b = _pack(model, rows, SEED + 21)
    masked = {k: v.copy() for k, v in b["data"].items()}
    assert W % 2 == 0 and H % 2 == 0
    masked["up_confidence"][:, H // 2, W // 2] = 0
    return b, masked


def conf(model, form, **more):
    return {"camera_model": model, **FORMS[form], "lambda_": LAMBDA, "fix_lambda": True, **more}


# ------------------------------------------------------------------ shared-intrinsics groups

SHARED_FRAMES = ("upside_a", "up_exact", "cross", "pole_pos", "near_pole", "upside_b")


def shared_kinds(model):
    return ("mid", "fmin", "fmax") + (("k",) if model != "pinhole" else ())


SHARED_STARTS = {("radial", "k"): {"k1": -0.699}, ("simple_divisional", "fmin"): {"vfov": 149.95},
                 ("simple_divisional", "fmax"): {"vfov": 4.95}}


@functools.lru_cache(maxsize=None)
def shared_group(model, form, kind):
    """Six frames of one camera with the gravities of SHARED_FRAMES; the group's intrinsics start mid-domain, at either
    focal bound, or with k at its bound (simple_divisional: k1 = -2.99 towards -3)."""
    if kind == "mid":
        start, gt, branch = MID, {**MID_GT, "k2": 0.0}, "mid"
    elif kind == "k":
        branch, ks, kg = K_STARTS[model]["kmin"]
        start, gt = {**MID, **ks, **SHARED_STARTS.get((model, kind), {})}, {**MID_GT, "k2": 0.0, **kg}
    else:
        branch, start, gt = _intrinsic_states(model)[kind]
        start = {**start, **SHARED_STARTS.get((model, kind), {})}
    rows = []
    for name in SHARED_FRAMES:
        # the pole frame: spherical form only (POLE_FORMS), and not in the group at the k bound -- with k1 = -0.69 the pixels
        # next to the principal point carry H ~ 2e6 on the pole frame's gravity block and the float32 ORACLE's step of that
        # frame misses the float64 one by 7.7x the gate (simple_radial; radial 3.1x)
        if name in EXACT_POLES and (form not in POLE_FORMS or kind == "k"):
            continue
        _, g0, gg = GRAVITIES[name]
        # one camera per group: the whole group's principal point is off the grid, for its pole frame (POLE_C_OFF)
        rows.append({"name": name, "branch": branch, "cam0": camera_row(model, **start, c_off=POLE_C_OFF), "grav0": _gravity(g0),
                     "cam_gt": camera_row(model, **gt, c_off=POLE_C_OFF), "grav_gt": _gravity(gg)})
    return _pack(model, rows, SEED + 1 + shared_kinds(model).index(kind))


# ------------------------------------------------------------------ far states for the lambda rule

LAMBDA_STARTS = (0.1, 1e-6, 2e3)
LAMBDA_STEPS = (1, 2, 3, 4)
# simple_divisional is not here: from k1 != 0 its float32 step misses the float64 one (test_step_parity.DIV_STEPS), and on
# these states the float32 ORACLE itself takes another decision than the float64 one on a cost change of 3e-3 (one image,
# lambda0 = 1e-6, step 2).  The rule is the same code for every model (gclm_device.h: cost_rules).
LAMBDA_MODELS = ("pinhole", "simple_radial", "radial")
N_FAR = 12


FAR_POOL = 64


@functools.lru_cache(maxsize=None)
def far_states(model):
    """Twelve seeded states far from their ground truth: candidates 0, 1, ... drawn from default_rng(1), per candidate start
    and truth independently (roll +-180 deg, pitch +-80 deg, vfov 20..140 deg).  The first ten are taken as they come; the
    draw then goes on until two more are found on which the float64 ORACLE's cost rises within four adaptive steps from
    lambda0 = 0.1 or 1e-6 on a decision under test (decisions_under_test), so that the x10 branch of the rule is taken for
    every model -- pinhole's cost rises on 5 of the first 300 candidates only (23, 37, 64, 163, 188).  A candidate's fields
    are a function of its own index, so the choice does not change any image."""
    from oracle import lm_oracle
    rng = np.random.default_rng(1)
    a = np.array([[rng.uniform(-180, 180), rng.uniform(-80, 80), rng.uniform(20, 140),
                   rng.uniform(-180, 180), rng.uniform(-80, 80), rng.uniform(20, 140)] for _ in range(FAR_POOL)])
    k1 = np.random.default_rng([1, 7]).uniform(-0.3, 0.1, FAR_POOL)
    cam0 = np.stack([camera_row(model, v) for v in a[:, 2]]).astype(np.float32)
    cam_gt = np.stack([camera_row(model, v, k1=k) for v, k in zip(a[:, 5], k1)])
    grav0 = np.stack([rp_gravity(r, p) for r, p in a[:, 0:2]]).astype(np.float32)
    grav_gt = np.stack([rp_gravity(r, p) for r, p in a[:, 3:5]])
    pool = {"data": _noisy_fields(model, cam_gt, grav_gt, SEED + 11), "cam0": cam0, "grav0": grav0}
    rises = np.zeros(FAR_POOL, bool)
    for lam0 in (0.1, 1e-6):
        _, cost, _ = lambda_run(lm_oracle, model, lam0, "f64", start=pool)
        rises |= ((cost[1:] > cost[:-1]) & decisions_under_test(lam0, cost)).any(0)
    late = [i for i in np.flatnonzero(rises) if i >= N_FAR - 2][:2]
    assert len(late) == 2, (model, np.flatnonzero(rises))
    pick = np.array(list(range(N_FAR - 2)) + late)
    return {"data": {k: v[pick] for k, v in pool["data"].items()}, "cam0": cam0[pick], "grav0": grav0[pick],
            "candidates": pick}


def lambda_run(oracle, model, lam0, precision, steps=max(LAMBDA_STEPS), start=None):
    """Adaptive-lambda oracle steps from the far states, or from `start` = {data, cam0, grav0}: (result, cost (steps + 1, N)
    at the states 0 .. steps, lambda (steps + 1, N) after 0 .. steps steps)."""
    far = far_states(model) if start is None else start
    c = {"camera_model": model, "num_steps": steps, "early_stop": False, "fix_lambda": False}
    out = oracle.solve(far["data"], c, precision=precision, training=True, trace=True,
                       init=(far["cam0"], far["grav0"], np.full(len(far["cam0"]), lam0, np.float32)))
    cost = np.concatenate([out["trace"]["cost_up"] + out["trace"]["cost_lat"], out["final_cost"][None].astype(np.float64)])
    lam = np.concatenate([out["trace"]["lambda"], out["lambda"][None].astype(np.float64)])
    return out, cost, lam


def decisions_under_test(lam0, cost):
    """(steps, N) bool: decision k of an image (the rule after step k + 1) is under test while it and every earlier decision
    of that image rests on a relative cost change >= 1e-3 in the float64 oracle -- no float32 rounding of a cost flips
    such a decision, and after one that it could flip the trajectories need not agree.  From lambda0 = 2e3 only the first
    decision is under test, and unconditionally: 200 and 2e4 both clamp to 1e2, and the steps are tiny afterwards."""
    if lam0 == 2e3:
        m = np.zeros((len(cost) - 1, cost.shape[1]), bool)
        m[0] = True
        return m
    rel = np.abs(cost[1:] - cost[:-1]) / cost[:-1]
    return np.logical_and.accumulate(rel >= 1e-3, axis=0)


# ------------------------------------------------------------------ float64 restatement of the update, with mutants

UPDATE_MUTANTS = {
    # mutant -> (form it shows in or None for both, models or None for all, the states named for it)
    "roll_branch_dropped": ("rp_lin", None, ("upside_a", "upside_b")),
    "sgn_dropped": ("rp_lin", None, ("up_exact",)),
    "focal_bounds_from_width": (None, None, ("fmin", "fmax", "fmin_ratio", "fmax_ratio")),
    "fov_bounds_10_140": (None, None, ("fmin", "fmax", "fmin_ratio", "fmax_ratio")),
    "ratio_lost": (None, None, ("fmin_ratio", "fmax_ratio")),
    "divisional_clamped_at_0.7": (None, ("simple_divisional",), ("kmax", "kmin")),
    "k2_not_clamped": (None, ("radial",), ("k2max",)),
    "sigma_floor_dropped": ("sph_log", None, ("pole_pos",)),
}
LAMBDA_MUTANTS = ("lambda_clamp_1e3", "lambda_x10_on_fall")


def grav_roll(g, mutant=None):
    """Gravity.roll (gravity.py:63-81) in float64."""
    front = np.arcsin(-g[:, 0] / (np.sqrt(1 - g[:, 2] ** 2) + 1e-4))
    sgn = np.ones_like(front) if mutant == "sgn_dropped" else np.sign(g[:, 0])
    back = -front - np.pi * sgn
    return front if mutant == "roll_branch_dropped" else np.where(g[:, 1] < 0, front, back)


def householder(g, mutant=None):
    """SphericalManifold.householder_vector (misc.py:182-209), pivot = last component: (v (B, 3), beta (B,), sigma)."""
    sigma = g[:, 0] ** 2 + g[:, 1] ** 2
    norm = np.sqrt(sigma + g[:, 2] ** 2)
    if mutant != "sigma_floor_dropped":
        sigma = np.where(sigma < 1e-7, sigma + 1e-7, sigma)
    with np.errstate(all="ignore"):
        vpiv = np.where(g[:, 2] < 0, g[:, 2] - norm, -sigma / (g[:, 2] + norm))
        beta = 2 * vpiv ** 2 / (sigma + vpiv ** 2)
        v = np.stack([g[:, 0] / vpiv, g[:, 1] / vpiv, np.ones_like(vpiv)], 1)
    return v, beta, sigma


def apply_update(model, form, cam, grav, delta, mutant=None):
    """update_estimate (lm_optimizer.py:518-549) of float64 (cam (B, 8), grav (B, 3)) by delta (B, 5) = [d0, d1, df, dk1,
    dk2]: Gravity.update, BaseCamera.update_focal, update_dist."""
    cam, grav, delta = np.array(cam, np.float64), np.array(grav, np.float64), np.asarray(delta, np.float64)
    d0, d1 = delta[:, 0], delta[:, 1]
    if FORMS[form]["use_spherical_manifold"]:
        nx = np.linalg.norm(grav, axis=1)
        v, beta, _ = householder(grav, mutant)
        nd = np.sqrt(d0 ** 2 + d1 ** 2)
        nd_ = np.where(nd < 1e-7, nd + 1e-7, nd)
        sinc = np.where(nd < 1e-7, 1.0, np.sin(nd_) / nd_)
        e = np.stack([sinc * d0, sinc * d1, np.cos(nd)], 1)
        with np.errstate(all="ignore"):
            out = nx[:, None] * (e - v * (beta * (v * e).sum(1))[:, None])
    else:
        roll, pitch = grav_roll(grav, mutant) + d0, np.arcsin(grav[:, 2]) + d1
        out = np.stack([-np.sin(roll) * np.cos(pitch), -np.cos(roll) * np.cos(pitch), np.sin(pitch)], 1)
    with np.errstate(all="ignore"):
        grav = out / np.maximum(np.linalg.norm(out, axis=1), 1e-12)[:, None]
    fx, fy = cam[:, 2].copy(), cam[:, 3].copy()
    nfy = np.exp(np.log(fy) + delta[:, 2]) if FORMS[form]["use_log_focal"] else fy + delta[:, 2]
    side = cam[:, 0] if mutant == "focal_bounds_from_width" else cam[:, 1]
    fov_hi, fov_lo = (140.0, 10.0) if mutant == "fov_bounds_10_140" else (150.0, 5.0)
    lo, hi = side / 2 / np.tan(np.deg2rad(fov_hi) / 2), side / 2 / np.tan(np.deg2rad(fov_lo) / 2)
    fyc = np.minimum(np.maximum(nfy, lo), hi)
    cam[:, 2] = fyc if mutant == "ratio_lost" else fyc * fx / fy
    cam[:, 3] = fyc
    if model != "pinhole":
        b = 0.7 if mutant == "divisional_clamped_at_0.7" else K_BOUND[model]
        cam[:, 6] = np.clip(cam[:, 6] + delta[:, 3], -b, b)
        k2 = cam[:, 7] + (delta[:, 4] if model == "radial" else delta[:, 3])
        cam[:, 7] = k2 if mutant == "k2_not_clamped" else np.clip(k2, -b, b)
    return cam, grav


def unclamped(model, form, cam, delta):
    """What the update would give without its clamps: (fy, k1, k2), float64."""
    cam, delta = np.asarray(cam, np.float64), np.asarray(delta, np.float64)
    fy = np.exp(np.log(cam[:, 3]) + delta[:, 2]) if FORMS[form]["use_log_focal"] else cam[:, 3] + delta[:, 2]
    return fy, cam[:, 6] + delta[:, 3], cam[:, 7] + (delta[:, 4] if model == "radial" else delta[:, 3])


def fx_error(cam0, cam1):
    """|fx - fy (fx0 / fy0)| / fx of a step cam0 -> cam1, the product in float64.  The step gate compares fy only
    (test_step_oracle.step_params: "fx keeps its ratio"), so the ratio rebuild of update_focal is held to this instead, at
    FX_TOL = 2^-23: one float32 ulp at its coarsest, the bound for the two roundings of fy * fx0 / fy0."""
    c0, c1 = np.asarray(cam0, np.float64), np.asarray(cam1, np.float64)
    return np.abs(c1[:, 2] - c1[:, 3] * (c0[:, 2] / c0[:, 3])) / c1[:, 2]


FX_TOL = 2.0 ** -23


def lambda_rule(lam, prev_cost, new_cost, mutant=None):
    """update_lambda (lm_optimizer.py:95-106): x10 where the cost rose, x0.1 elsewhere, clamped to [1e-6, 1e2]."""
    rose = new_cost > prev_cost
    if mutant == "lambda_x10_on_fall":
        rose = ~rose
    return np.clip(lam * np.where(rose, 10.0, 0.1), 1e-6, 1e3 if mutant == "lambda_clamp_1e3" else 1e2)


# ------------------------------------------------------------------ oracle steps and the classes' update, one definition

def oracle_step(oracle, model, form, b, precision="f64", shared=False, steps=1, training=True, **more):
    """`steps` oracle steps from the start of batch / group `b` at its lambda, with the trace."""
    c = conf(model, form, num_steps=steps, early_stop=False, shared_intrinsics=shared, **more)
    return oracle.solve(b["data"], c, precision=precision, training=training, trace=steps > 0,
                        init=(b["cam0"], b["grav0"], b["lam"]))


def class_outputs(model, gravity_cls, camera_cls, cam0, grav0, delta, as_given=False):
    """Gravity.roll / pitch / J_rp / update and BaseCamera.update_focal / update_dist of `gravity_cls`, `camera_cls` (the
    package's or the reference's) in float64 at (cam0, grav0) with the steps `delta` (B, 5), as numpy.  as_given: the
    gravity is taken as it is, like the oracle's init, instead of re-normalised by the constructor."""
    import torch
    d = torch.from_numpy(np.asarray(delta, np.float64))
    g64 = torch.from_numpy(np.asarray(grav0, np.float64))
    if as_given:
        g = gravity_cls.__new__(gravity_cls)
        g._data = g64
    else:
        g = gravity_cls(g64)
    c = camera_cls(torch.from_numpy(np.asarray(cam0, np.float64)))
    out = {"roll": g.roll, "pitch": g.pitch, "J_rp": g.J_rp(),
           "update_sph": g.update(d[:, :2], spherical=True).vec3d, "update_rp": g.update(d[:, :2], spherical=False).vec3d,
           "focal_log": c.update_focal(d[:, 2:3], as_log=True)._data, "focal_lin": c.update_focal(d[:, 2:3], as_log=False)._data}
    nd = NDIST[model]
    if nd:
        out["dist"] = c.update_dist(d[:, 3:3 + nd])._data
    return {k: v.detach().numpy().copy() for k, v in out.items()}
