"""-m gpu: the per-image LM update of the HIP solve at its branch edges (tests/update_edges.py) against the float64 oracle.

The update -- lambda rule, damped solve, manifold / focal / distortion update, tangent basis of the new gravity
(geocalib_amd/csrc/gclm_device.h) -- exists in four copies that must agree: the batch update_kernel, the one-launch-per-
step kernel that splits it over three waves (gclm_pass.hip), the shared-intrinsics apply (gclm_update.hip; in one call and
through gclm_shared_reduce / _apply) and the final uncertainty pass.  Every other test runs them in the middle of their
domain.  Here every copy starts at the edge table's states: gravity with g.y > 0, exactly up, across g.y = 0, at the pole
(spherical form, principal point off the pixel grid: update_edges.POLE_C_OFF / POLE_FORMS say why) and next to it; focal
at either fov bound, with fx != fy; distortion at its clamps.  Asserted per state:
  - the step gate of tests/test_step_oracle.py (TAU_REL / TAU_FLOOR unchanged; shared groups with the scale of
    tests/shared_gate.py; simple_divisional with div_k_allowance on k, and on its first step only: test_step_parity
    .DIV_STEPS) against one float64 oracle step from HIP's own state, and the same step_failures;
  - where the float64 unclamped step crosses a bound by update_edges.BOUND_MARGIN gates, the result EQUALS the float32
    bound, computed here as the reference computes it; fx keeps its ratio to fy (update_edges.fx_error);
  - the quirk at g = (0, 1, 0): the (roll, pitch) step ends at g.y < 0, the spherical one at g.y > 0;
  - two steps, so that a state at a bound / with g.y > 0 is also the INPUT of an update and of a parameter block;
  - the one-launch-per-step path equals the two-launch path bit for bit (camera, gravity, costs, covariance, lambda);
  - num_steps = 0 in eval mode: covariance (the COV_EPS x condition number criterion of test_step_parity.check_steps)
    and the five sigmas at 1e-3 -- the first time tangent_rp runs with g.y > 0;
  - the lambda rule over k = 1..4 adaptive steps from seeded far states.
Every measured ratio goes to MEASURED under update_edges/<model>/<form>/<path>/<state>."""
import numpy as np
import pytest
import torch

from conftest import MEASURED
import shared_gate as sg
import update_edges as ue
from test_step_oracle import TAU_FLOOR, TAU_REL, div_k_allowance, step_gate
from test_step_parity import COST_RTOL, COV_EPS, DIV_STEPS, _expect_fused, _expect_slat, _oracle_step, _to_dev, hip_run

pytestmark = pytest.mark.gpu

CONFIGS = [(m, f) for m in ue.MODELS for f in ue.FORMS]
TWO_LAUNCH = {"fused": 0, "slat": 1, "row_pairs": False}
ONE_LAUNCH = {"fused": 1, "slat": 1, "row_pairs": False}
BOUND_BRANCHES = ("focal_min", "focal_max", "k_hi", "k_lo", "k2_hi")
SIGMA_COLS = {"roll_uncertainty": 7, "pitch_uncertainty": 8, "gravity_uncertainty": 9, "focal_uncertainty": 10,
              "vfov_uncertainty": 11}
SIGMA_RTOL = 1e-3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from geocalib_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _runs(dev, conf, data_dev, init, knobs, steps, expect):
    out = {}
    for s in steps:
        out[s] = hip_run(dev, conf, data_dev, s, knobs, init)
        expect(out[s], s)
    return out


def _gate_step(oracle, tag, conf, b, r0, r1, names, gated, scale=1.0, notes=None):
    """One HIP step r0 -> r1 against the float64 oracle step from r0's state; returns the oracle's step."""
    model = conf["camera_model"]
    start, lam = (r0["cam"], r0["grav"]), b["lam"]
    ref64 = _oracle_step(oracle, conf, b["data"], start, lam, "f64")
    extra = None
    if model == "simple_divisional":
        extra = div_k_allowance(model, _oracle_step(oracle, conf, b["data"], start, lam, "f32"), ref64)
    scale = np.asarray(scale, np.float64).reshape(-1, 1) if np.ndim(scale) else scale
    ratio = step_gate(model, start, (r1["cam"], r1["grav"]), (ref64["camera"], ref64["gravity"]), TAU_REL * scale,
                      TAU_FLOOR * scale, extra)
    for i, n in enumerate(names):
        MEASURED[f"{tag}/{n}"] = {"ratio": ratio[i].tolist(), "gated": bool(gated[i]), **(notes or {})}
    print(tag, {n: round(float(r.max()), 4) for n, r in zip(names, ratio)})
    assert np.isfinite(ratio[gated]).all() and (ratio[gated] <= 1).all(), (tag, dict(zip(names, ratio.max(1))))
    hip_failed = r1["info"][:, 14] > r0["info"][:, 14]
    assert np.array_equal(hip_failed, ref64["step_failures"] > 0), (tag, hip_failed, ref64["step_failures"])
    return ref64


def _check_bounds(tag, model, b, r0, r1):
    """Exact bounds after the first step, the float32 bound computed as the reference does; fx keeps its ratio."""
    lo, hi = ue.f32_focal_bounds(ue.H)
    kb = np.float32(ue.K_BOUND[model])
    cam0, cam1 = r0["cam"], r1["cam"]
    assert cam1.dtype == np.float32
    for i, (name, branch) in enumerate(zip(b["names"], b["branches"])):
        why = (tag, name, branch, cam1[i])
        if branch == "focal_min":
            assert cam1[i, 3] == lo, why
        elif branch == "focal_max":
            assert cam1[i, 3] == hi, why
        elif branch == "k_hi":
            assert cam1[i, 6] == kb, why
        elif branch == "k_lo":
            assert cam1[i, 6] == -kb, why
        elif branch == "k2_hi":
            assert cam1[i, 7] == kb, why
    err = ue.fx_error(cam0, cam1)
    assert (err <= ue.FX_TOL).all(), (tag, dict(zip(b["names"], err)))
    assert np.array_equal(cam1[:, [0, 1, 4, 5]], cam0[:, [0, 1, 4, 5]]), tag          # size and principal point untouched


def _check_quirk(tag, form, names, r1):
    if "up_exact" in names:
        gy = r1["grav"][names.index("up_exact"), 1]
        assert gy < -0.9 if form == "rp_lin" else gy > 0.9, (tag, gy)


def _same_bits(tag, a, b, first_col=0):
    """Camera, gravity and every written column of the info rows: stop_at, the costs, the sigmas, the parameter count,
    lambda, step_failures and the covariance."""
    P = int(a["info"][0, 12])
    cols = list(range(first_col, 15)) + list(range(16, 16 + P * P))
    for key, x, y in (("cam", a["cam"], b["cam"]), ("grav", a["grav"], b["grav"]), ("info", a["info"][:, cols], b["info"][:, cols])):
        assert np.array_equal(x, y, equal_nan=True), (tag, key, np.argwhere(x != y)[:8])


def _second_step_gated(model, b):
    """Step 2 is gated on the clamp and upside-down states (a state at a bound / with g.y > 0 as the input of an update);
    simple_divisional on its first step only (test_step_parity.DIV_STEPS)."""
    if 2 not in DIV_STEPS and model == "simple_divisional":
        return np.zeros(len(b["names"]), bool)
    return np.array([n in ue.UPSIDE or br in BOUND_BRANCHES for n, br in zip(b["names"], b["branches"])])


def _check_uncertainty(oracle, tag, conf, b, r0):
    """num_steps = 0, eval mode: the covariance and the sigmas of HIP at the start states against the float64 oracle at
    the same states.  The two exact-pole states are excluded from the comparison -- the covariance is degenerate there
    (d gravity / d roll = 0 at the pole: roll sigma ~ 2e4) -- and held to finiteness and step_failures only."""
    names = b["names"]
    at = _oracle_step(oracle, conf, b["data"], (r0["cam"], r0["grav"]), b["lam"], "f64", steps=0, training=False)
    keep = np.array([n not in ue.EXACT_POLES for n in names])
    e0 = np.abs(r0["info"][:, 6] / at["final_cost"] - 1)
    assert (e0 <= COST_RTOL).all(), (tag, e0.max())
    Cr = at["covariance"].astype(np.float64)
    P = int(r0["info"][0, 12])
    assert Cr.shape[1] == P
    Ch = r0["info"][:, 16:16 + P * P].reshape(-1, P, P).astype(np.float64)
    sig_h = np.stack([r0["info"][:, c] for c in SIGMA_COLS.values()], 1).astype(np.float64)
    sig_r = np.stack([at[k] for k in SIGMA_COLS], 1).astype(np.float64)
    assert np.array_equal(np.isfinite(Ch).all((1, 2)), np.isfinite(Cr).all((1, 2))), tag
    assert np.array_equal(np.isfinite(sig_h), np.isfinite(sig_r)), (tag, sig_h, sig_r)
    assert not r0["info"][:, 14].any() and not at["step_failures"].any(), tag
    Cr, Ch, sig_h, sig_r = Cr[keep], Ch[keep], sig_h[keep], sig_r[keep]
    Hr = np.linalg.inv(Cr)
    d = 1 / np.sqrt(np.abs(np.einsum("bii->bi", Hr)))
    kappa = np.linalg.cond(Hr * d[:, :, None] * d[:, None, :])
    sd = np.sqrt(np.abs(np.einsum("bii->bi", Cr)))
    ecov = (np.abs(Ch - Cr) / (sd[:, :, None] * sd[:, None, :])).max((1, 2)) / kappa
    esig = np.abs(sig_h / sig_r - 1).max(1)
    kept = [n for n in names if n not in ue.EXACT_POLES]
    for i, n in enumerate(kept):
        MEASURED[f"{tag}/{n}"] = {"cov_over_kappa": float(ecov[i]), "kappa": float(kappa[i]), "sigma_rel": float(esig[i])}
    print(tag, {n: (float(f"{a:.2g}"), float(f"{c:.2g}"), float(f"{k:.3g}")) for n, a, c, k in zip(kept, esig, ecov, kappa)})
    assert (ecov <= COV_EPS).all(), (tag, dict(zip(kept, ecov)))
    assert (esig <= SIGMA_RTOL).all(), (tag, dict(zip(kept, esig)))


# ------------------------------------------------------------------ independent images: batch and single

@pytest.mark.parametrize("model,form", CONFIGS)
def test_update_edges_batch(dev, oracle, model, form):
    """Every state of the table in one batch, on the two-launch path and on the one-launch-per-step path forced on it."""
    b = ue.batch(model, form)
    conf, init = ue.conf(model, form), (b["cam0"], b["grav0"])
    data_dev = _to_dev(b["data"], dev)
    two = _runs(dev, conf, data_dev, init, TWO_LAUNCH, (0, 1, 2), _expect_slat(True))
    one = _runs(dev, conf, data_dev, init, ONE_LAUNCH, (0, 1, 2), _expect_fused)
    everything = np.ones(len(b["names"]), bool)
    for path, runs in (("two_launch", two), ("one_launch", one)):
        tag = f"update_edges/{model}/{form}/{path}"
        _gate_step(oracle, tag + "/k1", conf, b, runs[0], runs[1], b["names"], everything)
        _check_quirk(tag, form, b["names"], runs[1])
        _gate_step(oracle, tag + "/k2", conf, b, runs[1], runs[2], b["names"], _second_step_gated(model, b))
        assert (ue.fx_error(runs[1]["cam"], runs[2]["cam"]) <= ue.FX_TOL).all(), tag
    # the states reached what they are there for, on the device too: g.y > 0 before and after, across g.y = 0
    at = {n: i for i, n in enumerate(b["names"])}
    g0, g1 = two[0]["grav"], two[1]["grav"]
    assert g0[at["upside_a"], 1] > 0.1 < g1[at["upside_a"], 1] and g0[at["upside_b"], 1] > 0.1 < g1[at["upside_b"], 1]
    assert g0[at["cross"], 1] < 0 < g1[at["cross"], 1]
    for s in (0, 1, 2):
        _same_bits(f"{model}/{form}/steps{s}", two[s], one[s])
    _check_uncertainty(oracle, f"update_edges/{model}/{form}/uncertainty", conf, b, two[0])
    for path, runs in (("two_launch", two), ("one_launch", one)):
        _check_bounds(f"update_edges/{model}/{form}/{path}", model, b, runs[0], runs[1])


def _single_states(model, form):
    pole = "pole_pos" if form in ue.POLE_FORMS else "near_pole"          # update_edges.POLE_FORMS: why
    return ("upside_a", pole, "fmin", "fmax") + (("kmin",) if model != "pinhole" else ())


@pytest.mark.parametrize("model,form", CONFIGS)
def test_update_edges_single_image(dev, oracle, model, form):
    """B = 1 (the interactive case, one launch per step by the library's own choice too): the upside-down, pole and clamp
    states one at a time, against the oracle and, bit for bit, against the two-launch path on the same single image."""
    full = ue.batch(model, form)
    conf = ue.conf(model, form)
    for name in _single_states(model, form):
        i = full["names"].index(name)
        b = {"names": [name], "branches": [full["branches"][i]], "lam": full["lam"][i:i + 1],
             "data": {k: v[i:i + 1] for k, v in full["data"].items()}}
        init = (full["cam0"][i:i + 1], full["grav0"][i:i + 1])
        data_dev = _to_dev(b["data"], dev)
        one = _runs(dev, conf, data_dev, init, ONE_LAUNCH, (0, 1, 2), _expect_fused)
        two = _runs(dev, conf, data_dev, init, TWO_LAUNCH, (0, 1, 2), _expect_slat(True))
        tag = f"update_edges/{model}/{form}/one_launch_B1"
        _gate_step(oracle, tag + "/k1", conf, b, one[0], one[1], b["names"], np.ones(1, bool))
        _gate_step(oracle, tag + "/k2", conf, b, one[1], one[2], b["names"], _second_step_gated(model, b))
        for s in (0, 1, 2):
            _same_bits(f"{model}/{form}/B1/{name}/steps{s}", two[s], one[s])
        _check_uncertainty(oracle, f"{tag}/uncertainty", conf, b, one[0])
        _check_bounds(tag, model, b, one[0], one[1])


# ------------------------------------------------------------------ shared intrinsics: one call and split

def _shared_scale(oracle, conf, b, start, lam):
    """tests/shared_gate.py: the gate scaled by the group's own conditioning, from the float64 per-frame systems in this
    configuration's parametrisation."""
    keep = ("camera_model", "use_log_focal", "use_spherical_manifold")
    H = oracle.system(b["data"], start[0], start[1], {k: conf[k] for k in keep}, precision="f64")["H"]
    scale, kappa = sg.group_scale(conf["camera_model"], H, lam[0], [np.arange(len(H))])
    return scale, {"kappa_g": float(kappa.max()), "scale": float(scale.max())}


def _split_run(dev, conf, data_dev, init, sels, steps):
    """The gclm_shared_begin / _reduce / _apply / _finish protocol on one device, one group, from the state `init`
    (test_gpu_parity.run_virtual_ranks): rank r holds the frames sels[r]; assembled over the ranks in frame order."""
    from test_gpu_parity import run_virtual_ranks
    H, W = data_dev["latitude_field"].shape[-2:]
    B = len(init[0])
    start = tuple(torch.from_numpy(a).to(dev) for a in init)
    gofs = [torch.zeros(sel.numel(), device=dev, dtype=torch.int32) for sel in sels]
    res = run_virtual_ranks(dev, {**conf, "num_steps": steps, "early_stop": False}, data_dev, sels, gofs, 1, H, W, init=start)
    cam, grav = np.zeros((B, 8), np.float32), np.zeros((B, 3), np.float32)
    info = np.zeros((B, res[0][2].shape[1]), np.float32)
    for (c, g, i, _), sel in zip(res, sels):
        sel = sel.cpu().numpy()
        if sel.size:
            cam[sel], grav[sel], info[sel] = c, g, i
    return {"cam": cam, "grav": grav, "info": info}


@pytest.mark.parametrize("model,form", CONFIGS)
def test_update_edges_shared_intrinsics(dev, oracle, model, form):
    """Six frames of one camera with the table's gravities (group_size = the batch), the group's focal mid-domain and at
    either bound, its k at the bound (simple_divisional: towards -3 from -2.99; its first shared run anywhere): in one
    call, and split over two virtual ranks of three frames each.  The halves sum the group's partials in another order
    than the one call, so they are held to the step gate; a session in which one rank holds every frame and the other
    none IS the one-call solve and must equal it bit for bit."""
    for kind in ue.shared_kinds(model):
        b = ue.shared_group(model, form, kind)
        n = len(b["names"])
        conf = ue.conf(model, form, shared_intrinsics=True, group_size=None)
        init = (b["cam0"], b["grav0"])
        data_dev = _to_dev(b["data"], dev)
        frames = torch.arange(n, device=dev)
        paths = {"shared_one_call": {s: hip_run(dev, conf, data_dev, s, {}, init) for s in (0, 1, 2)},
                 "shared_split": {s: _split_run(dev, conf, data_dev, init, [frames[:n // 2], frames[n // 2:]], s) for s in (0, 1, 2)}}
        whole = {s: _split_run(dev, conf, data_dev, init, [frames, frames[:0]], s) for s in (0, 1, 2)}
        for path, runs in paths.items():
            tag = f"update_edges/{model}/{form}/{path}_{kind}"
            for k in (1, 2):
                r0, r1 = runs[k - 1], runs[k]
                # step 2: the upside-down frames (their camera is the group's, at its bound), simple_divisional never
                gated = np.ones(n, bool) if k == 1 else _second_step_gated(model, {**b, "branches": ["mid"] * n})
                scale, notes = _shared_scale(oracle, conf, b, (r0["cam"], r0["grav"]), b["lam"])
                _gate_step(oracle, f"{tag}/k{k}", conf, b, r0, r1, b["names"], gated, scale, notes)
                assert (ue.fx_error(r0["cam"], r1["cam"]) <= ue.FX_TOL).all(), tag
            _check_quirk(tag, form, b["names"], runs[1])
            for s in (1, 2):                                           # one camera per group
                c = runs[s]["cam"]
                assert (c[:, 2:4] == c[:1, 2:4]).all() and (c[:, 6:] == c[:1, 6:]).all(), (tag, s)
        for s in (0, 1, 2):          # everything but stop_at, which a session without a solve loop does not decide
            _same_bits(f"{model}/{form}/{kind}/whole_session/steps{s}", whole[s], paths["shared_one_call"][s], first_col=1)
        for path, runs in paths.items():
            _check_uncertainty(oracle, f"update_edges/{model}/{form}/{path}_{kind}/uncertainty", conf, b, runs[0])
        for path, runs in paths.items():
            _check_bounds(f"update_edges/{model}/{form}/{path}_{kind}", model, b, runs[0], runs[1])


@pytest.mark.parametrize("h", [231, 480])
def test_focal_bounds_at_other_heights(dev, oracle, h):
    """The fov clamps at other image heights than the table's: two pinhole images that start just outside the 150 deg and
    the 5 deg bound with a ground truth further out, so the float64 unclamped step stays outside; HIP's focal must EQUAL
    what the reference's own float32 update_focal clamps to at this height (recorded in golden_update_edges.npz)."""
    import os
    from conftest import GOLDEN
    w, model, form = 64, "pinhole", "sph_log"
    bounds = np.load(os.path.join(GOLDEN, "golden_update_edges.npz"))[f"bounds_f32/{h}"]

    def cams(vfovs):
        f = h / 2 / np.tan(np.deg2rad(np.array(vfovs)) / 2)
        return np.stack([np.full(2, w), np.full(2, h), f, f, np.full(2, w / 2), np.full(2, h / 2), 0 * f, 0 * f], 1)
    grav0 = np.tile(ue._gravity(ue.RP0), (2, 1)).astype(np.float32)
    up, lat = oracle.render(model, h, w, cams([165.0, 3.0]), np.tile(ue._gravity(ue.RP0_GT), (2, 1)), precision="f64")
    data, cam0 = {"up_field": up, "latitude_field": lat}, cams([150.5, 4.9]).astype(np.float32)
    conf = ue.conf(model, form)
    runs = {s: hip_run(dev, conf, _to_dev(data, dev), s, {}, (cam0, grav0)) for s in (0, 1)}
    lam = np.full(2, ue.LAMBDA, np.float32)
    ref = oracle.solve(data, {**conf, "num_steps": 1, "early_stop": False}, precision="f64", training=True, trace=True,
                       init=(runs[0]["cam"], runs[0]["grav"], lam))
    fy_u, _, _ = ue.unclamped(model, form, runs[0]["cam"], ref["trace"]["delta"][0])
    lo, hi = ue.f64_focal_bounds(h)
    assert fy_u[0] < lo * (1 - 1e-3) and fy_u[1] > hi * (1 + 1e-3), (fy_u, lo, hi)
    got = runs[1]["cam"]
    MEASURED[f"update_edges/focal_bounds/h{h}"] = {"hip": got[:, 3].tolist(), "reference": bounds.tolist()}
    assert got[0, 3] == bounds[0] and got[1, 3] == bounds[1], (got[:, 3], bounds)
    assert np.array_equal(got[:, 2], got[:, 3])


# ------------------------------------------------------------------ the pole with the principal point on a pixel

@pytest.mark.parametrize("model,form", CONFIGS)
def test_pole_on_the_pixel_grid_pins_the_known_deviation(dev, oracle, model, form):
    """g = (0, 0, +-1) with cx = W / 2, cy = H / 2: the one input on which HIP and the reference take DIFFERENT steps, on
    purpose (update_edges.POLE_C_OFF).  At the principal-point pixel the up vector is 0 / 0; the
    reference's J_vecnorm guard (|q| = 1e-6) lets that pixel pin gravity (|delta| ~ 1e-6), the sweep's rank-one Jacobian
    gives it nothing.  This test pins what HIP does, so the divergence is visible and a change of either side shows:
      - spherical form: HIP's step meets the unchanged step gate against the float64 oracle on the same fields with that
        pixel's up confidence zeroed (the reference without the pixel's up term);
      - both forms: HIP's step misses the reference's own step by more than 1000 gates (64000 in float64), no step
        fails, everything is finite, and both launch paths agree bit for bit.
    In the (roll, pitch) form the step without the pixel is ill-conditioned in float32 by the reference's own formulas
    (float32 oracle 130x .. 950x the gate, update_edges.POLE_FORMS), so HIP is not held to a gate there."""
    b, masked = ue.pole_on_grid(model, form)
    conf, init = ue.conf(model, form), (b["cam0"], b["grav0"])
    data_dev = _to_dev(b["data"], dev)
    two = _runs(dev, conf, data_dev, init, TWO_LAUNCH, (0, 1), _expect_slat(True))
    one = _runs(dev, conf, data_dev, init, ONE_LAUNCH, (0, 1), _expect_fused)
    for s in (0, 1):
        _same_bits(f"{model}/{form}/pole_on_grid/steps{s}", two[s], one[s])
    r0, r1 = two[0], two[1]
    assert np.isfinite(r1["cam"]).all() and np.isfinite(r1["grav"]).all() and not r1["info"][:, 14].any()
    tag = f"update_edges/{model}/{form}/pole_on_grid"
    start = (r0["cam"], r0["grav"])
    ref = _oracle_step(oracle, conf, b["data"], start, b["lam"], "f64")
    away = step_gate(model, start, (r1["cam"], r1["grav"]), (ref["camera"], ref["gravity"])).max(1)
    MEASURED[tag + "/against_reference"] = dict(zip(b["names"], away.tolist()))
    assert (away > 1000).all(), (tag, away)
    gated = np.full(len(b["names"]), form in ue.POLE_FORMS)
    _gate_step(oracle, tag + "/without_the_pixel", conf, {**b, "data": masked}, r0, r1, b["names"], gated)


# ------------------------------------------------------------------ the lambda rule

@pytest.mark.parametrize("model", ue.LAMBDA_MODELS)
def test_lambda_rule(dev, oracle, model):
    """Adaptive lambda from the seeded far states: the lambda of HIP after k = 1..4 steps (info[:, 13]) equals the float64
    oracle's after k steps from the same start to 1e-6, on every decision under test (update_edges.decisions_under_test;
    tests/test_update_edge_oracle.py shows for these seeds that those rest on cost changes >= 1e-3, contain x10 steps, and
    that honest float32 takes them like float64).  lambda0 = 2e3 gives exactly 1e2 (the upper clamp), 1e-6 stays at 1e-6
    on a fall (the lower clamp).  Both launch paths, which must also agree bit for bit."""
    far = ue.far_states(model)
    data_dev = _to_dev(far["data"], dev)
    for lam0 in ue.LAMBDA_STARTS:
        conf = {"camera_model": model, "lambda_": lam0, "fix_lambda": False}
        steps = (0,) + ue.LAMBDA_STEPS
        two = _runs(dev, conf, data_dev, (far["cam0"], far["grav0"]), TWO_LAUNCH, steps, _expect_slat(True))
        one = _runs(dev, conf, data_dev, (far["cam0"], far["grav0"]), ONE_LAUNCH, steps, _expect_fused)
        start = {"data": far["data"], "cam0": two[0]["cam"], "grav0": two[0]["grav"]}
        _, cost, lam = ue.lambda_run(oracle, model, lam0, "f64", start=start)
        under = ue.decisions_under_test(lam0, cost)
        assert np.allclose(two[0]["info"][:, 13], lam0, rtol=1e-6)
        worst = 0.0
        for k in ue.LAMBDA_STEPS:
            _same_bits(f"lambda/{model}/{lam0:g}/steps{k}", two[k], one[k])
            got, ref, m = two[k]["info"][:, 13].astype(np.float64), lam[k], under[k - 1]
            bad = m & ~np.isclose(got, ref, rtol=1e-6, atol=0)
            for i in np.flatnonzero(bad):          # both costs at the step, before deciding that it is a bug
                print(f"lambda {model} lam0 {lam0:g} step {k} image {i}: HIP lambda {got[i]:g} cost {two[k]['info'][i, 6]:.9g} "
                      f"(before: {two[k - 1]['info'][i, 6]:.9g}); float64 lambda {ref[i]:g} cost {cost[k, i]:.9g} "
                      f"(before: {cost[k - 1, i]:.9g})")
            assert not bad.any(), (model, lam0, k, np.flatnonzero(bad))
            if m.any():
                worst = max(worst, float(np.abs(got[m] / ref[m] - 1).max()))
        if lam0 == 2e3:
            assert (two[1]["info"][:, 13] == np.float32(1e2)).all()
        MEASURED[f"update_edges/{model}/lambda/{lam0:g}"] = {"worst_rel": worst, "under_test": int(under.sum()),
                                                               "x10_under_test": int(((cost[1:] > cost[:-1]) & under).sum())}
