"""-m gpu: the stage kernels of the reference-compatible API against the float64 references and gates of
tests/test_stage_oracle.py, at the shapes and edges where per-pixel and per-system kernels go wrong: several workgroups
per image and ragged tails, B > 1 with a different camera per image, every P and R, branch thresholds, NULL outputs,
NaN inputs and the batch limits.  Python wrappers where they reach a case, the C ABI (ctypes) where only it does.

Semantics pinned here:
  - gclm_huber_costs floors the weight at FLT_EPSILON as the reference's huber_loss does, gives (inf, eps, -0) at
    y = +inf, and does not multiply the second derivative by the confidence (scaled_loss's d2 carries none).
  - gclm_optimizer_step reads the lower triangle of H only (as torch.linalg.cholesky); a NaN there fails the system
    (delta = 0, failed = 1).  A NaN in G with a positive definite H is not a failure: delta is NaN, failed = 0, as
    torch.cholesky_solve gives the reference.
Worst measured ratios to each gate go to MEASURED (1 = at the gate)."""
import numpy as np
import pytest
import torch

from conftest import MEASURED
from test_stage_oracle import (EPS32, FIELD_SHAPES, MODELS, U, contraction_bounds, contraction_gate, contraction_inputs,
                               contraction_ref, head_gate, head_inputs, head_ref, huber_gate, huber_inputs, jacobian_gate,
                               residual_gate, spd_systems, stage_cameras, stage_fields, step_families, step_gate, step_ref,
                               symmetric_prefill, x2_of)
from test_step_parity import _to_dev

pytestmark = pytest.mark.gpu

MODEL_ID = {"pinhole": 0, "simple_radial": 1, "radial": 2, "simple_divisional": 3}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from geocalib_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _lib():
    from geocalib_amd import _lib as lib
    return lib.load()


def _t(a, dev):
    """A device copy of a float32 / int32 array; never a zero-size allocation (an empty tensor's data_ptr is NULL)."""
    a = np.ascontiguousarray(a)
    t = torch.empty(max(a.size, 1), dtype=torch.from_numpy(a[:0]).dtype, device=dev)
    if a.size:
        t[:a.size].copy_(torch.from_numpy(a.reshape(-1)))
    return t[:a.size].view(a.shape) if a.size else t


def _p(t):
    return None if t is None else t.data_ptr()


def _s(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _np(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def record(key, r):
    v = float(np.max(r)) if np.size(r) else 0.0
    MEASURED[f"stage/{key}"] = max(MEASURED.get(f"stage/{key}", 0.0), v)
    return v


# ------------------------------------------------------------------ gclm_residual_fields / gclm_jacobian_fields

def _camera(model, cams, gravs, dev):
    from geocalib_amd.camera import camera_models
    from geocalib_amd.gravity import Gravity
    return camera_models[model](_t(cams, dev)), Gravity(_t(gravs, dev))


@pytest.mark.parametrize("shape", FIELD_SHAPES)
@pytest.mark.parametrize("model", MODELS)
def test_residual_fields_against_float64(dev, oracle, model, shape):
    """calculate_residuals (gclm_residual_fields) of 3 images with different cameras, latitudes beyond +-pi/2 included,
    per pixel against the float64 oracle; aligned and unaligned views; one field alone (the other output NULL) gives the
    same bits."""
    from geocalib_amd import LMOptimizer
    H, W = shape
    cams, gravs = stage_cameras(model, 3, H, W)
    data = stage_fields(oracle, model, cams, gravs, H, W)
    r64 = oracle.residual_fields(model, data, cams, gravs, precision="f64")
    r32 = oracle.residual_fields(model, data, cams, gravs, precision="f32")
    opt = LMOptimizer({"camera_model": model}).eval()
    cam, grav = _camera(model, cams, gravs, dev)
    first = None
    for unaligned in (False, True):
        dd = _to_dev(data, dev, unaligned=unaligned)
        res = {k: _np(v) for k, v in opt.calculate_residuals(cam, grav, dd).items()}
        for k in r64:
            assert res[k].shape == r64[k].shape
            r = record(f"residual/{model}/{k}", residual_gate(model, res[k], r64[k], r32[k], H, W))
            assert r <= 1, (k, unaligned, r)
        if first is None:
            first = res
        for k in r64:
            assert np.array_equal(res[k], first[k]), k
        for key, rk in (("latitude_field", "latitude_residual"), ("up_field", "up_residual")):
            alone = opt.calculate_residuals(cam, grav, {key: dd[key]})
            assert list(alone) == [rk] and np.array_equal(_np(alone[rk]), res[rk]), key


@pytest.mark.parametrize("form", ["loop", "rpf"])
@pytest.mark.parametrize("shape", FIELD_SHAPES)
@pytest.mark.parametrize("model", MODELS)
def test_jacobian_fields_against_float64(dev, oracle, model, shape, form):
    """J_perspective_field (gclm_jacobian_fields) of 3 different cameras, spherical / log-focal and rpf forms, every entry
    against the RMS of its column in float64."""
    from geocalib_amd import perspective_fields as pf
    H, W = shape
    sph = form == "loop"
    cams, gravs = stage_cameras(model, 3, H, W)
    J64 = oracle.jacobian_fields(model, H, W, cams, gravs, sph, sph, precision="f64")
    J32 = oracle.jacobian_fields(model, H, W, cams, gravs, sph, sph, precision="f32")
    cam, grav = _camera(model, cams, gravs, dev)
    got = pf.J_perspective_field(cam, grav, spherical=sph, log_focal=sph)
    for name, g, r64, r32 in zip(("J_up", "J_lat"), got, J64, J32):
        g = _np(g)
        assert g.shape == r64.shape
        r = record(f"jacobian/{model}/{form}/{name}", jacobian_gate(model, g, r64, r32))
        assert r <= 1, (name, r)


def test_field_kernels_take_65535_images_and_refuse_65536(dev, oracle):
    """B = 65535 (the grid.y limit): every image equals the same camera's result in a 3-image call bit for bit; 65536 is
    refused with -3 before any launch.  Both per-pixel kernels."""
    lib = _lib()
    model, H, W = "radial", 2, 3
    cams, gravs = stage_cameras(model, 3, H, W)
    data = stage_fields(oracle, model, cams, gravs, H, W)
    big = 65536
    rep = lambda a: np.ascontiguousarray(np.resize(a, (big,) + a.shape[1:]))  # noqa: E731  image b = image b % 3
    up, lat, cam, grav = (_t(rep(a), dev) for a in (data["up_field"], data["latitude_field"], cams, gravs))
    r_up = torch.full((big, H * W, 2), np.nan, device=dev)
    r_lat = torch.full((big, H * W, 1), np.nan, device=dev)
    J_up = torch.full((big, H, W, 2, 5), np.nan, device=dev)
    J_lat = torch.full((big, H, W, 1, 5), np.nan, device=dev)
    m = MODEL_ID[model]
    for B, want in ((3, 0), (65535, 0), (65536, -3)):
        if want:
            r_up.fill_(np.nan)
            J_up.fill_(np.nan)
        assert lib.gclm_residual_fields(m, _p(up), _p(lat), _p(cam), _p(grav), B, H, W, _p(r_up), _p(r_lat), _s(dev)) == want
        assert lib.gclm_jacobian_fields(m, _p(cam), _p(grav), B, H, W, 1, 1, _p(J_up), _p(J_lat), _s(dev)) == want
        if B == 3:
            small = [_np(t[:3]).copy() for t in (r_up, r_lat, J_up, J_lat)]
            r64 = oracle.residual_fields(model, data, cams, gravs, precision="f64")
            r32 = oracle.residual_fields(model, data, cams, gravs, precision="f32")
            assert residual_gate(model, small[0], r64["up_residual"], r32["up_residual"], H, W).max() <= 1
        elif want == 0:
            for t, s in zip((r_up, r_lat, J_up, J_lat), small):
                assert np.array_equal(_np(t[:B]), np.resize(s, (B,) + s.shape[1:]))
        else:
            assert torch.isnan(r_up).all() and torch.isnan(J_up).all()          # nothing was written


# ------------------------------------------------------------------ gclm_huber_costs

def _huber_dev(dev, rows, n, dim, a, conf, want=(True, True, True)):
    lib = _lib()
    r = _t(np.asarray(rows, np.float32), dev)
    c = None if conf is None else _t(np.asarray(conf, np.float32), dev)
    outs = [torch.full((max(n, 1),), np.nan, device=dev) for _ in range(3)]
    rc = lib.gclm_huber_costs(_p(r), n, dim, float(a), _p(c), *[_p(o) if w else None for o, w in zip(outs, want)], _s(dev))
    assert rc == 0
    return [_np(o)[:n] for o in outs]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 10 ** 6 + 3])
@pytest.mark.parametrize("dim", [0, 1, 2, 3, 4])
def test_huber_costs_against_float64(dev, dim, n):
    """gclm_huber_costs: cost, weight and second derivative against the reference's formulas in float64 (eps floor and
    +1e-8 included) at scales 1, 1e-2, 3, with and without a confidence, on inputs that start with the edges (0, a^2 and
    one ulp either side, 1e13, 1e14, 1e20, +inf)."""
    conf = np.random.default_rng([n, dim]).uniform(0.05, 1, n).astype(np.float32)
    for a in (1.0, 1e-2, 3.0):
        rows = huber_inputs(n, dim, a)
        x2 = x2_of(rows, dim)
        for c in (None, conf):
            got = _huber_dev(dev, rows, n, dim, a, c)
            for name, r in zip(("cost", "weight", "second"), huber_gate(got, x2, a, c)):
                v = record(f"huber/dim{dim}/{name}", r)
                assert v <= 1, (a, c is not None, name, v, x2[np.argmax(r)])


def test_huber_costs_write_only_what_is_asked(dev):
    """Every subset of the three outputs: the requested ones equal the all-outputs call bit for bit, the others keep
    their NaN canary; no output at all is refused (-3)."""
    n, dim, a = 257, 2, 1e-2
    rows = huber_inputs(n, dim, a)
    conf = np.random.default_rng(5).uniform(0.05, 1, n).astype(np.float32)
    full = _huber_dev(dev, rows, n, dim, a, conf)
    for mask in range(1, 8):
        want = tuple(bool(mask >> i & 1) for i in range(3))
        got = _huber_dev(dev, rows, n, dim, a, conf, want)
        for w, g, f in zip(want, got, full):
            assert np.array_equal(g, f) if w else np.isnan(g).all(), (want,)
    r = _t(rows, dev)
    assert _lib().gclm_huber_costs(_p(r), n, dim, a, None, None, None, None, _s(dev)) == -3


def test_huber_loss_keeps_the_reference_eps_floor(dev):
    """huber_loss (lm_optimizer.py:79-87) floors isx = max(eps, 1/sqrt(x + 1e-8)) at eps = FLT_EPSILON: beyond
    x = 1/eps^2 (~7.04e13) the first derivative is eps and the second -eps / 2x, and x = +inf gives (inf, eps, -0).  Before
    the floor was restored, the kernel returned 1/sqrt(x) there and a NaN cost at +inf."""
    from geocalib_amd.lm_optimizer import huber_loss, scaled_loss
    xs = np.array([1e13, 7.0e13, 7.1e13, 1e14, 1e20, 3e38, np.inf], np.float32)
    loss, d1, d2 = (_np(t) for t in huber_loss(_t(xs, dev)))
    assert np.array_equal(d1[2:], np.full(5, np.float32(EPS32)))
    assert loss[-1] == np.inf and d2[-1] == 0 and np.signbit(d2[-1])
    for name, r in zip(("cost", "weight", "second"), huber_gate((loss, d1, d2), xs.astype(np.float64), 1.0)):
        assert record(f"huber/floor/{name}", r) <= 1, name
    for a in (1e-2, 3.0):                                      # scaled, through scaled_loss and the C ABI with a confidence
        x = xs * np.float32(a * a)
        sl = [_np(t) for t in scaled_loss(_t(x, dev), huber_loss, a)]
        assert np.array_equal(sl[1][3:], np.full(4, np.float32(EPS32)))
        conf = np.linspace(0.1, 1, len(x)).astype(np.float32)
        got = _huber_dev(dev, x, len(x), 0, a, conf)
        for r in huber_gate(got, x.astype(np.float64), a, conf):
            assert r.max() <= 1
        assert got[0][-1] == np.inf and got[1][-1] == np.float32(EPS32) * conf[-1] and got[2][-1] == 0


def test_huber_second_derivative_carries_no_confidence(dev):
    """gclm_huber_costs multiplies cost and weight by the confidence, not the second derivative (scaled_loss's d2,
    lm_optimizer.py:76, has no confidence in it; include/gclm.h says so).  Before, d2 was scaled by it too."""
    for dim, a in ((0, 1.0), (2, 1e-2), (3, 3.0)):
        n = 1000
        rows = huber_inputs(n, dim, a)
        conf = np.random.default_rng(dim).uniform(0.05, 0.9, n).astype(np.float32)
        with_c = _huber_dev(dev, rows, n, dim, a, conf)
        without = _huber_dev(dev, rows, n, dim, a, None)
        assert (without[2] != 0).sum() > n // 4
        assert np.array_equal(with_c[2], without[2])
        assert np.array_equal(with_c[1], without[1] * conf)


# ------------------------------------------------------------------ gclm_gradient_hessian

def _gh_dev(dev, J, r, w, B, N, R, P, accumulate, G0=None, H0=None):
    G = _t(G0, dev) if accumulate else torch.full((max(B * P, 1),), np.nan, device=dev)
    H = _t(H0, dev) if accumulate else torch.full((max(B * P * P, 1),), np.nan, device=dev)
    Jd, rd, wd = _t(J, dev), _t(r, dev), _t(w, dev)
    rc = _lib().gclm_gradient_hessian(_p(Jd), _p(rd), _p(wd), B, N, R, P, accumulate, _p(G), _p(H), _s(dev))
    assert rc == 0
    return _np(G).reshape(-1)[:B * P].reshape(B, P), _np(H).reshape(-1)[:B * P * P].reshape(B, P, P)


@pytest.mark.parametrize("N", [0, 1, 255, 256, 257, 307200])
def test_gradient_hessian_against_float64(dev, N):
    """gclm_gradient_hessian for P = 1..5, R = 1..4, per entry against the float64 contraction; B = 7 with image 3's
    weights all zero (exactly zero G and H) and every 5th weight zero elsewhere, B = 1 at 307 200 pixels; accumulate = 0
    and 1, the latter onto a symmetric prefill."""
    B = 1 if N > 1000 else 7
    for P in range(1, 6):
        for R in range(1, 5):
            J, r, w = contraction_inputs(B, N, R, P, zero_image=3)
            G0, H0 = symmetric_prefill(B, P)
            for acc in (0, 1):
                G, H = _gh_dev(dev, J, r, w, B, N, R, P, acc, G0, H0)
                pre = (G0, H0) if acc else (None, None)
                G64, H64 = contraction_ref(J, r, w, *pre)
                rg, rh = contraction_gate(G, H, J, r, w, G64, H64, *pre)
                assert record(f"contraction/G/P{P}/R{R}", rg) <= 1 and record(f"contraction/H/P{P}/R{R}", rh) <= 1, \
                    (P, R, acc, rg.max(), rh.max())
                assert np.array_equal(H, H.transpose(0, 2, 1))
                if B > 3 and not acc:
                    assert (G[3] == 0).all() and (H[3] == 0).all()


def test_gradient_hessian_batch_edges_and_arguments(dev):
    """B = 0 is a no-op (nothing written); B = 70 000 at 3 pixels is gated like any batch; R outside 1..4, P outside 1..5,
    negative sizes and every NULL pointer are refused with -3."""
    lib = _lib()
    J, r, w = contraction_inputs(70000, 3, 2, 3)
    G, H = _gh_dev(dev, J, r, w, 70000, 3, 2, 3, 0)
    G64, H64 = contraction_ref(J, r, w)
    rg, rh = contraction_gate(G, H, J, r, w, G64, H64)
    assert record("contraction/G/B70000", rg) <= 1 and record("contraction/H/B70000", rh) <= 1
    Jd, rd, wd = _t(J, dev), _t(r, dev), _t(w, dev)
    Gd, Hd = torch.full((8,), np.nan, device=dev), torch.full((32,), np.nan, device=dev)
    assert lib.gclm_gradient_hessian(_p(Jd), _p(rd), _p(wd), 0, 3, 2, 3, 0, _p(Gd), _p(Hd), _s(dev)) == 0
    assert torch.isnan(Gd).all() and torch.isnan(Hd).all()
    ptrs = [_p(Jd), _p(rd), _p(wd)]
    for B, N, R, P in ((1, 3, 0, 3), (1, 3, 5, 3), (1, 3, 2, 0), (1, 3, 2, 6), (-1, 3, 2, 3), (1, -1, 2, 3)):
        assert lib.gclm_gradient_hessian(*ptrs, B, N, R, P, 0, _p(Gd), _p(Hd), _s(dev)) == -3, (B, N, R, P)
    full = ptrs + [_p(Gd), _p(Hd)]
    for k in range(5):
        args = [None if i == k else v for i, v in enumerate(full)]
        assert lib.gclm_gradient_hessian(*args[:3], 1, 3, 2, 3, 0, *args[3:], _s(dev)) == -3, k
    torch.cuda.synchronize()
    assert torch.isnan(Gd).all() and torch.isnan(Hd).all()


@pytest.mark.parametrize("case", ["pinhole", "simple_radial", "radial", "simple_divisional", "radial+priors",
                                  "simple_radial+priors"])
def test_setup_system_against_float64(dev, oracle, case):
    """setup_system (J_perspective_field + gclm_gradient_hessian per field, then up + latitude) per entry against the
    float64 contraction of the same float32 Jacobians, residuals and weights, for all four models (radial: P = 5) and
    with prior_gravity + prior_focal (radial: P = 2, simple_radial: P = 1)."""
    from geocalib_amd import LMOptimizer
    from geocalib_amd import perspective_fields as pf
    model = case.split("+")[0]
    B, H, W = 3, 33, 47
    cams, gravs = stage_cameras(model, B, H, W, seed=4)
    data = stage_fields(oracle, model, cams, gravs, H, W, wild=False)
    rng = np.random.default_rng(4)
    data["up_confidence"] = rng.uniform(0, 1, (B, H, W)).astype(np.float32)
    data["latitude_confidence"] = rng.uniform(0, 1, (B, H, W)).astype(np.float32)
    dd = {k: _t(v, dev) for k, v in data.items()}
    if case.endswith("+priors"):
        dd["prior_gravity"], dd["prior_focal"] = _t(gravs, dev), _t(cams[:, 3].copy(), dev)
    opt = LMOptimizer({"camera_model": model}).eval()
    opt.setup_optimization_and_priors(dd, shared_intrinsics=False)
    cols = opt._column_dims()
    assert len(cols) == {"radial+priors": 2, "simple_radial+priors": 1}.get(case, 3 + (model != "pinhole") + (model == "radial"))
    cam, grav = _camera(model, cams, gravs, dev)
    res = opt.calculate_residuals(cam, grav, dd)
    _, weights = opt.calculate_costs(res, dd)
    for as_rpf in (False, True):
        G, Hm = (_np(t) for t in opt.setup_system(cam, grav, res, weights, as_rpf=as_rpf))
        flag = opt.conf.use_spherical_manifold and not as_rpf
        J_up, J_lat = (_np(t) for t in pf.J_perspective_field(cam, grav, spherical=flag,
                                                              log_focal=opt.conf.use_log_focal and not as_rpf))
        parts = [(J_up.reshape(B, H * W, 2, -1)[..., cols], _np(res["up_residual"]), _np(weights["up_weights"])),
                 (J_lat.reshape(B, H * W, 1, -1)[..., cols], _np(res["latitude_residual"]), _np(weights["latitude_weights"]))]
        G64 = sum(contraction_ref(*p)[0] for p in parts)
        H64 = sum(contraction_ref(*p)[1] for p in parts)
        gG = sum(contraction_bounds(*p)[0] for p in parts) + U * np.abs(G64)
        gH = sum(contraction_bounds(*p)[1] for p in parts) + U * np.abs(H64)
        rg = np.where(G == G64, 0, np.abs(G - G64) / gG)
        rh = np.where(Hm == H64, 0, np.abs(Hm - H64) / gH)
        assert record(f"setup_system/{case}", np.concatenate([rg.ravel(), rh.ravel()])) <= 1, (as_rpf, rg.max(), rh.max())


# ------------------------------------------------------------------ gclm_optimizer_step

def _step_dev(dev, G, H, lam, eps, failed=True):
    B, P = G.shape
    lam = np.asarray(lam, np.float32)
    Gd, Hd, ld = _t(G, dev), _t(H, dev), _t(lam.reshape(-1), dev)
    d = torch.full((B, P), np.nan, device=dev)
    f = torch.full((B,), -7, dtype=torch.int32, device=dev) if failed else None
    rc = _lib().gclm_optimizer_step(_p(Gd), _p(Hd), _p(ld), int(lam.size == 1), float(eps), B, P, _p(d), _p(f), _s(dev))
    assert rc == 0
    return _np(d), (_np(f) if failed else None)


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5])
def test_optimizer_step_against_float64(dev, P):
    """gclm_optimizer_step on the families of test_stage_oracle.step_families (scalar and per-image lambda incl. 0,
    rank-deficient H made definite by eps, lambda diag H below eps, scaled condition numbers 1e1..1e6, garbage in the
    upper triangle, eps 1e-3) against a float64 Cholesky of the lower triangle; then non-PD, all-zero and NaN systems."""
    for name, (G, H, lam, eps) in step_families(P).items():
        d, f = _step_dev(dev, G, H, lam, eps)
        d64, f64, A = step_ref(G, H, lam, eps)
        r = step_gate(d, f, d64, f64, A)
        assert record(f"step/P{P}/{name}", r) <= 1, (name, r.max())
    G, H = spd_systems(8, P, 10.0, 3)
    Hb, Gb = H.copy(), G.copy()
    Hb[0] = -H[0]                                        # negative definite
    Hb[1] = 0                                            # eps I: definite
    Hb[2, P - 1, 0] = np.nan                             # NaN in the lower triangle (the diagonal for P = 1)
    if P > 1:
        Hb[3, 0, P - 1] = np.nan                         # NaN in the upper triangle only: not read
    Gb[4, 0] = np.nan                                    # NaN gradient, PD H: NaN step, no failure
    Hb[5, P - 1, P - 1] = -10 * abs(H[5, P - 1, P - 1])  # indefinite
    d, f = _step_dev(dev, Gb, Hb, np.float32(0.1), 1e-6)
    d64, f64, A = step_ref(Gb, Hb, np.float32(0.1), 1e-6)
    assert f.tolist() == f64.tolist() == [1, 0, 1, 0, 0, 1, 0, 0]
    assert (d[[0, 2, 5]] == 0).all() and np.isnan(d[4]).all()
    r = step_gate(d, f, d64, f64, A)
    assert record(f"step/P{P}/edges", r) <= 1, r
    clean, _ = _step_dev(dev, G, H, np.float32(0.1), 1e-6)
    assert np.array_equal(d[3], clean[3])
    dn, _ = _step_dev(dev, Gb, Hb, np.float32(0.1), 1e-6, failed=False)      # d_failed = NULL
    assert np.array_equal(dn, d, equal_nan=True)


@pytest.mark.parametrize("B", [1000, 70000])
def test_optimizer_step_results_do_not_depend_on_the_batch(dev, B):
    """Every system of a B-system call equals its own B = 1 call bit for bit (one thread per system, 128-thread blocks:
    B = 70 000 spans 547 of them)."""
    lib = _lib()
    for P in ((1, 2, 3, 4, 5) if B == 1000 else (3, 5)):
        G, H = spd_systems(B, P, 1e3, 9)
        lam = np.random.default_rng(P).uniform(0, 1, B).astype(np.float32)
        d, f = _step_dev(dev, G, H, lam, 1e-6)
        Gd, Hd, ld = _t(G, dev), _t(H, dev), _t(lam, dev)
        one = torch.full((B, P), np.nan, device=dev)
        s = _s(dev)
        for b in range(B):
            lib.gclm_optimizer_step(Gd.data_ptr() + 4 * P * b, Hd.data_ptr() + 4 * P * P * b, ld.data_ptr() + 4 * b, 0,
                                    1e-6, 1, P, one.data_ptr() + 4 * P * b, None, s)
        assert np.array_equal(_np(one), d), P
        assert (f == 0).all()


def test_optimizer_step_python_batch_shapes(dev):
    """optimizer_step on (2, 3, P) batches: the same bits as the flat (6, P) call, per-system and scalar lambda."""
    from geocalib_amd.lm_optimizer import optimizer_step
    for P in (1, 5):
        G, H = spd_systems(6, P, 10.0, 11)
        lam = np.linspace(0, 1, 6).astype(np.float32)
        flat, _ = _step_dev(dev, G, H, lam, 1e-6)
        got = optimizer_step(_t(G.reshape(2, 3, P), dev), _t(H.reshape(2, 3, P, P), dev), _t(lam, dev))
        assert got.shape == (2, 3, P) and np.array_equal(_np(got).reshape(6, P), flat)
        flat, _ = _step_dev(dev, G, H, np.float32(0.1), 1e-6)
        got = optimizer_step(_t(G.reshape(2, 3, P), dev), _t(H.reshape(2, 3, P, P), dev), torch.tensor(0.1, device=dev))
        assert np.array_equal(_np(got).reshape(6, P), flat)


# ------------------------------------------------------------------ gclm_pack_fields

@pytest.mark.parametrize("case", [(1, 2160, 3840, False), (1, 2160, 3839, False), (4100, 8, 8, False), (2, 33, 48, True)])
def test_pack_fields_against_float64(dev, case):
    """pack_fields (gclm_pack_fields) against the head epilogues in float64: saturated tanh (+-30), up vectors of norm
    < 1e-12, 0 and 1e18, logits +-100.  2160 x 3840 (float4 path) and 2160 x 3839 (scalar path) run the grid-stride
    loop in x, 8 x 8 at B = 4100 the one in y, an unaligned view the scalar path; in place gives the same bits."""
    from geocalib_amd.fields import pack_fields
    B, H, W, unaligned = case
    up_raw, lat_raw, ulc, llc = head_inputs(B, H, W)
    ref = head_ref(up_raw, lat_raw, ulc, llc)
    ins = _to_dev({"u": up_raw, "l": lat_raw, "uc": ulc, "lc": llc}, dev, unaligned=unaligned)
    out = pack_fields(ins["u"], ins["l"], ins["uc"], ins["lc"])
    got = [_np(out[k]) for k in ("up_field", "latitude_field", "up_confidence", "latitude_confidence")]
    for name, r in zip(("up", "latitude", "up_conf", "lat_conf"), head_gate(got, ref)):
        assert record(f"pack/{name}", r) <= 1, (name, r.max())
    # in place, on copies with the same alignment (the float4 and scalar paths may differ by rounding; both are gated)
    cp = _to_dev({"u": up_raw, "l": lat_raw, "uc": ulc, "lc": llc}, dev, unaligned=unaligned)
    inp = pack_fields(cp["u"], cp["l"], cp["uc"], cp["lc"], inplace=True)
    for k, g in zip(("up_field", "latitude_field", "up_confidence", "latitude_confidence"), got):
        assert inp[k].data_ptr() == cp[{"up_field": "u", "latitude_field": "l", "up_confidence": "uc",
                                        "latitude_confidence": "lc"}[k]].data_ptr(), k
        assert np.array_equal(_np(inp[k]), g), k
    del out, inp
    bare = pack_fields(ins["u"], ins["l"])
    assert set(bare) == {"up_field", "latitude_field"}
    assert np.array_equal(_np(bare["up_field"]), got[0]) and np.array_equal(_np(bare["latitude_field"]), got[1])
