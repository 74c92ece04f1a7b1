"""GPU: the three-pixel minimal solver on the HIP path (gclm_rpf_hypotheses behind ransac.solve_rpf) against the float64
gate of tests/rpf_gate.py (checked on CPU by test_rpf_solver_abi.py) and against itself -- a sample's rows must depend on its
three pixels alone --, RPFSolver end to end against the truth and against the torch path, and the LM started from it."""
import math

import pytest
import torch

from geocalib_amd import LMOptimizer, Pinhole, RPFSolver, fields, get_trivial_estimation, metrics, ransac, solve_rpf
import hypothesis_gate as hg
import rpf_gate as rg

pytestmark = pytest.mark.gpu

SMALL = (30, 44)
# (roll, pitch, vfov) of the end-to-end cases
E2E = ((10, 20, 60), (10, -20, 40), (0, 0, 70), (25, 0, 90), (-40, 35, 50), (-30, -35, 80), (3, -2, 60), (44, -44, 100))
_cache = {}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def to(data, dev):
    return {k: v.to(dev) for k, v in data.items()}


def rows(out):
    return out["cameras"]._data, out["gravities"]._data


def same(a, b):
    """Bitwise equality of float tensors that hold NaN rows."""
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def hip_case(case, dev, prior=None):
    """The device's rows of a case of rpf_gate (nine images: a call of eight and a call of one), on the CPU."""
    data, samples, f, g = rg.make_case(case)
    cams, gravs = [], []
    for lo, hi in ((0, 8), (8, 9)):
        pred = {k: v[lo:hi].to(dev) for k, v in data.items()}
        if prior is not None:
            pred.pop("latitude_field")
        out = solve_rpf(pred, samples[lo:hi].to(dev), None if prior is None else prior[lo:hi].to(dev))
        assert out["cameras"]._data.is_cuda and out["valid"].dtype == torch.bool and out["samples"].dtype == torch.int32
        assert torch.equal(out["valid"], ~out["cameras"]._data[..., 2].isnan())
        cams.append(out["cameras"]._data.cpu()), gravs.append(out["gravities"]._data.cpu())
    torch.cuda.synchronize()
    return data, samples, f, g, torch.cat(cams), torch.cat(gravs)


@pytest.mark.parametrize("case", rg.CASES, ids=rg.case_id)
def test_against_the_float64_gate(dev, case):
    data, samples, f, g, cam, grav = hip_case(case, dev)
    v = rg.verdict(data, samples, cam, grav)
    print(f"{rg.case_id(case)}: over {max(v['over']):.4f}, worst latitude residual {max(v['worst_deg']):.5f} deg, validity mismatch "
          f"{max(v['mismatch']):.5f}, valid share {min(v['valid']) / (2 * rg.N_GATE):.2f}..{max(v['valid']) / (2 * rg.N_GATE):.2f}")
    assert rg.passes(v), v
    if case[2] == 0.0:
        rate = rg.good_rate(cam, grav, f, g, rg.N_GATE)
        print(f"  known answers: {[round(r, 4) for r in rate.tolist()]}")
        for (roll, pitch, _), r in zip(rg.ALL_POSES, rate.tolist()):
            assert r >= (0.90 if (roll, pitch) == (0, 0) else 0.99), (roll, pitch, r)


@pytest.mark.parametrize("case", [rg.CASES[1], rg.CASES[2]], ids=rg.case_id)
def test_prior_focal(dev, case):
    """One root per sample, f the prior itself, the latitude not read (it is not even given)."""
    data, samples, f, g = rg.make_case(case)
    prior = (f * torch.linspace(0.9, 1.1, len(f))).float()
    data, samples, f, g, cam, grav = hip_case(case, dev, prior)
    v = rg.verdict(data, samples, cam, grav, prior=prior)
    print(f"{rg.case_id(case)} prior: {max(v['over']):.4f} {max(v['mismatch']):.5f}")
    assert rg.passes(v) and cam.shape == (9, rg.N_GATE, 8), v
    valid = ~cam[..., 2].isnan()
    assert (valid.float().mean(1) > 0.9).all() and torch.equal(cam[..., 2][valid], prior[:, None].expand(9, rg.N_GATE)[valid])
    out_of_range = torch.full((9,), 1e5)                 # beyond H / 2 / tan 2.5 deg: every row invalid
    *_, cam, grav = hip_case(case, dev, out_of_range)
    assert cam.isnan().all() and grav.isnan().all()


def drawn(dev, N, B=3, seed=5, first_index=9, H=SMALL[0], W=SMALL[1]):
    """solve_rpf with the in-kernel draw on fixed noisy fields of B poses."""
    key = (B, H, W)
    if key not in _cache:
        _cache[key] = rg.render(rg.ALL_POSES[1:1 + B], H, W, 0.02, seed=3)[0]
    return solve_rpf(to(_cache[key], dev), n=N, seed=seed, first_index=first_index), _cache[key]


def test_in_kernel_draw_is_the_restated_draw(dev):
    N = 257
    out, data = drawn(dev, N)
    mine = rg.draw(5, 9, 3, N, *SMALL)
    assert torch.equal(out["samples"].cpu(), mine)
    given = solve_rpf(to(data, dev), out["samples"])                       # the samples that came back, handed in
    assert same(rows(given)[0], rows(out)[0]) and same(rows(given)[1], rows(out)[1]) and torch.equal(given["samples"], out["samples"])
    again, _ = drawn(dev, N)
    assert same(rows(again)[0], rows(out)[0]) and same(rows(again)[1], rows(out)[1])
    for b in range(3):                                                     # image b alone, first_index advanced
        one = solve_rpf({k: v[b:b + 1].to(dev) for k, v in data.items()}, n=N, seed=5, first_index=9 + b)
        assert torch.equal(one["samples"][0], out["samples"][b])
        assert same(rows(one)[0][0], rows(out)[0][b]) and same(rows(one)[1][0], rows(out)[1][b])
    other, _ = drawn(dev, N, seed=6)
    assert not torch.equal(other["samples"], out["samples"])
    wide = solve_rpf(to(data, dev), n=5, seed=2 ** 63 + 1, first_index=-4)      # 64-bit seed, negative index: wrap-around
    assert torch.equal(wide["samples"].cpu(), rg.draw(2 ** 63 + 1, -4, 3, 5, *SMALL))
    # ... and the package's own copy of the draw, which the torch path uses, so both paths see the same pixels
    assert torch.equal(ransac.draw_samples(5, 9, 3, N, *SMALL), mine)
    cpu = solve_rpf(data, n=N, seed=5, first_index=9)
    assert torch.equal(cpu["samples"], mine) and (cpu["valid"] != out["valid"].cpu()).float().mean() <= rg.VALIDITY_CAP


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_rows_do_not_depend_on_n(dev, N):
    """The edges of the 256-lane block: the rows of the first N samples are the bits of a run of 4000."""
    if "long" not in _cache:
        _cache["long"] = drawn(dev, rg.N_GATE)[0]
    long, (out, data) = _cache["long"], drawn(dev, N)
    assert torch.equal(out["samples"], long["samples"][:, :N])
    assert same(rows(out)[0], rows(long)[0][:, :2 * N]) and same(rows(out)[1], rows(long)[1][:, :2 * N])
    v = rg.verdict(data, long["samples"], *rows(long))
    assert rg.passes(v), v


def test_degenerate_and_non_finite_samples(dev):
    """Identical pixels 0 and 1, a NaN up pixel, a NaN latitude pixel: invalid rows for exactly the samples that touch them,
    every other row keeps its bits.  A pixel outside the image (which the package refuses; handed to the library directly
    here) reads nothing and leaves invalid rows."""
    N = 257
    out, data = drawn(dev, N)
    cam, grav = (t.cpu() for t in rows(out))
    s = out["samples"].cpu().clone()
    H, W = SMALL

    def run(samples, d=data, prior=None):
        o = solve_rpf(to(d, dev), samples.to(dev), prior)
        return o["cameras"]._data.cpu(), o["gravities"]._data.cpu()

    def only(c, g, touched, Rn=2, base=(cam, grav)):
        t = touched.repeat_interleave(Rn, dim=1)
        assert c[t].isnan().all() and g[t].isnan().all()
        assert same(c[~t], base[0][~t]) and same(g[~t], base[1][~t])

    twin = s.clone()
    hit = torch.zeros(3, N, dtype=torch.bool)
    hit[:, [0, 64, 255, 256]] = True
    twin[:, :, 1][hit] = twin[:, :, 0][hit]
    only(*run(twin), hit)
    pc, pg = run(s, prior=torch.full((3,), 30.0, device=dev))
    tc, tg = run(twin, prior=torch.full((3,), 30.0, device=dev))           # with a prior focal f is finite: g is not
    only(tc, tg, hit, Rn=1, base=(pc, pg))
    # NaN pixels: image 1, pixel (x, y) = the first pixel of sample 7 / the latitude pixel of sample 9
    for field, ch, k in (("up_field", 0, 0), ("up_field", 1, 0), ("latitude_field", 0, 2)):
        x, y = s[1, 7 if k == 0 else 9, k].tolist()
        bad = {key: v.clone() for key, v in data.items()}
        bad[field][1, ch, y, x] = math.nan
        where = (s[..., 0] == x) & (s[..., 1] == y)                        # (B, N, 3): which pixel of which sample lies there
        touched = (where[..., :2].any(-1) if field == "up_field" else where[..., 2])
        touched[[0, 2]] = False
        assert touched.any()
        only(*run(s, bad), touched)
    # outside the image, straight to the library
    wild = s.clone()
    hit = torch.zeros(3, N, dtype=torch.bool)
    for i, (n, k, xy) in enumerate(((0, 0, (W, 0)), (63, 1, (0, H)), (64, 2, (-1, 3)), (256, 2, (3, -1)), (100, 0, (2 ** 31 - 1, 0)),
                                    (101, 1, (0, -2 ** 31)))):
        wild[i % 3, n, k] = torch.tensor(xy, dtype=torch.int32)
        hit[i % 3, n] = True
    d = to(data, dev)
    c, g, used = fields.rpf_hypotheses(d["up_field"], d["latitude_field"], None, wild.to(dev))
    torch.cuda.synchronize()
    only(c.cpu(), g.cpu(), hit)
    assert torch.equal(used.cpu(), wild)
    with pytest.raises(ValueError, match="outside"):
        solve_rpf(d, wild.to(dev))


def test_dispatch(dev, monkeypatch):
    out, data = drawn(dev, 65)
    d64 = {k: v.double().to(dev) for k, v in data.items()}
    slow = solve_rpf(d64, out["samples"])                                   # float64 on the device: the torch composition
    assert slow["cameras"]._data.dtype == torch.float64 and slow["cameras"]._data.is_cuda
    both = slow["valid"] & out["valid"]
    assert (slow["valid"] != out["valid"]).float().mean() <= 0.02 and both.float().mean() > 0.4

    def refuse(*a, **k):
        raise AssertionError("the torch composition was called")

    monkeypatch.setattr(ransac, "_solve_torch", refuse)
    solve_rpf(to(data, dev), out["samples"])
    with pytest.raises(AssertionError, match="torch composition"):
        solve_rpf(d64, out["samples"])


# ------------------------------------------------------------------ RPFSolver end to end
def e2e(noise):
    if ("e2e", noise) not in _cache:
        _cache["e2e", noise] = rg.render(E2E, 48, 64, noise, seed=5)
    return _cache["e2e", noise]


def errors(out, f, g):
    cam, grav = out["camera_opt"]._data.double().cpu(), out["gravity_opt"]._data.double().cpu()
    return (cam[:, 2] / f - 1).abs(), torch.rad2deg(torch.acos((grav * g).sum(-1).clamp(-1, 1)))


@pytest.mark.parametrize("noise,deg,rel", [(0.0, 0.1, 0.005), (0.02, 2.0, 0.10)], ids=["noise-free", "noise0.02"])
def test_the_winner_is_near_the_truth(dev, noise, deg, rel):
    data, f, g = e2e(noise)
    solver = RPFSolver({"n_iter": 128, "seed": 1})
    out = solver(to(data, dev))
    torch.cuda.synchronize()
    assert sorted(out) == ["camera_opt", "gravity_opt", "latitude_inliers", "n_valid", "score", "up_inliers"]
    assert type(out["camera_opt"]) is Pinhole and out["camera_opt"].shape == (8,) and out["up_inliers"].shape == (8, 48, 64)
    ferr, ang = errors(out, f, g)
    print(f"noise {noise}: focal {ferr.max():.4f}, gravity {ang.max():.3f} deg, scores {out['score'].tolist()}, valid {out['n_valid'].tolist()}")
    assert (ferr <= rel).all() and (ang <= deg).all(), (ferr, ang)
    assert not out["camera_opt"]._data.isnan().any() and (out["n_valid"] > 64).all()
    # the winner's inlier maps are what its score counted (no confidences, no mask: pixels)
    assert torch.equal(out["up_inliers"].sum((1, 2)) + out["latitude_inliers"].sum((1, 2)), out["score"])
    again = solver(to(data, dev))
    assert torch.equal(again["camera_opt"]._data, out["camera_opt"]._data) and torch.equal(again["score"], out["score"])


def test_hip_and_torch_paths_pick_the_same_winner(dev):
    """Noise 0.02, N = 128, the same pixels on both paths (the draw is one function of the seed).  The HIP `best` is the first
    argmax of the scores it returned; where the torch path's two best scores are further apart than 1 % of H W, both paths
    name the same row."""
    data, f, g = e2e(0.02)
    H, W, N = 48, 64, 128
    hip = solve_rpf(to(data, dev), n=N, seed=1)
    rank = metrics.rank_calibrations(to(data, dev), hip["cameras"], hip["gravities"])
    torch.cuda.synchronize()
    assert torch.equal(rank["best"].cpu(), hg.first_argmax(rank["scores"].cpu()))
    assert (rank["scores"][~hip["valid"]] == 0).all()                      # an invalid row scores exactly 0
    cpu = solve_rpf(data, n=N, seed=1)
    assert torch.equal(cpu["samples"], hip["samples"].cpu())
    sized = cpu["cameras"]._data.clone()
    sized[..., 0], sized[..., 1] = W, H                                    # (the torch ranking reads the size from row 0)
    ref = metrics.rank_calibrations(data, Pinhole(sized), cpu["gravities"])
    top = ref["scores"].topk(2, dim=1).values
    clear = (top[:, 0] - top[:, 1]) > 0.01 * H * W
    print(f"clear winners {clear.tolist()}, hip {rank['best'].tolist()}, torch {ref['best'].tolist()}")
    assert clear.any() and torch.equal(rank["best"].cpu()[clear], ref["best"][clear])


@pytest.mark.parametrize("how", ["float64", "requires_grad", "float64-prior", "masked-float64"])
def test_forward_on_device_tensors_that_take_the_torch_path(dev, how, monkeypatch):
    """Device tensors that are float64 or require grad (a CNN's outputs outside no_grad) take the torch composition of the
    solve AND of the ranking, on the device: about half of the rows the ranking is handed are invalid, the first of a chunk
    among them.  Same pixels as the HIP path (N = 128, seed 1), so the winner is held to the same bounds."""
    from geocalib_amd import fields as F
    data, f, g = e2e(0.0)
    d = to(data, dev)
    if "float64" in how:
        d = {k: v.double() for k, v in d.items()}
    else:
        d = {k: v.clone().requires_grad_(True) for k, v in d.items()}
    if "prior" in how:
        d["prior_focal"] = f.to(dev)
    if "masked" in how:
        d["inliers"] = torch.ones(8, 48, 64, device=dev, dtype=torch.float64)
        d["inliers"][:, :, 40:] = 0

    def refuse(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(F, "rpf_hypotheses", refuse)
    monkeypatch.setattr(F, "hypothesis_scores", refuse)
    monkeypatch.setattr(metrics, "_RANK_CHUNK_PIXELS", 8 * 48 * 64 * 5)      # five rows per chunk: many chunks start on an invalid row
    out = RPFSolver({"n_iter": 128, "seed": 1})(d)
    torch.cuda.synchronize()
    assert out["camera_opt"]._data.is_cuda and out["camera_opt"]._data.dtype == d["up_field"].dtype
    assert not out["camera_opt"]._data.isnan().any() and not out["gravity_opt"]._data.isnan().any()
    assert not out["score"].requires_grad and out["up_inliers"].shape == (8, 48, 64)
    ferr, ang = errors(out, f, g)
    print(f"{how}: focal {ferr.max():.4f}, gravity {ang.max():.3f} deg, valid {out['n_valid'].tolist()}")
    assert (ferr <= 0.005).all() and (ang <= 0.1).all(), (ferr, ang)
    assert (out["n_valid"] > 64).all() and ("prior" in how or (out["n_valid"] < 200).all())             # invalid rows were ranked
    assert (out["score"] > 0).all()


def test_inlier_masks(dev, monkeypatch):
    data, f, g = e2e(0.0)
    H, W = 48, 64
    mask = torch.ones(8, H, W)
    mask[0] = 0                                                            # image 0: no pixel at all
    mask[1, :, W // 2:] = 0                                                # image 1: the left half
    seen = {}
    real = ransac._solve
    monkeypatch.setattr(ransac, "_solve", lambda *a, **k: seen.setdefault("out", real(*a, **k)))
    out = RPFSolver({"n_iter": 128, "seed": 2})({**to(data, dev), "inliers": mask.to(dev)})
    torch.cuda.synchronize()
    s = seen["out"]["samples"].cpu()
    assert s.shape == (8, 128, 3, 2) and (s[1, ..., 0] < W // 2).all() and s[1, ..., 0].max() >= W // 2 - 4 and s[2, ..., 0].max() >= W - 4
    cam0, grav0 = get_trivial_estimation(to(data, dev), Pinhole)
    assert out["score"][0] == 0 and torch.equal(out["camera_opt"]._data[0], cam0._data[0]) and torch.equal(out["gravity_opt"]._data[0], grav0._data[0])
    ferr, ang = errors(out, f, g)
    assert (ferr[1:] <= 0.005).all() and (ang[1:] <= 0.1).all(), (ferr, ang)
    assert out["score"][1] <= 2 * H * W // 2 and (out["score"][1:] > 0).all()
    assert not out["camera_opt"]._data.isnan().any() and not out["gravity_opt"]._data.isnan().any()


# ------------------------------------------------------------------ the LM seam
def test_lm_from_the_ransac_estimate(dev):
    data, f, g = e2e(0.0)
    d = to(data, dev)
    conf = {"camera_model": "pinhole"}
    from_ransac = LMOptimizer({**conf, "init_conf": {"name": "ransac", "n_iter": 128, "seed": 1}}).eval()(dict(d))
    from_trivial = LMOptimizer({**conf, "init_conf": {"name": "trivial"}}).eval()(dict(d))
    torch.cuda.synchronize()
    cam, grav = from_ransac["camera"], from_ransac["gravity"]
    roll = torch.tensor([math.radians(p[0]) for p in E2E])
    pitch = torch.tensor([math.radians(p[1]) for p in E2E])
    print(f"f {(cam.f[:, 1].cpu().double() / f - 1).abs().max():.2e}, roll {(grav.roll.cpu() - roll).abs().max():.2e}, "
          f"pitch {(grav.pitch.cpu() - pitch).abs().max():.2e}, stop_at ransac {from_ransac['stop_at'].tolist()} trivial {from_trivial['stop_at'].tolist()}")
    assert ((cam.f[:, 1].cpu().double() / f - 1).abs() <= 1e-3).all()
    assert ((grav.roll.cpu() - roll).abs() <= 1e-3).all() and ((grav.pitch.cpu() - pitch).abs() <= 1e-3).all()
    assert (from_ransac["stop_at"] <= from_trivial["stop_at"]).all()
    assert sorted(from_ransac) == sorted(from_trivial)
    # a prior focal length passes through solver and solve
    prior = f.float().to(dev)
    fixed = LMOptimizer({**conf, "init_conf": {"name": "ransac", "n_iter": 128}}).eval()({**d, "prior_focal": prior})
    # (the solver's f is the prior bit for bit: test_prior_focal.  The solve holds it fixed as the reference does, through
    # exp(log f + 0) once per step: log f is good to an ulp of log f, which is up to 2-3 ulps of f, times at most 30 steps)
    assert ((fixed["camera"].f[:, 1] / prior - 1).abs() <= 30 * 3 * 2.0 ** -23).all()
    assert ((fixed["gravity"].pitch.cpu() - pitch).abs() <= 1e-3).all() and ((fixed["gravity"].roll.cpu() - roll).abs() <= 1e-3).all()
    # scales: fx takes their aspect, as the trivial estimate's does
    scaled = LMOptimizer({**conf, "init_conf": {"name": "ransac", "n_iter": 128}}).eval()({**d, "scales": torch.tensor([1.5, 1.0])})
    assert torch.allclose(scaled["camera"].f[:, 0], 1.5 * scaled["camera"].f[:, 1], rtol=1e-4)


def test_the_trivial_start_is_untouched(dev):
    """init_conf trivial (and heuristic) take the path they took: forward's result is calibrate_fields' own, bit for bit."""
    data, _, _ = e2e(0.02)
    d = to(data, dev)
    for name in ("trivial", "heuristic"):
        opt = LMOptimizer({"camera_model": "pinhole", "init_conf": {"name": name}}).eval()
        out = opt(dict(d))
        opt.setup_optimization_and_priors(d, shared_intrinsics=False)
        cam, grav, info = opt.calibrate_fields(dict(d))
        torch.cuda.synchronize()
        assert torch.equal(out["camera"]._data, cam._data) and torch.equal(out["gravity"]._data, grav._data)
        assert all(torch.equal(out[k], v) for k, v in info.items()), name
