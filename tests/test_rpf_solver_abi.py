"""CPU: the three-pixel minimal solver without a device -- gclm_rpf_hypotheses is declared, exported and bound, refuses its
invalid arguments before any HIP call, fields.rpf_hypotheses hands it the arguments of include/gclm.h; the in-kernel draw as
the header states it; ransac.solve_rpf's torch composition against the gate of tests/rpf_gate.py (which must fail its
mutants), against the known answers and against what the reference's solver returned on recorded inputs
(tests/golden/rpf_reference.npz); RPFSolver's conf and its refusals, the LM seam's refusals; and the kernel's code object."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from geocalib_amd import LMOptimizer, RPFSolver, _lib, fields, ransac, solve_rpf
from abi_harness import HEADER, LLVM, declared
import rpf_gate as rg
from test_host_calls import MAX, STREAM, p, rec  # noqa: F401  (the recorder fixture, not edited)
from conftest import ROOT

ARGS = ["const float*", "const float*", "const float*", "const int32_t*", "uint64_t", "int64_t", "int", "int", "int", "int",
        "float*", "float*", "int32_t*", "void*"]


def test_entry_point_is_declared_exported_and_bound():
    # (abi_harness.assert_declared_exported_and_bound knows int and size_t scalars only: the 64-bit pair is checked here)
    assert declared("gclm_rpf_hypotheses") == ARGS
    res, args = _lib._SIGNATURES["gclm_rpf_hypotheses"]
    assert res is C.c_int and len(args) == len(ARGS) and args[4] is C.c_uint64 and args[5] is C.c_int64 and args[6:10] == [C.c_int] * 4
    assert "gclm_rpf_hypotheses" in _lib.EXPORTED_SYMBOLS and hasattr(C.CDLL(_lib.LIB_PATH), "gclm_rpf_hypotheses")
    assert _lib.load().gclm_version() == 610 == _lib.ABI_VERSION
    assert all(a is C.c_void_p for a in args[:4] + args[10:])
    header = open(HEADER).read()
    assert "gclm_rpf_hypotheses" in header[header.index("ABI version:"):header.index("#define GCLM_VERSION")]
    assert int(re.search(r"#define GCLM_RPF_DRAW_SALT (0x[0-9A-Fa-f]+)ull", header).group(1), 16) == _lib.RPF_DRAW_SALT == rg.SALT
    assert f"#define GCLM_RPF_MAX_SAMPLES (1 << 24)" in header and _lib.RPF_MAX_SAMPLES == 1 << 24
    # the focal range is the LM's own clamp, constant for constant
    device = open(os.path.join(ROOT, "geocalib_amd", "csrc", "gclm_device.h")).read()
    for c in (rg.TAN_MAX, rg.TAN_MIN):
        assert f"{c}f" in device and f"{c}f" in open(os.path.join(ROOT, "geocalib_amd", "csrc", "gclm_rpf.hip")).read() and str(c) in header
    assert (ransac._TAN_MAX, ransac._TAN_MIN) == (rg.TAN_MAX, rg.TAN_MIN) and ransac.focal_range(48) == rg.focal_range(48)


def test_the_solver_s_constants_do_not_hang_on_the_chunk_override():
    """A build with -DGCLM_HYPOTHESIS_CHUNK=8 or 32 (the measured variants of gclm_hypotheses.hip) overrides one define of
    include/gclm.h; the solver's constants must be defined in such a build too."""
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or f"{LLVM}/clang"
    for flags in ([], ["-DGCLM_HYPOTHESIS_CHUNK=8"], ["-DGCLM_HYPOTHESIS_CHUNK=32"]):
        out = subprocess.run([cc, "-E", "-dM", "-x", "c", *flags, HEADER], capture_output=True, text=True, check=True).stdout
        macros = dict(re.findall(r"#define (GCLM_\w+) (.+)", out))
        assert macros["GCLM_HYPOTHESIS_CHUNK"] == (flags[0].split("=")[1] if flags else "16")
        assert macros["GCLM_RPF_MAX_SAMPLES"] == "(1 << 24)" and macros["GCLM_RPF_DRAW_SALT"] == "0x5250465F44524157ull", flags


# fake, never dereferenced device addresses: every call below must be refused before the first HIP call
UP, LAT, PRIOR, SAMPLES, CAM, GRAV, OUT = 0x4000000, 0x8000000, 0xC000000, 0x10000000, 0x20000000, 0x30000000, 0x40000000
OK = dict(up=UP, lat=LAT, prior=None, samples=SAMPLES, seed=1, first=0, B=2, N=7, H=48, W=64, cam=CAM, grav=GRAV, out=OUT)
PX = 48 * 64 * 4
BAD = [("NULL up", dict(up=None)), ("NULL camera rows", dict(cam=None)), ("NULL gravity rows", dict(grav=None)),
       ("NULL latitude without a prior focal", dict(lat=None)), ("N = 0", dict(N=0)), ("N = -1", dict(N=-1)),
       ("N over the limit", dict(N=(1 << 24) + 1)), ("B = 0", dict(B=0)), ("B > 65535", dict(B=65536)), ("H = 0", dict(H=0)),
       ("W = 0", dict(W=0)), ("H * W > 2^31 - 1", dict(H=65536, W=32768)),
       ("up misaligned", dict(up=UP + 2)), ("latitude misaligned", dict(lat=LAT + 1)), ("prior misaligned", dict(prior=PRIOR + 2)),
       ("samples misaligned", dict(samples=SAMPLES + 2)), ("camera rows misaligned", dict(cam=CAM + 1)),
       ("gravity rows misaligned", dict(grav=GRAV + 2)), ("samples_out misaligned", dict(out=OUT + 3)),
       ("camera rows overlap up", dict(cam=UP + 2 * 2 * PX - 4)), ("camera rows overlap the latitude", dict(cam=LAT - 4)),
       ("gravity rows overlap the samples", dict(grav=SAMPLES + 2 * 7 * 24 - 4)), ("gravity rows overlap the camera rows", dict(grav=CAM + 2 * 14 * 32 - 4)),
       ("samples_out is the samples", dict(out=SAMPLES)), ("samples_out overlaps the gravity rows", dict(out=GRAV + 2 * 14 * 12 - 4)),
       ("camera rows overlap the prior", dict(prior=PRIOR, cam=PRIOR + 4))]


def _call_abi(a):
    return _lib.load().gclm_rpf_hypotheses(a["up"], a["lat"], a["prior"], a["samples"], a["seed"], a["first"], a["B"], a["N"], a["H"],
                                           a["W"], a["cam"], a["grav"], a["out"], None)


@pytest.mark.parametrize("what,change", BAD, ids=[b[0] for b in BAD])
def test_invalid_arguments_are_refused_before_any_hip_call(what, change):
    assert _call_abi({**OK, **change}) == -3, what


def test_a_sample_outside_the_image_is_refused():
    """The samples live in device memory, where the C entry cannot look: the package refuses them before the call (the
    kernel reads nothing for such a sample and leaves invalid rows: test_rpf_solver.py)."""
    data, _, _ = rg.render(((10, 20, 60),), 30, 44)
    good = torch.tensor([[[[0, 0], [43, 29], [5, 7]]]])
    assert solve_rpf(data, good)["cameras"].shape == (1, 2)
    for bad in ([44, 0], [0, 30], [-1, 3], [3, -1]):
        s = good.clone()
        s[0, 0, 1] = torch.tensor(bad)
        with pytest.raises(ValueError, match="outside"):
            solve_rpf(data, s)
    for shape in ((1, 1, 3), (1, 0, 3, 2), (2, 1, 3, 2), (1, 1, 2, 2)):
        with pytest.raises(ValueError):
            solve_rpf(data, torch.zeros(shape, dtype=torch.int64))
    with pytest.raises(ValueError):
        solve_rpf(data, good.float())
    with pytest.raises(ValueError, match="at least one"):
        solve_rpf(data, n=0)
    with pytest.raises(ValueError, match="prior_focal"):
        solve_rpf({"up_field": data["up_field"]})


# ------------------------------------------------------------------ the call path (the recorder of test_host_calls.py)
def test_rpf_hypotheses_hands_over_the_arguments_of_the_header(rec):  # noqa: F811
    up, lat = torch.randn(2, 2, 3, 5), torch.randn(2, 1, 3, 5)
    cam, grav, samples = fields.rpf_hypotheses(up, lat, n=9, seed=2 ** 64 + 5, first_index=11)
    assert cam.shape == (2, 18, 8) and grav.shape == (2, 18, 3) and samples.shape == (2, 9, 3, 2) and samples.dtype == torch.int32
    (name, a), = rec.calls
    assert name == "gclm_rpf_hypotheses" and len(a) == len(ARGS)
    assert a == (p(up), p(lat), None, None, 5, 11, 2, 9, 3, 5, p(cam), p(grav), p(samples), STREAM)
    del rec.calls[:]
    given = torch.zeros(2, 4, 3, 2, dtype=torch.int32)
    prior = torch.tensor([3.0, 4.0])
    cam, grav, used = fields.rpf_hypotheses(up, lat, prior, given)
    assert used is given and cam.shape == (2, 4, 8)
    assert rec.calls[0][1] == (p(up), None, p(prior), p(given), 0, 0, 2, 4, 3, 5, p(cam), p(grav), None, STREAM)
    with pytest.raises(ValueError):
        fields.rpf_hypotheses(up)
    with pytest.raises(ValueError):
        fields.rpf_hypotheses(up, lat, samples=given.long())
    with pytest.raises(ValueError):
        fields.rpf_hypotheses(up, lat, n=0)


def test_rpf_hypotheses_slices_and_advances_every_pointer(rec):  # noqa: F811
    B = MAX + 2
    up, lat, prior = torch.zeros(B, 2, 1, 1), torch.zeros(B, 1, 1, 1), torch.ones(B)
    cam, grav, samples = fields.rpf_hypotheses(up, lat, n=3, seed=7, first_index=100)
    (_, first), (_, second) = rec.calls
    assert first == (p(up), p(lat), None, None, 7, 100, MAX, 3, 1, 1, p(cam), p(grav), p(samples), STREAM)
    assert second == (p(up) + MAX * 8, p(lat) + MAX * 4, None, None, 7, 100 + MAX, 2, 3, 1, 1, p(cam) + MAX * 6 * 32, p(grav) + MAX * 6 * 12,
                      p(samples) + MAX * 3 * 24, STREAM)
    del rec.calls[:]
    cam, grav, _ = fields.rpf_hypotheses(up, None, prior, samples)
    assert rec.calls[1][1][:4] == (p(up) + MAX * 8, None, p(prior) + MAX * 4, p(samples) + MAX * 72)
    assert rec.calls[1][1][10:12] == (p(cam) + MAX * 3 * 32, p(grav) + MAX * 3 * 12)


# ------------------------------------------------------------------ the draw
def test_the_draw_is_the_header_s():
    B, N, H, W = 3, 70, 30, 44
    mine = rg.draw(5, 9, B, N, H, W)
    assert torch.equal(ransac.draw_samples(5, 9, B, N, H, W), mine)
    x, y = mine[..., 0], mine[..., 1]
    assert x.min() >= 0 and x.max() < W and y.min() >= 0 and y.max() < H
    assert x.max() >= W - 3 and y.max() >= H - 3 and x.min() <= 2 and y.min() <= 2             # ... and fills it
    # a function of (seed, first_index + b, n, k) alone: image b alone, a longer run, another seed
    assert torch.equal(rg.draw(5, 9 + 2, 1, N, H, W)[0], mine[2]) and torch.equal(rg.draw(5, 9, B, 20, H, W), mine[:, :20])
    assert not torch.equal(rg.draw(6, 9, B, N, H, W), mine) and not torch.equal(mine[0], mine[1])
    assert len({tuple(r.flatten().tolist()) for r in mine.reshape(-1, 3, 2)}) == B * N
    big = ransac.draw_samples(2 ** 63 + 1, -4, 2, 5, 7, 2 ** 15)                                # wrap-around arithmetic
    assert torch.equal(big, rg.draw(2 ** 63 + 1, -4, 2, 5, 7, 2 ** 15))
    out = solve_rpf(rg.render(((10, 20, 60),) * B, H, W)[0], n=N, seed=5, first_index=9)
    assert torch.equal(out["samples"], mine)


# ------------------------------------------------------------------ the torch composition against the gate, and the gate itself
def _torch_rows(case, prior=None):
    data, samples, f, g = rg.make_case(case)
    out = solve_rpf(data if prior is None else {"up_field": data["up_field"]}, samples, prior)
    assert out["cameras"]._data.dtype == torch.float32 and torch.equal(out["valid"], ~out["cameras"]._data[..., 2].isnan())
    return data, samples, f, g, out["cameras"]._data, out["gravities"]._data


@pytest.mark.parametrize("case", rg.CASES, ids=rg.case_id)
def test_the_torch_composition_passes_the_gate(case):
    data, samples, f, g, cam, grav = _torch_rows(case)
    v = rg.verdict(data, samples, cam, grav)
    print(f"{rg.case_id(case)}: over {max(v['over']):.4f}, worst latitude residual {max(v['worst_deg']):.5f} deg, validity mismatch "
          f"{max(v['mismatch']):.5f}, valid share {min(v['valid']) / (2 * rg.N_GATE):.2f}..{max(v['valid']) / (2 * rg.N_GATE):.2f}")
    assert rg.passes(v), v
    data, samples, f, g, cam, grav = _torch_rows(case, f.float())
    v = rg.verdict(data, samples, cam, grav, prior=f.float())
    assert rg.passes(v) and cam.shape[1] == rg.N_GATE, v


@pytest.mark.parametrize("case", [c for c in rg.CASES if c[2] == 0.0], ids=rg.case_id)
def test_known_answers(case):
    """Noise-free fields: at least 99 % of the samples have a valid root within 0.5 degrees and 2 % of the truth, 90 % for
    the level camera, where half the pixels have sin(latitude) near 0."""
    data, samples, f, g, cam, grav = _torch_rows(case)
    rate = rg.good_rate(cam, grav, f, g, rg.N_GATE)
    print(f"{rg.case_id(case)}: {[round(r, 4) for r in rate.tolist()]}")
    for (roll, pitch, _), r in zip(rg.ALL_POSES, rate.tolist()):
        assert r >= (0.90 if (roll, pitch) == (0, 0) else 0.99), (roll, pitch, r)
    valid = (~cam[..., 2].isnan()).float().mean(1)
    assert valid.min() > 0.4 and valid.max() < 0.75
    # with the true focal length as prior every sample has one root, the gravity alone is estimated
    data, samples, f, g, cam, grav = _torch_rows(case, f.float())
    # (the level camera's up vectors are all equal: two pixels of one column, 1 / W of the samples, span no vanishing point)
    for (roll, pitch, _), r in zip(rg.ALL_POSES, rg.good_rate(cam, grav, f, g, rg.N_GATE).tolist()):
        assert r >= (0.90 if (roll, pitch) == (0, 0) else 0.99), (roll, pitch, r)


# (mutant, the case that must reject it, why)
REJECTS = [("divide_vz", (64, 64, 0.0), "the level camera: V_z = 0"), ("swap_pp", (48, 64, 0.0), "a non-square image"),
           ("swap_pp", (30, 44, 0.02), "a non-square image"), ("sign_from_vz", (64, 64, 0.0), "pitch < 0"),
           ("sign_from_vz", (48, 64, 0.02), "pitch < 0"), ("keep_spurious", (64, 64, 0.0), "the squared equation's other root"),
           ("keep_spurious", (30, 44, 0.02), "the squared equation's other root"), ("no_range", (64, 64, 0.0), "pitch 0: a0 is rounding noise"),
           ("textbook", (48, 64, 0.0), "pitch 0: a0 is rounding noise")]


@pytest.mark.parametrize("mutant,case,why", REJECTS, ids=[f"{m}-{rg.case_id(c)}" for m, c, _ in REJECTS])
def test_gate_rejects_each_mutant(mutant, case, why):
    assert case in rg.CASES
    data, samples, _, _ = rg.make_case(case)
    rows = rg.as_rows(*rg.solve(data, samples, None, torch.float32, mutant), case[0], case[1])
    v = rg.verdict(data, samples, *rows)
    print(f"{mutant} on {rg.case_id(case)} ({why}): over {max(v['over']):.3f} mismatch {max(v['mismatch']):.3f} range {v['range']}")
    assert not rg.passes(v), v
    honest = rg.as_rows(*rg.solve(data, samples, None, torch.float32), case[0], case[1])       # the same code without the error
    assert rg.passes(rg.verdict(data, samples, *honest))


def test_gate_counts_structure_norm_and_range():
    case = rg.CASES[0]
    data, samples, f, g, cam, grav = _torch_rows(case)
    first = int((~cam[0, :, 2].isnan()).nonzero()[0])
    for change, key in ((lambda c, gr: c[0, first, 4].fill_(1.0), "structure"), (lambda c, gr: gr[0, first].mul_(1 + 1e-6), "norm"),
                        (lambda c, gr: c[0, first, 2:4].fill_(1e4), "range"), (lambda c, gr: gr[0, first, 1].fill_(float("nan")), "structure")):
        c, gr = cam.clone(), grav.clone()
        change(c, gr)
        v = rg.verdict(data, samples, c, gr)
        assert v[key] >= 1 and not rg.passes(v), (key, v)


# ------------------------------------------------------------------ the reference, where it is right
def test_against_the_reference_solver():
    """tests/golden/rpf_reference.npz (make_golden_rpf.py): the reference's solve_rpf on noisy 64 x 64 fields.  On the rows
    that are valid here and that the reference's roll / pitch formulas can express (g_y < 0, g_z > 0) one of its two roots
    matches within 1e-3 relative in f and 0.05 degrees in roll and pitch; misses (the reference's root formula cancels, its
    roots are not range-checked) are capped at 2 % per pose."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "rpf_reference.npz"))
    data = {"up_field": torch.from_numpy(z["up_field"]), "latitude_field": torch.from_numpy(z["latitude_field"])}
    samples = torch.from_numpy(z["samples"].astype(np.int32))
    out = solve_rpf(data, samples)
    B, N = samples.shape[:2]
    f, g = out["cameras"]._data[..., 2].reshape(B, N, 2).double(), out["gravities"]._data.reshape(B, N, 2, 3).double()
    ref = torch.stack([torch.from_numpy(z["rpf_pos"]), torch.from_numpy(z["rpf_neg"])], 2).double()        # (B, N, root, (roll, pitch, f))
    roll, pitch = torch.asin(-g[..., 0] / torch.sqrt(1 - g[..., 2] ** 2)), torch.asin(g[..., 2])           # MinimalSolver.solve_rp
    sel = out["valid"].reshape(B, N, 2) & (g[..., 1] < 0) & (g[..., 2] > 0)
    close = ((f[..., None] / ref[:, :, None, :, 2] - 1).abs() < 1e-3) & \
        (torch.rad2deg((roll[..., None] - ref[:, :, None, :, 0]).abs()) < 0.05) & \
        (torch.rad2deg((pitch[..., None] - ref[:, :, None, :, 1]).abs()) < 0.05)
    miss = ((~close.any(-1)) & sel).reshape(B, -1).sum(1) / sel.reshape(B, -1).sum(1)
    print(f"rows compared {sel.reshape(B, -1).sum(1).tolist()}, misses {[round(m, 4) for m in miss.tolist()]}")
    assert (sel.reshape(B, -1).sum(1) > 2000).all() and (miss <= 0.02).all(), miss


# ------------------------------------------------------------------ RPFSolver and the LM seam, off the device
def test_default_conf_keys_are_the_reference_s():
    reference = {"n_iter": 1000, "up_inlier_th": 1, "latitude_inlier_th": 1, "error_fn": "angle", "up_weight": 1, "latitude_weight": 1,
                 "loss_weight": 1, "use_latitude": True}               # siclib/models/optimization/ransac.py: RPFSolver.default_conf
    assert {k: v for k, v in RPFSolver.default_conf.items() if k != "seed"} == reference
    assert list(RPFSolver.default_conf)[:8] == list(reference) and RPFSolver.default_conf["seed"] == 0
    assert not hasattr(RPFSolver, "loss")


def test_refusals():
    with pytest.raises(NotImplementedError, match="angle"):
        RPFSolver({"error_fn": "mse"})
    with pytest.raises(ValueError, match="unknown"):
        RPFSolver({"n_iters": 3})
    for n in (0, 40000):
        with pytest.raises(ValueError, match="n_iter"):
            RPFSolver({"n_iter": n})
    data, _, _ = rg.render(((10, 20, 60),), 30, 44)
    with pytest.raises(ValueError, match="prior_focal"):
        RPFSolver({"use_latitude": False, "n_iter": 4})(data)
    # the LM seam: refused before anything touches a device
    lm = LMOptimizer({"init_conf": {"name": "ransac", "n_iter": 16}})
    for extra, word in (({"prior_gravity": torch.tensor([[0.0, -1.0, 0.0]])}, "prior_gravity"), ({"prior_dist": torch.zeros(1)}, "prior_dist")):
        with pytest.raises(ValueError, match=word):
            lm({**data, **extra})
    with pytest.raises(ValueError, match="shared_intrinsics"):
        LMOptimizer({"init_conf": {"name": "ransac"}, "shared_intrinsics": True})(data)
    with pytest.raises(ValueError, match="up_field"):
        lm({"latitude_field": data["latitude_field"]})
    with pytest.raises(NotImplementedError):                              # the solver's conf errors surface at construction
        LMOptimizer({"init_conf": {"name": "ransac", "error_fn": "mse"}})
    with pytest.raises(ValueError, match="n_iter"):
        LMOptimizer({"init_conf": {"name": "ransac", "n_iter": 0}})
    assert isinstance(lm.ransac, RPFSolver) and lm.ransac.conf.n_iter == 16 and not hasattr(LMOptimizer({}), "ransac")
    import inspect
    assert list(inspect.signature(solve_rpf).parameters) == ["pred", "samples", "prior_focal", "n", "seed", "first_index"]
    with pytest.raises(RuntimeError, match="HIP device"):                 # ... and what is not refused goes on to the device
        lm(data)


def test_rpf_solver_forward_off_the_device():
    """The torch path end to end on two small noise-free images: the winner is the truth, the outputs have the reference's
    keys and shapes; an empty `inliers` mask gives the trivial estimate and score 0; a half mask draws inside it."""
    H, W = 24, 32
    poses = ((10, -20, 60), (-30, 35, 80))
    data, f, g = rg.render(poses, H, W)
    solver = RPFSolver({"n_iter": 24, "seed": 3})
    out = solver(dict(data))
    assert sorted(out) == ["camera_opt", "gravity_opt", "latitude_inliers", "n_valid", "score", "up_inliers"]
    assert out["camera_opt"].shape == (2,) and out["up_inliers"].shape == (2, H, W) == out["latitude_inliers"].shape
    assert ((out["camera_opt"]._data[:, 2].double() / f - 1).abs() < 5e-3).all()
    assert (torch.rad2deg(torch.acos((out["gravity_opt"]._data.double() * g).sum(-1).clamp(-1, 1))) < 0.1).all()
    assert (out["score"] > 1.5 * H * W).all() and (out["n_valid"] > 12).all()
    assert torch.equal(out["up_inliers"].sum((1, 2)) + out["latitude_inliers"].sum((1, 2)), out["score"])
    again = solver(dict(data))
    assert torch.equal(again["camera_opt"]._data, out["camera_opt"]._data) and torch.equal(again["score"], out["score"])
    m = solver.metrics(out, {"camera": out["camera_opt"], "gravity": out["gravity_opt"]})
    assert sorted(m) == ["pitch_opt_error", "roll_opt_error", "vfov_opt_error"] and all((v == 0).all() for v in m.values())
    # masks: image 0 empty, image 1 its left half
    mask = torch.zeros(2, H, W)
    mask[1, :, :W // 2] = 1
    seen = {}
    real = ransac._solve
    try:
        ransac._solve = lambda *a, **k: seen.setdefault("out", real(*a, **k))
        out = solver({**data, "inliers": mask})
    finally:
        ransac._solve = real
    s = seen["out"]["samples"]
    assert s.shape == (2, 24, 3, 2) and (s[1, ..., 0] < W // 2).all() and s[1, ..., 0].max() > W // 4
    assert out["score"][0] == 0 and out["score"][1] > 0.5 * H * W
    from geocalib_amd import Pinhole, get_trivial_estimation
    cam0, grav0 = get_trivial_estimation(data, Pinhole)
    assert torch.equal(out["camera_opt"]._data[0], cam0._data[0]) and torch.equal(out["gravity_opt"]._data[0], grav0._data[0])
    assert not out["camera_opt"]._data.isnan().any() and ((out["camera_opt"]._data[1, 2].double() / f[1] - 1).abs() < 5e-3)
    # a prior focal length is honoured: one root per sample, f is the prior
    out = solver({**data, "prior_focal": f.float()})
    assert torch.equal(out["camera_opt"]._data[:, 2], f.float()) and (out["n_valid"] <= 24).all()
    # images on which no sample is valid (a NaN up field): the trivial estimate, score 0, no NaN
    bad = {"up_field": data["up_field"].clone(), "latitude_field": data["latitude_field"]}
    bad["up_field"][0] = float("nan")
    out = solver(bad)
    assert out["n_valid"][0] == 0 and out["score"][0] == 0 and torch.equal(out["camera_opt"]._data[0], cam0._data[0])


# ------------------------------------------------------------------ code object
@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="LLVM tools missing")
def test_rpf_kernels_carry_no_scratch_and_no_lds(tmp_path):
    from test_kernel_audit import kernel_metadata
    k = {n: v for n, v in kernel_metadata(tmp_path).items() if "rpf_kernel" in n}
    print(k)
    assert len(k) == 2 and any("ILb0E" in n for n in k) and any("ILb1E" in n for n in k), sorted(k)
    assert all(v["scratch"] == 0 and v["lds"] == 0 and v["vgpr"] <= 64 for v in k.values()), k          # (64 VGPRs: eight waves per SIMD)
