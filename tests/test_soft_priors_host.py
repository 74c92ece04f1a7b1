"""Soft priors without a GPU: the float64 yardstick's two limits, the host's ValueErrors (raised before the library is
touched) and gclm_calibrate_soft at the C ABI -- declared, exported, bound, and -3 for invalid arguments before any HIP call
(fake device addresses, never dereferenced).

The limits anchor the new branch of lm_grad.lm_unrolled_torch to what the loop already did: with standard deviations so wide
that the priors carry no weight (1e6 px, 1e6 rad) it must give the free solve, started from the same initial estimate (a
prior seeds the initial estimate, so the free run is handed the soft run's) and run for the same number of steps; with
standard deviations so tight that the data carry none (1e-4 px, 1e-6 rad) it must return the priors, which is the hard
prior's answer.  float64, B = 3, 24 x 32, priors 10 % and 0.07 rad off the truth; both bounds are 1e-9."""
import pytest
import torch

from geocalib_amd import LMOptimizer, _lib, lm_grad
from abi_harness import HEADER, assert_declared_exported_and_bound
from soft_prior_cases import conf_for, make, state, with_priors

B, H, W, SEED = 3, 24, 32, 11


@pytest.mark.parametrize("model", ["pinhole", "simple_radial"])
def test_wide_priors_give_the_free_solve_from_the_same_start(model):
    data, priors, _, _ = make(model, B, H, W, SEED)
    conf = conf_for(model, "huber")
    wide = with_priors(data, priors, "both", torch.full((B,), 1e6), torch.full((B,), 1e6))
    opt = LMOptimizer(dict(conf))
    init = lm_grad._initial_estimate(opt, wide, torch.float64)
    soft = lm_grad.lm_unrolled_torch(wide, conf)
    free = lm_grad.lm_unrolled_torch(data, conf, init=init)
    assert soft["deltas"].shape == free["deltas"].shape == (5, B, 3 + (model != "pinhole"))
    (fs, gs, ks), (ff, gf, kf) = state(soft), state(free)
    assert float((fs / ff - 1).abs().max()) < 1e-9
    assert float((gs - gf).abs().max()) < 1e-9
    assert float((ks - kf).abs().max()) < 1e-9 * max(1.0, float(kf.abs().max()))
    assert float(soft["final_prior_cost"].max()) < 1e-9 and torch.equal(soft["final_cost"], soft["final_up_cost"]
                                                                       + soft["final_latitude_cost"] + soft["final_prior_cost"])
    # the free run's dict is the one it always was
    assert "final_prior_cost" not in free and "initial_prior_cost" not in free


@pytest.mark.parametrize("model", ["pinhole", "simple_radial"])
def test_tight_priors_give_the_hard_priors_answer(model):
    data, priors, _, _ = make(model, B, H, W, SEED)
    tight = with_priors(data, priors, "both", torch.full((B,), 1e-4), torch.full((B,), 1e-6))
    out = lm_grad.lm_unrolled_torch(tight, conf_for(model, "huber"))
    fy, g, _ = state(out)
    assert float((fy / priors["prior_focal"].double() - 1).abs().max()) < 1e-9
    g0 = priors["prior_gravity"].double()
    g0 = g0 / g0.norm(dim=-1, keepdim=True)
    angle = torch.atan2(torch.linalg.cross(g, g0).norm(dim=-1), (g * g0).sum(-1))
    assert float(angle.max()) < 1e-9


def test_the_yardstick_without_the_keys_is_unchanged_and_a_lone_uncertainty_raises():
    data, priors, _, _ = make("pinhole", B, H, W, SEED)
    conf = conf_for("pinhole", "huber", steps=2)
    hard = lm_grad.lm_unrolled_torch({**data, "prior_focal": priors["prior_focal"]}, conf)
    assert hard["deltas"].shape[-1] == 2 and "initial_prior_cost" not in hard        # the focal column is frozen, as ever
    soft = lm_grad.lm_unrolled_torch({**data, "prior_focal": priors["prior_focal"], "prior_focal_uncertainty": torch.full((B,), 5.0)}, conf)
    # the column is free; the prior seeds the start (its cost there is float32 rounding of the estimate) and pulls afterwards
    assert soft["deltas"].shape[-1] == 3 and float(soft["initial_prior_cost"].max()) < 1e-12 < float(soft["final_prior_cost"].min())
    with pytest.raises(ValueError, match="prior_gravity"):
        lm_grad.lm_unrolled_torch({**data, "prior_gravity_uncertainty": torch.full((B,), 0.1)}, conf)


# ------------------------------------------------------------------------------------------ the host's refusals
def fields():
    return {"up_field": torch.zeros(2, 2, 6, 8), "latitude_field": torch.zeros(2, 1, 6, 8)}


FOCAL = {"prior_focal": torch.full((2,), 9.0), "prior_focal_uncertainty": torch.full((2,), 1.0)}
GRAVITY = {"prior_gravity": torch.tensor([[0.0, -1.0, 0.0]] * 2), "prior_gravity_uncertainty": torch.full((2,), 0.1)}


@pytest.mark.parametrize("conf, data, limit", [
    ({"shared_intrinsics": True}, FOCAL, "shared_intrinsics"),
    ({"differentiable": True}, FOCAL, "differentiable"),
    ({"init_conf": {"name": "ransac"}}, GRAVITY, "ransac"),
    ({"use_log_focal": False}, FOCAL, "use_log_focal"),
    ({"use_spherical_manifold": False}, GRAVITY, "use_spherical_manifold"),
    ({}, {**FOCAL, "prior_focal_uncertainty": torch.tensor([1.0, 0.0])}, "finite and > 0"),
    ({}, {**FOCAL, "prior_focal_uncertainty": torch.tensor([1.0, -2.0])}, "finite and > 0"),
    ({}, {**GRAVITY, "prior_gravity_uncertainty": torch.tensor([float("nan"), 0.1])}, "finite and > 0"),
    ({}, {**GRAVITY, "prior_gravity_uncertainty": torch.tensor([float("inf"), 0.1])}, "finite and > 0"),
    ({}, {"prior_focal_uncertainty": torch.full((2,), 1.0)}, "needs `prior_focal`"),
    ({}, {"prior_gravity_uncertainty": torch.full((2,), 0.1)}, "needs `prior_gravity`"),
    ({}, {**FOCAL, "prior_focal_uncertainty": torch.full((3,), 1.0)}, "one value per image"),
])
def test_unsupported_combinations_raise_before_the_library_is_touched(monkeypatch, conf, data, limit):
    def touched(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", touched)
    opt = LMOptimizer(dict(conf))
    if conf.get("shared_intrinsics"):
        opt.shared_intrinsics = True
    with pytest.raises(ValueError, match=limit):
        opt({**fields(), **data})


def test_a_soft_prior_keeps_its_column_free_and_both_keys_are_sliced_per_image():
    opt = LMOptimizer({"camera_model": "simple_radial"})
    opt.setup_optimization_and_priors({**FOCAL, "prior_gravity": GRAVITY["prior_gravity"]})
    assert opt.estimate_focal and not opt.estimate_gravity and opt.focal_delta_dims == (0,)
    opt.setup_optimization_and_priors({**FOCAL, **GRAVITY})
    assert opt.estimate_focal and opt.estimate_gravity and opt._column_dims() == [0, 1, 2, 3]
    opt.setup_optimization_and_priors({"prior_focal": FOCAL["prior_focal"]})
    assert not opt.estimate_focal
    import inspect
    src = inspect.getsource(LMOptimizer._calibrate_chunked)
    assert '"prior_focal_uncertainty"' in src and '"prior_gravity_uncertainty"' in src


# ------------------------------------------------------------------------------------------ the C ABI
F, I = "const float*", "int"
SOFT = ["gclm_handle*", F, F, F, F, I, I, I, F, F, F, F, I, F, F, "float*", "float*", "float*", "float*", F, "void*"]


def test_entry_point_is_declared_exported_and_bound():
    assert_declared_exported_and_bound("gclm_calibrate_soft", SOFT)
    header = open(HEADER).read()
    assert "gclm_calibrate_soft" in header[header.index("ABI version:"):header.index("#define GCLM_VERSION")]
    assert f"#define GCLM_INFO_STRIDE {_lib.INFO_STRIDE}\n" in header and _lib.INFO_STRIDE == 48


UP, LAT, UPC, LATC, SC, PF, PG, PD = 0x4000000, 0x8000000, 0xC000000, 0x10000000, 0x14000000, 0x14100000, 0x14200000, 0x14300000
SF, SG, CAM, GRAV, INFO, COST, SLAT = 0x14400000, 0x14500000, 0x18000000, 0x18100000, 0x18200000, 0x18300000, 0x1C000000
OK = dict(up=UP, lat=LAT, upc=UPC, latc=LATC, B=2, H=48, W=64, sc=SC, pf=PF, pg=PG, pd=None, nd=0, sf=SF, sg=SG, cam=CAM, grav=GRAV,
          info=INFO, cost=COST, slat=None)
PX = 2 * 48 * 64 * 4
BAD = [("focal sigma without its prior", dict(pf=None)), ("gravity sigma without its prior", dict(pg=None)),
       ("NULL latitude", dict(lat=None)), ("NULL camera", dict(cam=None)), ("NULL gravity", dict(grav=None)),
       ("NULL info", dict(info=None)), ("B = 0", dict(B=0)), ("B < 0", dict(B=-1)), ("B > 65535", dict(B=65536)), ("H = 0", dict(H=0)),
       ("W = 0", dict(W=0)), ("focal sigma misaligned", dict(sf=SF + 2)), ("gravity sigma misaligned", dict(sg=SG + 1)),
       ("cost misaligned", dict(cost=COST + 2)), ("cost is the focal sigma", dict(cost=SF)), ("cost overlaps the info rows", dict(cost=INFO + 64)),
       ("camera overlaps the gravity sigma", dict(cam=SG - 16)), ("info overlaps the latitude", dict(info=LAT + PX - 4)),
       ("cost overlaps the prior gravity", dict(cost=PG + 8)), ("prior_dist_cols 3", dict(pd=PD, nd=3))]


def _soft(h, a):
    return _lib.load().gclm_calibrate_soft(h, a["up"], a["lat"], a["upc"], a["latc"], a["B"], a["H"], a["W"], a["sc"], a["pf"], a["pg"],
                                           a["pd"], a["nd"], a["sf"], a["sg"], a["cam"], a["grav"], a["info"], a["cost"], a["slat"], None)


@pytest.mark.parametrize("what,change", BAD, ids=[b[0] for b in BAD])
def test_invalid_arguments_are_refused_before_any_hip_call(what, change):
    """The arguments are checked before the handle is looked at: no handle (creating one needs a device) is needed to see it."""
    assert _soft(None, {**OK, **change}) == -3, what
    assert "gclm_calibrate_soft" in _lib.last_error(None)


def test_valid_arguments_reach_the_handle_and_no_sigma_is_the_plain_call():
    assert _soft(None, OK) == -1
    assert _soft(None, {**OK, "sf": None, "sg": None, "lat": None}) == -1      # gclm_calibrate_ex exactly: its own checks, its own order


def _create(**over):
    cfg = _lib.GclmConfig.default(0)
    for k, v in over.items():
        setattr(cfg, k, v)
    h = _lib.C.c_void_p()
    assert _lib.load().gclm_create(_lib.C.byref(h), _lib.C.byref(cfg)) == 0, _lib.last_error(None)
    return h


@pytest.mark.gpu
@pytest.mark.parametrize("over, code", [(dict(shared_intrinsics=1), -3), (dict(use_log_focal=0), -3), (dict(use_spherical_manifold=0), -3),
                                        (dict(estimate_focal=0), -2)],
                         ids=["shared_intrinsics", "use_log_focal off", "use_spherical_manifold off", "a frozen focal column"])
def test_configurations_without_soft_priors_are_refused_before_any_launch(over, code):
    """(a handle exists only where a device does; the fake addresses are still never dereferenced)"""
    h = _create(**over)
    try:
        assert _soft(h, OK) == code and _lib.last_error(h)
    finally:
        _lib.load().gclm_destroy(h)
