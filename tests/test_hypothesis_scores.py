"""GPU: metrics.rank_calibrations on the HIP path (gclm_hypothesis_scores) against the float64 yardstick of
tests/hypothesis_gate.py (checked on CPU by test_hypothesis_scores_abi.py), against gclm_field_errors, which is gated
already, and against itself: a hypothesis' bits must not depend on N, on its index, on the other hypotheses or images."""
import math

import pytest
import torch

from geocalib_amd import Gravity, LMOptimizer, camera_models, fields, get_trivial_estimation, metrics
import field_error_gate as fg
import hypothesis_gate as hg
import perspective_gate as pg

pytestmark = pytest.mark.gpu

K = fields.HYPOTHESIS_CHUNK
_C = {(c[0], c[2], c[3]): c for c in fg.CASES if not c[5]}
WAYS = ("all", "noconf", "up", "lat")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def on_device(t, dev, offset4=False):
    """`t` on the device; with `offset4` in a buffer that starts 4 bytes past an aligned address."""
    if t is None or not offset4:
        return None if t is None else t.to(dev)
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    flat[1:].copy_(t.reshape(-1))
    return flat[1:].view(t.shape)


def wrappers(model, hc, hgv, dev):
    cam, grav = camera_models[model](hc.to(dev)), Gravity(hgv.to(dev))
    grav._data = hgv.to(dev)                      # as stored: the cases' gravities are scored as they are
    return cam, grav


def rank(case, hc, hgv, data, dev, mask=None, **kw):
    """The device's answer in the form hypothesis_gate.verdict takes, and rank_calibrations' own dict."""
    cam, grav = wrappers(case[0], hc, hgv, dev)
    out = metrics.rank_calibrations({k: on_device(v, dev, case[5]) for k, v in data.items()}, cam, grav,
                                    mask=on_device(mask, dev, case[5]), **kw)
    torch.cuda.synchronize()
    assert all(out[k].dtype == torch.float32 for k in ("scores", "up_scores", "latitude_scores")) and out["best"].dtype == torch.int64
    return {"scores": torch.stack([out["up_scores"], out["latitude_scores"], out["scores"]], -1), "best": out["best"]}, out


def check(case, dev, N=7):
    cams, gravs, data = fg.make_case(case)
    hc, hgv = hg.hypotheses(cams, gravs, N)
    for which in WAYS:
        d = fg.subset(data, which)
        res, _ = rank(case, hc, hgv, d, dev)
        v = hg.verdict(hg.yardstick(case, hc, hgv, d), res)
        print(f"{fg.case_id(case)} N={N} {which}: {v}")
        assert hg.passes(v), (which, v)
        if "up_field" not in d:
            assert (res["scores"][..., 0] == 0).all()
        if "latitude_field" not in d:
            assert (res["scores"][..., 1] == 0).all()


@pytest.mark.parametrize("case", fg.CASES + fg.EXTREMES, ids=fg.case_id)
def test_parity_against_float64(dev, case):
    check(case, dev)


@pytest.mark.parametrize("N", [1, K - 1, K, K + 1, 2 * K + 3])
@pytest.mark.parametrize("model", ["pinhole", "simple_divisional"])
def test_parity_across_the_chunk_edges(dev, model, N):
    check(_C[model, 37, 53], dev, N)


@pytest.mark.parametrize("case,kw,masked", [(_C["simple_radial", 37, 53], dict(up_weight=0.75, latitude_weight=0.3), True),
                                            (_C["radial", 30, 200], dict(up_weight=0.75, latitude_weight=0.3), True),
                                            (_C["simple_divisional", 9, 132], dict(up_weight=2.0, latitude_weight=0.5, up_threshold=3.0,
                                                                                  latitude_threshold=0.5), False)],
                         ids=["mask-37x53", "mask-30x200", "weights-thresholds"])
def test_parity_with_mask_weights_and_thresholds(dev, case, kw, masked):
    cams, gravs, data = fg.make_case(case)
    hc, hgv = hg.hypotheses(cams, gravs, 7)
    mask = hg.make_mask(case) if masked else None
    res, _ = rank(case, hc, hgv, data, dev, mask, **kw)
    y = hg.yardstick(case, hc, hgv, data, (kw.get("up_threshold", 1.0), kw.get("latitude_threshold", 1.0)),
                     (kw["up_weight"], kw["latitude_weight"]), mask)
    v = hg.verdict(y, res)
    print(f"{fg.case_id(case)} {kw}: {v}")
    assert hg.passes(v), v


@pytest.mark.parametrize("model", ["pinhole", "simple_divisional"])
def test_counts_equal_those_of_field_errors(dev, model):
    """Without confidences and mask a score is a count of pixels, exact in float32: it must equal recall@t H W of
    gclm_field_errors at the same calibration, hypothesis by hypothesis -- both kernels compile the same per-pixel functions."""
    case = _C[model, 30, 200]
    cams, gravs, data = fg.make_case(case)
    hc, hgv = hg.hypotheses(cams, gravs, 7)
    d = fg.subset(data, "noconf")
    res, _ = rank(case, hc, hgv, d, dev)
    hw = case[2] * case[3]
    for n in range(7):
        stats, _, _ = fields.field_errors(model, hc[:, n].to(dev), hgv[:, n].to(dev), d["up_field"].to(dev), d["latitude_field"].to(dev),
                                          None, None, (1.0,))
        counts = (stats[:, [2, 5]].double() * hw).round()
        assert torch.equal(res["scores"][:, n, :2].double(), counts), (n, res["scores"][:, n, :2], counts)


@pytest.mark.parametrize("case", [_C["pinhole", 37, 53], _C["simple_divisional", 30, 200]], ids=fg.case_id)
def test_a_hypothesis_does_not_depend_on_its_company(dev, case):
    cams, gravs, data = fg.make_case(case)
    N = 2 * K + 3
    hc, hgv = hg.hypotheses(cams, gravs, N)
    full, _ = rank(case, hc, hgv, data, dev)
    again, _ = rank(case, hc, hgv, data, dev)
    assert torch.equal(full["scores"], again["scores"]) and torch.equal(full["best"], again["best"])      # NaN-free: equal is bitwise
    assert not full["scores"].isnan().any()
    i, j = hg.PAIR
    assert torch.equal(full["scores"][:, i], full["scores"][:, j])
    for n in (0, i, K - 1, K, N - 1):             # alone: N = 1
        alone, _ = rank(case, hc[:, n:n + 1], hgv[:, n:n + 1], data, dev)
        assert torch.equal(alone["scores"][:, 0], full["scores"][:, n]), n
    back, _ = rank(case, hc.flip(1), hgv.flip(1), data, dev)               # at another position, among other chunk mates
    assert torch.equal(back["scores"].flip(1), full["scores"])
    short, _ = rank(case, hc[:, 3:K + 2], hgv[:, 3:K + 2], data, dev)      # another N, shifted
    assert torch.equal(short["scores"], full["scores"][:, 3:K + 2])
    d = {k: on_device(v, dev) for k, v in data.items()}
    for b in range(case[1]):                      # image b alone, its planes where they lie in the batch
        cam, grav = wrappers(case[0], hc[b:b + 1], hgv[b:b + 1], dev)
        one = metrics.rank_calibrations({k: v[b:b + 1] for k, v in d.items()}, cam, grav)
        assert torch.equal(one["scores"][0], full["scores"][b, :, 2]) and torch.equal(one["up_scores"][0], full["scores"][b, :, 0])
        assert one["best"][0] == full["best"][b]
    # the identical pair first and second: equal totals, the lower index wins
    pair, _ = rank(case, hc[:, [0, j, i, 5]], hgv[:, [0, j, i, 5]], data, dev)
    assert torch.equal(pair["scores"][:, 1], pair["scores"][:, 2])
    assert pair["best"][-1] == 1, pair                                     # the last image's prediction is the exact target


def test_non_finite_inputs(dev):
    case = _C["pinhole", 30, 200]
    cams, gravs, data = fg.make_case(case)
    hc, hgv = hg.hypotheses(cams, gravs, K + 2)
    clean, _ = rank(case, hc, hgv, data, dev)
    # a hypothesis with a NaN focal length scores exactly 0, the others keep their bits
    bad_c = hc.clone()
    bad_c[:, 3, 2:4] = math.nan
    out, _ = rank(case, bad_c, hgv, data, dev)
    keep = [n for n in range(K + 2) if n != 3]
    assert (out["scores"][:, 3] == 0).all() and torch.equal(out["scores"][:, keep], clean["scores"][:, keep])
    bad_g = hgv.clone()
    bad_g[0, K, 1] = math.nan
    out, _ = rank(case, hc, bad_g, data, dev)
    assert (out["scores"][0, K] == 0).all() and torch.equal(out["scores"][1], clean["scores"][1])
    assert torch.equal(out["scores"][0, :K], clean["scores"][0, :K])
    # one NaN confidence pixel: that image's scores of that field are NaN for every hypothesis, best is the first index
    for key, col, other in (("up_confidence", 0, 1), ("latitude_confidence", 1, 0)):
        bad = {k: v.clone() for k, v in data.items()}
        bad[key][1, 10, 7] = math.nan
        out, _ = rank(case, hc, hgv, bad, dev)
        assert out["scores"][1, :, col].isnan().all() and out["scores"][1, :, 2].isnan().all() and out["best"][1] == 0
        assert torch.equal(out["scores"][1, :, other], clean["scores"][1, :, other])
        assert torch.equal(out["scores"][0], clean["scores"][0]) and out["best"][0] == clean["best"][0]
    # a NaN prediction pixel hits for no hypothesis; nothing else moves (without confidences: the scores are counts)
    d = fg.subset(data, "noconf")
    counts, _ = rank(case, hc, hgv, d, dev)
    for field, ch, col, other, key in (("up_field", 0, 0, 1, "up_error"), ("up_field", 1, 0, 1, "up_error"),
                                       ("latitude_field", 0, 1, 0, "latitude_error")):
        bad = {k: v.clone() for k, v in d.items()}
        bad[field][1, ch, 10, 7] = math.nan
        out, _ = rank(case, hc, hgv, bad, dev)
        for n in range(K + 2):
            cam, grav = wrappers(case[0], hc[:, n], hgv[:, n], dev)
            e = metrics.perspective_field_metrics({k: v.to(dev) for k, v in d.items()}, cam, grav, (1.0,), return_errors=True)[key]
            assert out["scores"][1, n, col] == counts["scores"][1, n, col] - float(e[1, 10, 7] < 1.0), (field, n)
        assert torch.equal(out["scores"][1, :, other], counts["scores"][1, :, other]) and torch.equal(out["scores"][0], counts["scores"][0])


def test_dispatch(dev, monkeypatch):
    case = _C["pinhole", 37, 53]
    cams, gravs, data = fg.make_case(case)
    hc, hgv = hg.hypotheses(cams, gravs, 3)
    cam, grav = wrappers(case[0], hc, hgv, dev)
    d = {k: v.to(dev) for k, v in data.items()}

    def refuse(*a, **k):
        raise AssertionError("torch path called")

    monkeypatch.setattr(metrics, "_rank_torch", refuse)
    out = metrics.rank_calibrations(d, cam, grav)
    assert sorted(out) == ["best", "camera", "gravity", "latitude_scores", "scores", "up_scores"]
    flat = metrics.rank_calibrations(d, *wrappers(case[0], hc.reshape(-1, 8), hgv.reshape(-1, 3), dev))       # the (B N) order
    assert torch.equal(flat["scores"], out["scores"])
    with pytest.raises(AssertionError, match="torch path"):
        metrics.rank_calibrations({k: v.double() for k, v in d.items()}, cam, grav)
    with pytest.raises(AssertionError, match="torch path"):
        metrics.rank_calibrations({**d, "up_field": d["up_field"].clone().requires_grad_(True)}, cam, grav)
    monkeypatch.undo()
    slow = metrics.rank_calibrations({k: v.double() for k, v in d.items()}, camera_models[case[0]](hc.double().to(dev)),
                                     wrappers(case[0], hc, hgv.double(), dev)[1])
    csum = d["up_confidence"].double().sum((1, 2)) + d["latitude_confidence"].double().sum((1, 2))
    assert ((slow["scores"] - out["scores"].double()).abs() <= 0.01 * csum[:, None]).all()


def test_ranking_solves_from_several_initialisations():
    """8 noise-free pinhole images at 48 x 64, solved from the trivial and from the heuristic initialisation: ranked together
    with the trivial initial estimate itself, the initial estimate never wins; and the winner, scored alone by
    perspective_field_metrics, has the recall@1 its score implies."""
    import numpy as np
    from oracle import synth
    dev = torch.device("cuda:0")
    B, H, W = 8, 48, 64
    raw, _, _ = synth.make_fields(11, range(B), "pinhole", H, W, noise=0.0, confidences=False)
    data = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in raw.items()}
    runs = [LMOptimizer({"camera_model": "pinhole", "init_conf": {"name": name}}).eval()(data) for name in ("trivial", "heuristic")]
    cam0, grav0 = get_trivial_estimation(data, camera_models["pinhole"])
    cams = torch.stack([r["camera"]._data for r in runs] + [cam0._data], 1).contiguous()
    gravs = torch.stack([r["gravity"]._data for r in runs] + [grav0._data], 1).contiguous()
    grav = Gravity(gravs)
    grav._data = gravs
    out = metrics.rank_calibrations(data, camera_models["pinhole"](cams), grav)
    torch.cuda.synchronize()
    print(out["best"].tolist(), out["scores"].tolist())
    assert (out["best"] != 2).all() and out["camera"].shape == (B,)
    rows = torch.arange(B, device=dev)
    assert (out["scores"][rows, out["best"]] > out["scores"][:, 2]).all()
    m = metrics.perspective_field_metrics(data, out["camera"], out["gravity"], (1.0,))
    assert torch.equal((m["up_angle_recall@1.0"].double() * H * W).round(), out["up_scores"][rows, out["best"]].double())
    assert torch.equal((m["latitude_angle_recall@1.0"].double() * H * W).round(), out["latitude_scores"][rows, out["best"]].double())


def test_64_bit_offsets(dev):
    """B * H * W = 520 * 2048 * 2048 > 2^31: the last image's latitude plane (8.7 GB in all) lies beyond every 32-bit offset.
    Its scores equal those of the image scored alone, bit for bit."""
    from geocalib_amd import perspective_fields as pf
    B, H, W = 520, 2048, 2048
    if torch.cuda.get_device_properties(dev).total_memory < 24 * 2 ** 30:
        pytest.skip("needs 24 GB of device memory")
    cams, gravs = pg.make_cameras("simple_radial", B, H, W, seed=9), pg.make_gravity(B, seed=9)
    moved = fg._perturbed(cams, gravs, 1.0)
    lat = pf.get_latitude_field(*wrappers("simple_radial", *moved, dev)).view(B, 1, H, W)
    hc, hgv = hg.hypotheses(cams, gravs, 2)      # scales 1.2 and 0.1: 0.6 and 2.7 degrees from the prediction
    cam, grav = wrappers("simple_radial", hc, hgv, dev)
    batch = metrics.rank_calibrations({"latitude_field": lat}, cam, grav)
    last = metrics.rank_calibrations({"latitude_field": lat[-1:]}, *wrappers("simple_radial", hc[-1:], hgv[-1:], dev))
    first = metrics.rank_calibrations({"latitude_field": lat[:1]}, *wrappers("simple_radial", hc[:1], hgv[:1], dev))
    torch.cuda.synchronize()
    assert batch["scores"].shape == (B, 2) and (batch["up_scores"] == 0).all()
    assert torch.equal(batch["scores"][-1], last["scores"][0]) and torch.equal(batch["scores"][0], first["scores"][0])
    assert (batch["best"] == 0).all() and (batch["scores"][:, 0] > batch["scores"][:, 1]).all() and (batch["scores"][:, 0] > 0.5 * H * W).all()
