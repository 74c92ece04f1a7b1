"""GPU: PerspectiveParamOpt on the HIP path (gclm_param_opt, gclm_param_opt_cost, gclm_param_opt_step) against what the
reference's module computed on the same fields (tests/golden/param_opt_reference.npz, written by
tests/golden/make_golden_param_opt.py) and against torch.optim run live; section 9 holds the pass at its branch edges, ragged
tiles and batches to the bound tests/param_opt_gate.py derives on the CPU.  Every test prints the figures it gates."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from geocalib_amd import Gravity, PerspectiveParamOpt, Pinhole, _lib, perspective_opt
from conftest import MEASURED
import param_opt_gate as pg

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
STOP_OFF = {"abs_tol": -1.0, "rel_tol": 0.0}
SMALL = (0, 1, 2)                             # the 48 x 64 images of golden


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def data_of(images, dev, offset=0):
    """The golden fields of `images` as one batch on the device; with `offset` each tensor starts that many floats past a
    256-byte aligned address."""
    out = {}
    for k, j in (("up_field", 0), ("latitude_field", 1)):
        t = torch.from_numpy(np.concatenate([pg.fields(i)[j] for i in images]))
        flat = torch.empty(t.numel() + offset, dtype=t.dtype, device=dev)
        flat[offset:].copy_(t.reshape(-1))
        out[k] = flat[offset:].view(t.shape)
    return out


def run(images, dev, conf=None, **kw):
    out = PerspectiveParamOpt(conf or {})(data_of(images, dev), **kw)
    torch.cuda.synchronize()
    return out


def bits(out):
    return {k: out[k].cpu().numpy().tobytes() for k in ("rpv", "steps", "converged", "final_cost", "final_up_cost",
                                                        "final_latitude_cost", "lr", "initial")}


# ------------------------------------------------------------------ 1. cost and gradient
@pytest.mark.parametrize("i", range(7))
def test_cost_and_gradient_against_the_reference_float64(i, dev):
    """Golden (a): each of the eight numbers no further from the reference's float64 autograd than the reference's own float32
    autograd is at that state, with a floor of 16 * 2^-23 relative to the largest gradient entry of its term.  A state the
    maker still rejected after two retries (a pixel within 1e-6 of a sign switch: worth 1 / (H W) of a gradient in any float32
    evaluation) is held on its two costs only; its gradients are printed."""
    g = pg.golden()
    worst = 0.0
    for s in range(2):
        rpv = torch.from_numpy(g["states"][i, s].astype(np.float32))[None].to(dev)
        out = perspective_opt.cost_function(rpv, data_of([i], dev))
        got = torch.cat([out["up"][:, None], out["latitude"][:, None], out["up_grad"], out["latitude_grad"]], 1)[0].double().cpu().numpy()
        want, ref32 = g["cost64"][i, s], g["cost32"][i, s]
        for cost, grad in ((0, slice(2, 5)), (1, slice(5, 8))):
            floor = 16 * ULP * np.abs(want[grad]).max()
            idx = [cost] + ([] if g["rejected"][i, s] else list(range(grad.start, grad.stop)))
            for k in idx:
                err, bound = abs(got[k] - want[k]), max(abs(ref32[k] - want[k]), floor)
                print(f"image {i} state {s} number {k}: hip {got[k]:+.9e} f64 {want[k]:+.9e} err {err:.2e} ref32 err {abs(ref32[k] - want[k]):.2e} "
                      f"floor {floor:.2e} ratio {err / bound:.3f}")
                worst = max(worst, err / bound)
        if g["rejected"][i, s]:
            print(f"image {i} state {s} rejected by the maker: gradients {got[2:]} against float64 {want[2:]}")
    print(f"image {i}: largest ratio {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("i,offsets", [(3, (1,)), (0, (1, 2, 4)), (6, (1, 2))], ids=["33x47", "48x64", "120x160"])
def test_unaligned_planes_give_the_aligned_values_to_summation_order(i, offsets, dev):
    """Planes that start 1, 2 or 4 floats past an aligned address take one, two or four pixels per lane; the eight numbers equal
    the aligned copy's to summation order: 4 * 2^-23 of the largest entry of their term (33 x 47 is odd: one pixel per lane
    either way, the same bits)."""
    g = pg.golden()
    rpv = torch.from_numpy(g["states"][i, 1].astype(np.float32))[None].to(dev)
    def numbers(offset):
        out = perspective_opt.cost_function(rpv, data_of([i], dev, offset))
        return torch.cat([out["up"][:, None], out["latitude"][:, None], out["up_grad"], out["latitude_grad"]], 1)[0].double().cpu().numpy()
    base = numbers(0)
    for offset in offsets:
        got = numbers(offset)
        for sl in (slice(0, 1), slice(1, 2), slice(2, 5), slice(5, 8)):
            err = np.abs(got[sl] - base[sl]).max() / np.abs(base[sl]).max()
            print(f"image {i} offset {offset} {sl}: {err:.2e}")
            assert err <= 4 * ULP
        if g["sizes"][i][1] % 2:
            assert np.array_equal(got, base)


# ------------------------------------------------------------------ 2. initial estimate
def test_initial_estimate_equals_the_reference_to_4_ulp(dev):
    g = pg.golden()
    for i in range(7):
        out = run([i], dev, {"max_steps": 1})
        got, want = out["initial"][0].double().cpu().numpy(), g["init64"][i]
        ulps = np.abs(got - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        print(f"image {i}: initial {got} reference {want} ulps {ulps}")
        assert (ulps <= 4).all()


# ------------------------------------------------------------------ 3. the state machine
@pytest.mark.parametrize("name", ["stopping off", "default", "loose rel_tol", "cooldown and floor", "no scheduler"])
def test_state_machine_on_the_device_equals_torch(name, dev):
    """gclm_param_opt_step fed the three recorded 200-step sequences at once: the lr after every step, the steps at which it
    was reduced and the step of the stop are torch's; the parameters lie within steps * 2^-23 * max(1, |param|) of torch's
    float64 ones (one rounding per step)."""
    from test_param_opt_abi import MACHINES
    g = pg.golden()
    conf = MACHINES[name]
    cfg = _lib.GclmParamOptConfig.default()
    for k, v in conf.items():
        setattr(cfg, k, v)
    seq, rpv0 = g["sequence"], g["init64"][:3].astype(np.float32)
    want = [pg.torch_replay(seq[b], rpv0[b].astype(np.float64), **conf) for b in range(3)]
    state = torch.from_numpy(pg.fresh_state(rpv0, cfg.lr).view(np.int32)).to(dev)
    costs = torch.from_numpy(seq).to(dev).transpose(0, 1).contiguous()          # (200, 3, 8)
    stream = torch.cuda.current_stream(dev).cuda_stream
    lrs, params, done = [], [], []
    for t in range(seq.shape[1]):
        assert _lib.load().gclm_param_opt_step(state.data_ptr(), costs[t].data_ptr(), 3, C.byref(cfg), stream) == 0
        s = pg.read_state(state.cpu().numpy().view(np.uint32))
        lrs.append(s["lr"]), params.append(s["rpv"]), done.append(s["done"])
    lrs, params, done = np.array(lrs), np.array(params), np.array(done)
    for b in range(3):
        t_params, t_lrs, t_stop = want[b]
        n = len(t_lrs)
        stop = int(np.argmax(done[:, b])) + 1 if done[:, b].any() else 0
        worst = (np.abs(params[:n, b] - t_params) / ((np.arange(n)[:, None] + 1) * ULP * np.maximum(1, np.abs(t_params)))).max()
        print(f"{name} sequence {b}: stop {stop} (torch {t_stop}), lr reductions at {(np.flatnonzero(np.diff(lrs[:n, b])) + 2).tolist()}, "
              f"final lr {lrs[n - 1, b]:.3e}, parameters within {worst:.3f} of the bound")
        assert stop == t_stop
        assert np.array_equal(lrs[:n, b], t_lrs)
        assert worst <= 1.0
        if stop:                              # a converged record freezes
            assert (params[n:, b] == params[n - 1, b]).all() and (lrs[n:, b] == lrs[n - 1, b]).all()


# ------------------------------------------------------------------ 4. fixed-length runs
@pytest.mark.parametrize("i", range(7))
def test_fixed_length_runs_against_the_reference_float64(i, dev):
    """Golden (b), stopping off: after K = 1, 5, 20, 100 steps within 3x the reference's own float32 spread of that case (the
    largest |float32 - float64| over its nine float32 runs and three parameters), never tighter than 16 * 2^-23 * K rad."""
    g = pg.golden()
    for k, K in enumerate(g["ks"].tolist()):
        out = run([i], dev, {**STOP_OFF, "max_steps": K})
        got = out["rpv"][0].double().cpu().numpy()
        err, spread = np.abs(got - g["fixed64"][i, k]).max(), g["fixed_spread"][i, k].max()
        bound = max(3 * spread, 16 * ULP * K)
        print(f"image {i} K {K}: err {math.degrees(err):.2e} deg, reference spread {math.degrees(spread):.2e} deg, ratio to bound {err / bound:.3f}, "
              f"ratio to spread {err / spread:.3f}")
        assert int(out["steps"][0]) == K and not bool(out["converged"][0])
        assert err <= bound


# ------------------------------------------------------------------ 5. default conf
@pytest.mark.parametrize("i", range(7))
def test_default_conf_against_the_reference_float64(i, dev):
    """Golden (c): within 3x the reference's own float32 spread of the case (never tighter than 16 * 2^-23 * steps rad), 1 <=
    steps <= max_steps, converged, and within 0.3 degrees of the pose the fields were rendered at."""
    g = pg.golden()
    out = run([i], dev)
    got, steps = out["rpv"][0].double().cpu().numpy(), int(out["steps"][0])
    err, spread = np.abs(got - g["default64"][i]).max(), g["default_spread"][i].max()
    bound = max(3 * spread, 16 * ULP * steps)
    miss = np.degrees(np.abs(got - np.radians(g["poses"][i])))
    print(f"image {i}: steps {steps} (reference float64 {g['default_steps64'][i]}, float32 {g['default_steps32'][i].tolist()}), err "
          f"{math.degrees(err):.2e} deg, reference spread {math.degrees(spread):.2e} deg, ratio to bound {err / bound:.3f}, miss of the truth "
          f"{miss.round(4).tolist()} deg, final cost {float(out['final_cost'][0]):.6e}, lr {float(out['lr'][0]):.1e}")
    assert 1 <= steps <= 1000
    assert bool(out["converged"][0])
    assert err <= bound
    assert miss.max() <= 0.3


# ------------------------------------------------------------------ 6. batching
def test_a_batch_gives_each_image_the_bits_of_that_image_alone(dev):
    """Fast and slow stoppers in one call: per image the bits of that image solved alone, `steps` included; two calls give
    the same bits; poll_every = 0 and poll_every = 7 give the same bits."""
    batch = run(SMALL, dev)
    steps = batch["steps"].tolist()
    print("steps of the batch", steps)
    assert len(set(steps)) > 1
    again = run(SMALL, dev)
    assert bits(batch) == bits(again)
    for b, i in enumerate(SMALL):
        alone = run([i], dev)
        for k in ("rpv", "steps", "converged", "final_cost", "final_up_cost", "final_latitude_cost", "lr", "initial"):
            assert torch.equal(alone[k][0], batch[k][b]), (i, k, alone[k], batch[k][b])
    assert bits(run(SMALL, dev, {"poll_every": 0})) == bits(batch) == bits(run(SMALL, dev, {"poll_every": 7}))
    # the order inside a batch does not matter either
    flipped = run(SMALL[::-1], dev)
    assert torch.equal(flipped["rpv"].flip(0), batch["rpv"]) and torch.equal(flipped["steps"].flip(0), batch["steps"])


# ------------------------------------------------------------------ 7. NaN
def test_a_nan_pixel_stays_in_its_image(dev):
    conf = {"max_steps": 5}
    clean = PerspectiveParamOpt(conf)(data_of(SMALL, dev))
    data = data_of(SMALL, dev)
    data["latitude_field"][1, 0, 7, 9] = math.nan
    out = PerspectiveParamOpt(conf)(data)
    torch.cuda.synchronize()
    assert not bool(out["converged"][1]) and int(out["steps"][1]) == 5
    assert math.isnan(float(out["final_cost"][1])) and math.isnan(float(out["final_latitude_cost"][1]))
    for b in (0, 2):
        for k in ("rpv", "steps", "converged", "final_cost", "final_up_cost", "final_latitude_cost", "lr"):
            assert torch.equal(out[k][b], clean[k][b]), (b, k)
    data = data_of(SMALL, dev)
    data["up_field"][1, 1, 40, 3] = math.nan
    out = PerspectiveParamOpt(conf)(data)
    assert math.isnan(float(out["final_up_cost"][1])) and not bool(out["converged"][1])
    assert torch.equal(out["rpv"][[0, 2]], clean["rpv"][[0, 2]])


# ------------------------------------------------------------------ 8. the Python module
def test_module_dict_in_dict_out(dev):
    g = pg.golden()
    one = run([1], dev)
    five = run([0, 1, 2, 1, 0], dev)
    for out, B in ((one, 1), (five, 5)):
        assert isinstance(out["camera_opt"], Pinhole) and isinstance(out["gravity_opt"], Gravity)
        assert out["camera_opt"].shape == (B,) and out["gravity_opt"].shape == (B,)
        assert out["steps"].shape == out["converged"].shape == out["final_cost"].shape == (B,)
        assert out["steps"].dtype == torch.int32 and out["converged"].dtype == torch.bool and out["final_cost"].dtype == torch.float32
        assert torch.equal(out["camera_opt"].size, torch.tensor([[64.0, 48.0]], device=dev).expand(B, 2))
        lamb = 0.5
        total = (lamb * out["final_latitude_cost"].double() + (1 - lamb) * out["final_up_cost"].double()).float()
        assert torch.equal(total, out["final_cost"])
    assert torch.equal(five["rpv"][1], one["rpv"][0]) and torch.equal(five["rpv"][3], one["rpv"][0]) and torch.equal(five["rpv"][4], five["rpv"][0])
    # the objects carry the parameters: roll, pitch and vfov read back from them are the optimiser's to float32 rounding
    back = torch.stack([one["gravity_opt"].roll, one["gravity_opt"].pitch, one["camera_opt"].vfov], -1)
    assert (back - one["rpv"]).abs().max() < 2e-4       # (Gravity.roll's 1e-4 in its denominator)
    # cost_function: a (camera, gravity) pair or the numbers; the module's adds the total
    data = data_of([1], dev)
    mod = PerspectiveParamOpt({"lamb": 0.25})
    a, b = mod.cost_function(one["rpv"], data), mod.cost_function((one["camera_opt"], one["gravity_opt"]), data)
    assert sorted(a) == ["latitude", "latitude_grad", "total", "up", "up_grad"]
    assert torch.allclose(a["up"], b["up"], rtol=1e-2) and torch.allclose(a["latitude"], b["latitude"], rtol=1e-2)
    assert torch.equal(a["total"], (0.25 * a["latitude"].double() + 0.75 * a["up"].double()).float())
    # a start of the caller's: from the truth the optimiser stays within the same 0.3 degrees
    truth = torch.tensor(np.radians(g["poses"][1]), dtype=torch.float32, device=dev)[None]
    warm = PerspectiveParamOpt({})(data, init=truth)
    assert torch.equal(warm["initial"], truth) and (warm["rpv"] - truth).abs().max() < math.radians(0.3)
    # float64 and strided inputs are converted, not refused; wrong shapes are
    wide = PerspectiveParamOpt({"max_steps": 3})({k: v.double() for k, v in data.items()})
    assert torch.equal(wide["rpv"], PerspectiveParamOpt({"max_steps": 3})(data)["rpv"])
    with pytest.raises(ValueError):
        PerspectiveParamOpt({})({"up_field": data["up_field"][:, :1], "latitude_field": data["latitude_field"]})
    with pytest.raises(ValueError):
        perspective_opt.cost_function(one["rpv"].repeat(2, 1), data)
    with pytest.raises(RuntimeError, match="HIP device"):
        PerspectiveParamOpt({})({k: v.cpu() for k, v in data.items()})


# ------------------------------------------------------------------ 9. the pass at its branch edges and ragged tiles
# Every number below is held to param_opt_gate.gate's bound, MARGIN * D_k + MARGIN * 2^-23 * A_k, derived on the CPU from the
# float64 statement and its float32 restatement: nothing the device computes enters it.  test_param_opt_abi.py shows that
# every case is decisive and that the bound refuses each mutant of the pass by POWER x or more.
def planes_of(up, lat, dev, shift=0):
    """(B, 2, H, W) and (B, 1, H, W) arrays as device tensors that start `shift` floats past an aligned address."""
    out = {}
    for k, a in (("up_field", up), ("latitude_field", lat)):
        t = torch.from_numpy(np.array(a, np.float32))
        flat = torch.empty(t.numel() + shift, dtype=t.dtype, device=dev)
        assert flat.data_ptr() % 256 == 0
        flat[shift:].copy_(t.reshape(-1))
        out[k] = flat[shift:].view(t.shape)
    return out


def eight(states, data):
    """gclm_param_opt_cost: the (B, 8) float32 tensor [up, lat, up gradient, latitude gradient]."""
    rpv = torch.from_numpy(np.asarray(states, np.float32).reshape(-1, 3)).to(data["up_field"].device)
    out = perspective_opt.cost_function(rpv, data)
    torch.cuda.synchronize()
    return torch.cat([out["up"][:, None], out["latitude"][:, None], out["up_grad"], out["latitude_grad"]], 1)


def hold(tag, got, up, lat, state):
    """Prints, records and returns the ratio of each of the eight numbers to its bound (inf: not exactly 0 where the bound is 0)."""
    want, bound, _ = pg.gate(up, lat, state)
    got = np.asarray(got, np.float64)
    r = pg.ratios(got, want, bound)
    for k in range(8):
        print(f"{tag} number {k}: hip {got[k]:+.9e} f64 {want[k]:+.9e} err {abs(got[k] - want[k]):.2e} bound {bound[k]:.2e} ratio {r[k]:.3f}")
    MEASURED[f"param_opt_edges/{tag}"] = r.tolist()
    return r


@pytest.mark.parametrize("name", list(pg.RAGGED))
def test_ragged_tiles_against_float64(name, dev):
    """(a) The smallest shapes that reach a second tile column with idle lanes, a last tile row with idle waves, more tiles
    than the finish kernel has chains, and two and one pixels per lane natively: each number within its bound."""
    H, W, shift, px, tiles, _, _ = pg.RAGGED[name]
    up, lat, state = pg.ragged_case(name)
    data = planes_of(up[None], lat[None], dev, shift)
    assert pg.pixels_per_lane(W, data["up_field"].data_ptr(), data["latitude_field"].data_ptr()) == px       # the path under test
    assert pg.tile_count(H, W, px) == tiles
    r = hold(f"ragged/{name}", eight(state, data)[0].cpu().numpy(), up, lat, state)
    assert r.max() <= 1.0, r


@pytest.mark.parametrize("name", pg.EDGE_NAMES)
def test_branch_edges_against_float64(name, dev):
    """(b) tests/golden/param_opt_edges.npz: the latitude clamp, the clamp of |q|, both forms of the short-target branch, both
    angle clips (up gradients exactly 0 where every pixel is inside a clip), sign(0) and the extreme poses."""
    up, lat, state = pg.edge_case(name)
    got = eight(state, planes_of(up[None], lat[None], dev))[0].cpu().numpy()
    r = hold(f"edge/{name}", got, up, lat, state)
    assert r.max() <= 1.0, r
    if name in ("lower_clip", "upper_clip"):
        assert not got[2:5].any()


@pytest.mark.parametrize("name", ["B70 6x8", "B3 50x516"])
def test_batches_of_the_cost_entry_against_float64_and_each_image_alone(name, dev):
    """(c) gclm_param_opt_cost with B > 1 (B = 70: the pose kernel's second block): every image within its own bound and equal,
    bit for bit, to that image evaluated alone."""
    up, lat, states = pg.batch70() if name.startswith("B70") else pg.batch3()
    got = eight(states, planes_of(up, lat, dev))
    worst = np.zeros(8)
    for b in range(len(states)):
        alone = eight(states[b], planes_of(up[b:b + 1], lat[b:b + 1], dev))
        assert torch.equal(alone[0], got[b]), (b, alone[0], got[b])
        worst = np.maximum(worst, hold(f"batch/{name}/{b}", got[b].cpu().numpy(), up[b], lat[b], states[b]))
    print(f"{name}: worst ratio per number {worst.round(3).tolist()}")
    assert worst.max() <= 1.0, worst


@pytest.mark.parametrize("name", list(pg.RAGGED))
def test_loop_of_one_step_reports_the_bits_of_the_cost_entry(name, dev):
    """(d) gclm_param_opt with max_steps = 1 from an explicit init, three distinct images of a ragged shape: final_up_cost and
    final_latitude_cost are the bits gclm_param_opt_cost gives at that init (the same pass and sums; the loop reads the state
    32 words apart, the cost entry 3)."""
    H, W, shift, px, _, _, _ = pg.RAGGED[name]
    up, lat, states = pg.batch3(H, W)
    data = planes_of(up, lat, dev, shift)
    assert pg.pixels_per_lane(W, data["up_field"].data_ptr(), data["latitude_field"].data_ptr()) == px
    init = torch.from_numpy(states.astype(np.float32)).to(dev)
    cost = eight(states, data)
    out = PerspectiveParamOpt({"max_steps": 1})(data, init=init)
    torch.cuda.synchronize()
    print(name, "cost entry", cost[:, :2].tolist(), "loop", out["final_up_cost"].tolist(), out["final_latitude_cost"].tolist())
    assert out["steps"].tolist() == [1, 1, 1] and torch.equal(out["initial"], init)
    assert torch.equal(out["final_up_cost"], cost[:, 0]) and torch.equal(out["final_latitude_cost"], cost[:, 1])
    assert len({float(c) for c in cost[:, 0]}) == 3                              # distinct images: a wrong `b` would show


def test_initial_estimate_at_its_edges(dev):
    """(e) Rolls beyond +-90 degrees and of exactly 90 (the mirrored branch, g_y >= 0) and both ends of the vfov clamp, in one
    call: each parameter inside param_opt_gate.initial_interval."""
    fields = [pg.init_fields(pose) for pose in pg.INIT_EDGES]
    data = planes_of(np.stack([f[0] for f in fields]), np.stack([f[1] for f in fields]), dev)
    out = PerspectiveParamOpt({"max_steps": 1})(data)
    torch.cuda.synchronize()
    got = out["initial"].double().cpu().numpy()
    for b, pose in enumerate(pg.INIT_EDGES):
        lo, hi = pg.initial_interval(*fields[b])
        est = pg.initial_estimate(*fields[b])
        where = (got[b] - lo) / (hi - lo)
        print(f"pose {pose}: initial {np.degrees(got[b])} float64 {np.degrees(est)} position in the interval {where.round(3).tolist()}")
        MEASURED[f"param_opt_edges/initial/{pose}"] = where.tolist()
        assert (lo <= got[b]).all() and (got[b] <= hi).all(), (pose, got[b], lo, hi)
