"""CPU: the host-side logic of bench.py that does not need a device.

(1) without a HIP device `bench.py` (and `bench.py --gpus N`, which would start its own ranks) answers with ONE JSON line
    carrying `error` and a non-zero exit code -- never a traceback, never a CPU fallback of the product path;
(2) `cpu_baseline()` has two branches: the reference's own PyTorch path timed on THIS box when the checkout is there
    ($GEOCALIB_REFERENCE / /root/reference: the build container; a stub checkout here), otherwise the C port alone with
    `reference_on_this_box: false`.  Both keep the keys the driver parses (value, unit, cores, kind);
(3) `dump_outputs()` (--dump-outputs DIR) writes the timed path's result as .npy files, sampled beyond its size cap;
(4) `--full` is off by default: a plain run measures the headline only."""
import json
import os
import subprocess
import sys
import types

import pytest
import torch

from conftest import ROOT


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


@pytest.mark.parametrize("extra", [[], ["--gpus", "2"], ["--gpus", "8", "--shared-group", "16"]])
def test_without_a_device_bench_prints_one_error_line(extra):
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, capture_output=True, text=True, timeout=300,
                         cwd=ROOT, env=env)
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert res.returncode == 2 and len(lines) == 1, (res.returncode, res.stdout, res.stderr[-1000:])
    out = json.loads(lines[0])
    assert out["value"] is None and "no HIP device" in out["error"]
    assert out["n_gpus"] == (int(extra[1]) if extra else 1) and out["unit"] == "images/sec"
    assert "Traceback" not in res.stderr


def _sample(n, H=48, W=64, model="pinhole"):
    from oracle import synth
    data, _, _ = synth.make_fields(11, range(n), model, H, W)
    return data


def _args(model="pinhole", H=48, W=64, steps=5):
    return types.SimpleNamespace(camera_model=model, lm_steps=steps, height=H, width=W)


def test_cpu_baseline_without_the_reference_is_the_port(monkeypatch):
    bench = _bench()
    from oracle import ref_import
    monkeypatch.setattr(ref_import, "REFERENCE_ROOT", "/nonexistent/reference")
    assert not ref_import.available()
    out = bench.cpu_baseline(_args(), 4, _sample(4))
    assert out["kind"] == "port" and out["reference_on_this_box"] is False
    assert out["value"] > 0 and out["unit"] == "images/sec" and 1 <= out["cores"] <= 4
    assert "port" not in out and "oracle/lm_oracle.c" in out["sample"]
    # the committed build-container timing of the reference is attached only for the shape it was measured at
    assert "reference_torch" not in out
    full = bench.reference_torch(types.SimpleNamespace(camera_model="pinhole", lm_steps=20, height=480, width=640))
    assert full is None or (full["kind"] == "reference" and "build container" in full["measured_on"])


STUB_LM_OPTIMIZER = '''
import torch

CALLS = []


class LMOptimizer(torch.nn.Module):
    """Stands in for the reference's LMOptimizer: records how it is driven, returns the shapes a caller reads."""

    def __init__(self, conf):
        super().__init__()
        self.conf = dict(conf)

    def forward(self, data):
        n = data["latitude_field"].shape[0]
        CALLS.append({"conf": self.conf, "training": self.training, "grad": torch.is_grad_enabled(), "images": n,
                      "threads": torch.get_num_threads(), "keys": sorted(data)})
        return {"camera": torch.zeros(n, 8), "gravity": torch.zeros(n, 3)}
'''


def test_cpu_baseline_times_the_reference_where_it_exists(monkeypatch, tmp_path):
    """A checkout at $GEOCALIB_REFERENCE (here a stub package with the modules ref_import loads): its LMOptimizer is timed
    as the baseline of record, in eval mode without autograd, on the host's granted cores, after a one-image warm-up,
    with the port beside it."""
    pkg = tmp_path / "geocalib"
    pkg.mkdir()
    for name in ("__init__", "perspective_fields", "camera", "gravity", "misc", "utils"):
        (pkg / f"{name}.py").write_text("")
    (pkg / "lm_optimizer.py").write_text(STUB_LM_OPTIMIZER)
    bench = _bench()
    from oracle import lm_oracle, ref_import
    real_root = ref_import.REFERENCE_ROOT
    monkeypatch.setattr(ref_import, "REFERENCE_ROOT", str(tmp_path))
    monkeypatch.setattr(sys, "path", [q for q in sys.path if q != real_root])     # (ref_import.load prepends the stub's root)
    assert ref_import.available()
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "geocalib" or k.startswith("geocalib.")}
    threads = torch.get_num_threads()
    try:
        out = bench.cpu_baseline(_args(), 3, _sample(3))
        calls = sys.modules["geocalib.lm_optimizer"].CALLS
    finally:
        for k in [k for k in sys.modules if k == "geocalib" or k.startswith("geocalib.")]:
            del sys.modules[k]
        sys.modules.update(saved)
    assert out["kind"] == "reference" and out["measured_on"] == "this box" and out["reference_on_this_box"] is True
    assert out["value"] > 0 and out["unit"] == "images/sec" and out["cores"] >= 1
    assert "lm_optimizer.py:141" in out["code"] and "the first 3 images" in out["sample"]
    assert out["port"]["kind"] == "port" and out["port"]["value"] > 0
    # one-image warm-up, then the timed call on the whole sample; the conf of the line, eval mode, no autograd, all cores
    assert [c["images"] for c in calls] == [1, 3]
    cores = lm_oracle.effective_cpus()
    for c in calls:
        assert c["conf"] == {"camera_model": "pinhole", "num_steps": 5, "early_stop": False, "shared_intrinsics": False}
        assert c["training"] is False and c["grad"] is False and c["threads"] == cores
        assert c["keys"] == ["latitude_confidence", "latitude_field", "up_confidence", "up_field"]
    # the thread count of the process is restored
    assert torch.get_num_threads() == threads


def test_cpu_baseline_survives_a_broken_reference_checkout(monkeypatch, tmp_path):
    """A directory that looks like a checkout but does not import: the baseline falls back to the port and says why."""
    (tmp_path / "geocalib").mkdir()
    bench = _bench()
    from oracle import ref_import
    real_root = ref_import.REFERENCE_ROOT
    monkeypatch.setattr(ref_import, "REFERENCE_ROOT", str(tmp_path))
    monkeypatch.setattr(sys, "path", [q for q in sys.path if q != real_root])     # (an earlier test may have imported the real one)
    assert ref_import.available()
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "geocalib" or k.startswith("geocalib.")}
    try:
        out = bench.cpu_baseline(_args(), 2, _sample(2))
    finally:
        for k in [k for k in sys.modules if k == "geocalib" or k.startswith("geocalib.")]:
            del sys.modules[k]
        sys.modules.update(saved)
    assert out["kind"] == "port" and out["reference_on_this_box"] is False and "reference_error" in out


def test_vs_oracle_record_and_the_kept_oracle_result(monkeypatch):
    """`check.vs_oracle`: cpu_baseline hands the oracle's solve of the sample back (`keep`), vs_oracle turns
    it and the HIP rows into the record of the bench line -- distances next to the 1e-4 gate; a NaN is never inside a gate;
    shared-intrinsics samples are solved group by group like the reference does."""
    import numpy as np
    bench = _bench()
    from oracle import ref_import
    monkeypatch.setattr(ref_import, "REFERENCE_ROOT", "/nonexistent/reference")
    data = _sample(6)
    kept = {}
    out = bench.cpu_baseline(_args(), 6, data, keep=kept)
    assert out["kind"] == "port" and set(kept) == {"camera", "gravity", "final_cost"}
    assert kept["camera"].shape == (6, 8) and kept["gravity"].shape == (6, 3) and kept["final_cost"].shape == (6,)
    same = bench.vs_oracle({k: v.copy() for k, v in kept.items()}, kept, "itself")
    assert same["within_gate"] is True and same["images"] == 6 and same["gate"] == 1e-4
    assert same["max_focal_rel"] == same["max_gravity_abs"] == same["max_final_cost_rel"] == 0.0
    off = {k: v.copy() for k, v in kept.items()}
    off["camera"][2, 3] *= 1 + 3e-4
    rec = bench.vs_oracle(off, kept, "a focal 3e-4 off")
    assert rec["within_gate"] is False and 2.9e-4 < rec["max_focal_rel"] < 3.1e-4 and "a focal 3e-4 off" in rec["against"]
    nan = {k: v.copy() for k, v in kept.items()}
    nan["gravity"][0, 0] = np.nan
    assert bench.vs_oracle(nan, kept, "nan")["within_gate"] is False
    # more HIP rows than oracle rows: only the sample is compared
    more = {k: np.concatenate([v, v]) for k, v in kept.items()}
    assert bench.vs_oracle(more, kept, "prefix")["images"] == 6
    # shared intrinsics: one oracle call per group of `group` frames (lm_optimizer.py:350-383), concatenated in order
    args = _args()
    args.shared_group = 3
    kept_g = {}
    out_g = bench.cpu_baseline(args, 6, data, keep=kept_g)
    assert out_g["unit"] == "frames/sec" and "2 shared-intrinsics groups of 3" in out_g["sample"]
    assert kept_g["camera"].shape == (6, 8)
    for lo in (0, 3):
        assert np.ptp(kept_g["camera"][lo:lo + 3, 3]) == 0            # one focal per group ...
    assert kept_g["camera"][0, 3] != kept_g["camera"][3, 3]          # ... and not the same for both
    direct = bench.oracle_solve("pinhole", 5, {k: v[:3] for k, v in data.items()}, 3, 2)
    assert np.array_equal(direct["camera"], kept_g["camera"][:3])


def test_dump_outputs_writes_what_the_caller_receives(tmp_path):
    """--dump-outputs: every tensor of the result dict as DIR/<name>.npy (the camera / gravity records of the wrappers),
    float32 kept, other dtypes as float64; beyond the size cap one seeded sample of images, the same for every output."""
    import numpy as np
    bench = _bench()
    n = 40
    rec = types.SimpleNamespace
    out = {"camera": rec(_data=torch.arange(n * 8, dtype=torch.float32).reshape(n, 8)),
           "gravity": rec(_data=torch.arange(n * 3, dtype=torch.float32).reshape(n, 3)),
           "covariance": torch.arange(n * 9, dtype=torch.float32).reshape(n, 3, 3),
           "final_cost": torch.linspace(0, 1, n, dtype=torch.float64), "stop_at": torch.full((n,), 7, dtype=torch.int32),
           "note": "not an array"}
    info = bench.dump_outputs(out, str(tmp_path / "all"))
    assert info["images"] == n and info["sampled_images"] is None and info["arrays"] == sorted(k for k in out if k != "note")
    got = {k: np.load(tmp_path / "all" / f"{k}.npy") for k in info["arrays"]}
    assert sorted(os.listdir(tmp_path / "all")) == sorted(f"{k}.npy" for k in info["arrays"])
    assert got["camera"].dtype == np.float32 and np.array_equal(got["camera"], out["camera"]._data.numpy())
    assert got["covariance"].shape == (n, 3, 3) and got["final_cost"].dtype == np.float64
    assert got["stop_at"].dtype == np.float64 and (got["stop_at"] == 7).all()
    assert info["bytes"] == sum(a.nbytes for a in got.values())
    # a cap of ~half the bytes: the same images of every output, named by dump_rows, within the cap, the same on every call
    cap = info["bytes"] // 2
    small = bench.dump_outputs(out, str(tmp_path / "s1"), max_bytes=cap)
    again = bench.dump_outputs(out, str(tmp_path / "s2"), max_bytes=cap)
    assert 0 < small["sampled_images"] < n and small["bytes"] <= cap and small == {**again, "dir": small["dir"]}
    rows = np.load(tmp_path / "s1" / "dump_rows.npy").astype(np.int64)
    assert np.array_equal(rows, np.load(tmp_path / "s2" / "dump_rows.npy")) and np.all(np.diff(rows) > 0)
    for k in info["arrays"]:
        assert np.array_equal(np.load(tmp_path / "s1" / f"{k}.npy"), got[k][rows]), k


def test_full_is_off_by_default(monkeypatch):
    """A plain `bench.py --gpus 1 --steps N --warmup W` measures the headline only; --full adds the records that take runs
    of their own (read ceiling, CPU baseline and oracle check, secondary, overlap, best of n allocations, N > 1 parity)."""
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    plain = bench.parse()
    assert plain.full is False and (plain.gpus, plain.steps, plain.warmup) == (1, 20, 5)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    full = bench.parse()
    assert full.full is True and vars(full) == {**vars(plain), "full": True}
