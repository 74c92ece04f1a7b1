"""CPU: the packed confidence format of the pinhole solve (gclm_device.h: conf_encode / conf_decode / conf_word;
include/gclm.h: gclm_set_conf_pack), restated in numpy, and what rounding the confidences to it does to a solve.

The format: q = rint(c * 65535) on float32 (round half to even), word = q_up | q_lat << 16, c' = float32(q) * float32(1 / 65535).
tests/test_conf_pack.py (-m gpu) holds the HIP solve to these functions bit for bit; here they are pinned against
themselves, and the float32 oracle solves 64 images of 48x64 with c and with c': focal (relative), gravity (absolute) and
final cost (relative) must agree within BUDGET = 1e-5, a tenth of the project's 1e-4 end-of-solve gate (measured: 5.4e-7 /
1.3e-7 / 4.8e-7; the oracle's own float32-vs-float64 spread on the same fields is 4.8e-7 / 2.0e-7 / 1.8e-7)."""
import os

import numpy as np
import pytest

import test_kernel_audit as audit

SCALE = np.float32(65535)
STEP = np.float32(1) / np.float32(65535)
BUDGET = 1e-5


def encode(c):
    """q of a float32 confidence in [0, 1]."""
    c = np.asarray(c, np.float32)
    assert ((c >= 0) & (c <= 1)).all()
    return np.rint(c * SCALE).astype(np.uint32)


def decode(q):
    return np.asarray(q, np.uint32).astype(np.float32) * STEP


def word(q_up, q_lat):
    return np.asarray(q_up, np.uint32) | (np.asarray(q_lat, np.uint32) << np.uint32(16))


def unword(w):
    w = np.asarray(w, np.uint32)
    return w & np.uint32(0xFFFF), w >> np.uint32(16)


def roundtrip(c):
    return decode(encode(c))


def test_every_code_survives_the_round_trip():
    q = np.arange(65536, dtype=np.uint32)
    c = decode(q)
    assert c.dtype == np.float32 and c[0] == 0 and c[-1] == 1 and (np.diff(c) > 0).all()
    assert np.array_equal(encode(c), q)
    assert np.array_equal(roundtrip(c).view(np.uint32), c.view(np.uint32))
    # both halves of a word are independent
    a, b = np.meshgrid(q[::257], q[::255])
    ua, ub = unword(word(a, b))
    assert np.array_equal(ua, a) and np.array_equal(ub, b)


def test_rounding_is_to_nearest_even_within_half_a_step():
    rng = np.random.default_rng(5)
    c = rng.random(1 << 16, dtype=np.float32)
    r = roundtrip(c)
    assert np.abs(r.astype(np.float64) - c).max() <= 0.5 / 65535 + 2.0 ** -24
    assert np.array_equal(roundtrip(r).view(np.uint32), r.view(np.uint32))          # idempotent
    # exact halves go to the even code: (q + 0.5) / 65535 is not a float32 in general, so take the product's own ties
    ties = (np.arange(0, 64, dtype=np.float32) + np.float32(0.5))                   # c * 65535 == k + 0.5 exactly
    assert np.array_equal(np.rint(ties).astype(np.uint32) % 2, np.zeros(64, np.uint32))
    assert encode(np.float32(0)) == 0 and encode(np.float32(1)) == 65535 and encode(np.float32(-0.0)) == 0


def test_rounded_confidences_move_the_solve_by_float32_rounding(oracle):
    from oracle import synth
    n, H, W = 64, 48, 64
    data = synth.make_fields(7, range(n), "pinhole", H, W)[0]
    conf = {"camera_model": "pinhole", "num_steps": 20, "early_stop": False}
    rounded = dict(data)
    for k in ("up_confidence", "latitude_confidence"):
        rounded[k] = roundtrip(data[k])
        assert not np.array_equal(rounded[k], data[k])
    a = oracle.solve(data, conf, precision="f32")
    b = oracle.solve(rounded, conf, precision="f32")
    focal = np.abs(b["camera"][:, 2:4] / a["camera"][:, 2:4] - 1).max()
    gravity = np.abs(b["gravity"] - a["gravity"]).max()
    cost = np.abs(b["final_cost"] / a["final_cost"] - 1).max()
    print(f"conf_pack rounding, {n} images of {H}x{W}: focal {focal:.2e} gravity {gravity:.2e} final cost {cost:.2e}")
    assert focal <= BUDGET and gravity <= BUDGET and cost <= BUDGET, (focal, gravity, cost)


@pytest.mark.skipif(not (os.path.exists(audit.SO) and os.path.exists(f"{audit.LLVM}/llvm-readelf")), reason="library or LLVM tools missing")
def test_the_packed_sweeps_are_four_kernels_without_scratch(tmp_path):
    """conf_pack_sweep_kernel<LOGF, CPACK>: the fill and the reader in both focal forms, the 4-wave reduction buffer(s) as their
    only LDS (the reader holds two bodies: the packed one and the five-plane one of a flagged image), at most 96 VGPRs (five
    waves per SIMD: the reader's launches keep five workgroups per CU), and no scratch in the log-focal form every loop sweep of
    the default conf runs."""
    k = {n: v for n, v in audit.kernel_metadata(tmp_path).items() if "conf_pack_sweep_kernelI" in n}
    assert len(k) == 4, sorted(k)
    for n, v in k.items():
        assert v["lds"] <= 512 and v["vgpr"] <= 96, (n, v)
        if "ILb1E" in n:
            assert v["scratch"] == 0, (n, v)
