"""Writes tests/golden/param_opt_edges.npz: tiny fields at the branch edges of the param_opt pass (gclm_param_opt.hip), the
states they are evaluated at and, per case, the eight numbers [up, lat, d up / d(r, p, v), d lat / d(r, p, v)] of the
reference's cost (siclib/models/optimization/perspective_opt.py) under float64 autograd at that state.  Data only.  The cases
(`names`; per case up_<name> (2, H, W), lat_<name> (1, H, W) float32, state_<name> (3,) float64 holding float32 numbers,
ref64_<name> (8,), nudges_<name>):

  zenith, nadir      8 x 12, vfov 60 degrees, roll 0, pitch +-atan(f / 2): sin(latitude) = +-1 at pixel (2, 6) / (6, 6), where the
                     latitude clamp is active and the predicted up vector has no direction.  Fields rendered 0.03 rad off in
                     pitch with sigma = 0.02 noise; the target up at that pixel and at one more is exactly (0, 0), a third is
                     (3e-9, -4e-9): both forms of the short-target branch
  zenith_q0          6 x 12, roll 0, pitch pi / 4, vfov 2 atan(3 / 2) (f = 2): the zenith on pixel (1, 6) again, chosen so that the
                     float32 pose record has b = -c and 1 / f = 0.5 exactly: q is exactly (0, 0) in the kernel's arithmetic
                     and its clamp of |q| at 1e-12 is taken (at the two cases above the float32 state leaves |q| near 1e-8)
  lower_clip         6 x 8, the state is the pose the fields were rendered at: all 48 up angles inside the lower clip; the
                     latitude target is offset by a +-0.01 checkerboard
  upper_clip         the same with the up target negated in columns 0 to 2: 18 pixels at pi - theta_clip
  exact_zero         6 x 8 at the state (0.3, 0, 60 degrees), whose predicted latitude at the principal point's pixel (3, 4) is
                     exactly 0 in either precision; the latitude target is the prediction +-0.01 and exactly 0 at that
                     pixel: the one pixel of the suite where sign(0) is taken
  roll80_vfov120, vfov20, pitch-60        extreme poses, noise-free, the state an offset from the pose (pitch -60 degrees at
                     33 x 47 is rendered at vfov 40 degrees, the nadir 8 degrees below the last row: with the nadir inside the
                     image float32 resolves the latitude of its nearest pixels to 6e-6 only, which no decisive case may hold)

Every case is made decisive (param_opt_gate.make_decisive: offending targets moved by 1e-3) before the reference sees it.  The
reference run in float64 clamps sin(latitude) at the double 1 - 1e-6; the tests pin param_opt_gate.cost_and_gradient to these
numbers with that bound (clamp_hi).  `finite_<name>` marks the numbers the reference returned finite: a number it did not is
held to the yardstick alone.  (At this writing every number of every case is finite: torch's norm, cosine_similarity and
l1_loss all take the zero subgradient at their kinks, as the kernel does.)

Runs where a checkout of the reference is available (oracle/ref_import.py says where); the tests that read the file need
none.

    python tests/golden/make_golden_param_opt_edges.py
"""
import importlib
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

import param_opt_gate as pg  # noqa: E402
from make_golden_param_opt import cost_and_gradient  # noqa: E402
from make_golden_rpf import reference_solver  # noqa: E402

CHECKER = 0.01


def checkerboard(H, W):
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.where((x + y) % 2 == 0, CHECKER, -CHECKER)


def pole(sign, seed, H=8, v=math.radians(60), rows=2):
    W = 12
    f = 0.5 * H / math.tan(0.5 * v)
    p = sign * math.atan(f / rows)
    state = pg.f32([0.0, p, v])
    up, lat = pg.render((0.0, p + 0.03, v), H, W, pg.NOISE, seed)
    row = H // 2 - rows if sign > 0 else H // 2 + rows
    up[:, row, 6] = 0.0                       # the pole's pixel: the predicted up has no direction there
    up[:, H - 1 - row, 3] = 0.0
    up[:, 4, 9] = (3e-9, -4e-9)
    return up, lat, state


def clip_case(negate):
    H, W = 6, 8
    state = pg.f32(np.radians([10.0, 20.0, 60.0]))
    up, lat = pg.render(state, H, W)
    lat = (lat.astype(np.float64) + checkerboard(H, W)).astype(np.float32)
    if negate:
        up[:, :, 0:3] *= -1
    return up, lat, state


def exact_zero():
    H, W = 6, 8
    state = pg.f32([0.3, 0.0, math.radians(60)])
    up, _ = pg.render(state + np.array(pg.OFFSET), H, W)
    _, lat = pg.render(state, H, W)
    lat = (lat.astype(np.float64) + checkerboard(H, W)).astype(np.float32)
    lat[0, 3, 4] = 0.0
    return up, lat, state


def extreme(H, W, fields_deg, state_deg):
    up, lat = pg.render(np.radians(np.array(fields_deg, np.float64)), H, W)
    return up, lat, pg.f32(np.radians(np.array(state_deg, np.float64)))


def cases():
    off = np.degrees(np.array(pg.OFFSET))
    return {"zenith": pole(+1, 11), "nadir": pole(-1, 12),
            "zenith_q0": pole(+1, 13, H=6, v=2 * math.atan(1.5)), "lower_clip": clip_case(False), "upper_clip": clip_case(True),
            "exact_zero": exact_zero(),
            "roll80_vfov120": extreme(8, 12, (80, 10, 118), (80 + off[0], 10 + off[1], 120)),
            "vfov20": extreme(8, 12, (5, 3, 20 + off[2]), (5 + off[0], 3 + off[1], 20)),
            "pitch-60": extreme(33, 47, (-10, -60, 40), np.array((-10, -60, 40)) + off)}


def main():
    reference_solver()
    po = importlib.import_module("siclib.models.optimization.perspective_opt")
    out = {"names": np.array(list(cases()))}
    for name, (up, lat, state) in cases().items():
        up, lat, nudges = pg.make_decisive(up, lat, state)
        ref, _ = cost_and_gradient(po, {"up_field": up[None], "latitude_field": lat[None]}, state, torch.float64)
        mine = pg.cost_and_gradient(up, lat, state, clamp_hi=pg.LAT_HI64)
        print(name, lat.shape[-2:], "nudges", nudges, "finite", np.isfinite(ref).tolist(), "\n  reference", ref, "\n  yardstick", mine, flush=True)
        out.update({f"up_{name}": up, f"lat_{name}": lat, f"state_{name}": state, f"ref64_{name}": ref,
                    f"finite_{name}": np.isfinite(ref), f"nudges_{name}": np.int32(nudges)})
    path = os.path.join(HERE, "param_opt_edges.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
