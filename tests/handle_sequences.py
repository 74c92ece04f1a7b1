"""The catalogue of call kinds behind tests/test_handle_reuse.py (no test in here, no GPU, no library).

By design the plan of a call depends on the call's arguments, the handle's configuration and its knobs, nothing else: a call on
a used gclm_handle must return the bits of the same call on a handle that has done nothing before.  A kind is one such call as
a plain record -- the gclm_config fields that differ from gclm_default_config, a value for EVERY knob the seven setters hold
(so a reused and a fresh handle never differ in one), the entry point, and seeded inputs (oracle.synth).  Shapes are the
smallest that reach the path a kind names.  RESULT kinds have outputs that are compared; DISTURBANCE kinds return nothing
that is compared -- what follows them is.
"""
import random
from dataclasses import dataclass, field

import numpy as np

MODELS = {"pinhole": 0, "simple_radial": 1, "radial": 2, "simple_divisional": 3}
SQUARED_LOSS_SCALE = float(2 ** 20)      # LMOptimizer._SQUARED_LOSS_SCALE: the Huber loss with an unreachable threshold

# the seven setters, in the order they are called, with the values of a handle that was never touched
KNOBS = {"sweep_iters": 0, "fused_steps": -1, "slat_plane": -1, "conf_pack": -1, "row_pairs": -1, "paced_launches": 0, "timing": 0}
SETTERS = tuple(f"gclm_set_{k}" for k in KNOBS)

# every configuration states these (the rest of gclm_config keeps gclm_default_config's value): five fixed steps
BASE_CFG = {"num_steps": 5, "early_stop": 0}


@dataclass(frozen=True)
class Kind:
    name: str
    entry: str                      # the C entry point ("split": begin, num_steps x (reduce, apply), finish; "abandoned": no finish)
    model: str = "pinhole"
    B: int = 3
    H: int = 16
    W: int = 64
    cfg: dict = field(default_factory=dict)       # gclm_config fields over BASE_CFG; None: the handle keeps what it has
    knobs: dict = field(default_factory=dict)     # over KNOBS
    planes: str = "all"             # "all" | "four" (no up confidence) | "latitude" (latitude and its confidence only)
    unaligned: bool = False         # every plane a view 4 bytes into its allocation
    sin_lat: bool = False           # d_sin_lat = torch.sin of the latitude handed over
    priors: tuple = ()              # of "scales", "prior_focal", "prior_gravity", "prior_dist"
    groups: int = 0                 # shared intrinsics: groups of B / groups frames (oracle.synth.make_shared_group)
    as_rpf: int = 0                 # gclm_system
    result: bool = True
    seed: int = 31

    def config(self):
        if self.cfg is None:
            return None
        return {**BASE_CFG, "camera_model": MODELS[self.model], **self.cfg}

    def all_knobs(self):
        return {**KNOBS, **self.knobs}


_TWO = {"fused_steps": 0}           # the two-launch sequence (a fixed-length solve this small takes one launch per step on its own)
_NO_GRAV = {"estimate_gravity": 0}
_SHARED = {"shared_intrinsics": 1, "group_size": 4}

CATALOGUE = (
    Kind("pinhole_b3", "gclm_calibrate", H=50, W=68, knobs={**_TWO, "sweep_iters": 2}),       # two chunks per image, the last ragged
    Kind("pinhole_b1_paced", "gclm_calibrate", B=1, cfg={"num_steps": 30, "early_stop": 1},
         knobs={"fused_steps": 1, "paced_launches": 3}),
    Kind("pinhole_cpack", "gclm_calibrate", H=50, W=68, knobs={**_TWO, "conf_pack": 1}),
    Kind("pinhole_lat_scalar", "gclm_calibrate", B=2, H=8, W=18, planes="latitude"),           # W % 4 != 0
    Kind("sr_slat", "gclm_calibrate", model="simple_radial", H=48, W=64, knobs={**_TWO, "slat_plane": 1, "timing": 1}),
    Kind("sr_unaligned", "gclm_calibrate", model="simple_radial", B=2, unaligned=True),
    Kind("sr_four", "gclm_calibrate", model="simple_radial", H=50, W=68, planes="four"),
    Kind("abandoned_session", "abandoned", model="simple_radial", B=8, groups=2, cfg=dict(_SHARED), result=False),
    Kind("sr_sinlat", "gclm_calibrate_ex", model="simple_radial", H=48, W=64, sin_lat=True, knobs=_TWO),
    Kind("sr_strips", "gclm_calibrate", model="simple_radial", B=2, H=8, W=2600),              # W > 2048: strips
    Kind("radial_pairs", "gclm_calibrate", model="radial", B=4, H=48, W=64, knobs={**_TWO, "row_pairs": 1}),
    Kind("radial_b66", "gclm_calibrate", model="radial", B=66, H=6, W=8, knobs=_TWO),           # growth; two blocks of the per-image kernels
    Kind("div_wide", "gclm_calibrate", model="simple_divisional", B=2, H=6, W=640),
    Kind("prior_focal", "gclm_calibrate", model="simple_radial", cfg={"estimate_focal": 0}, priors=("prior_focal",)),
    Kind("prior_gravity", "gclm_calibrate", model="simple_radial", cfg=_NO_GRAV, priors=("prior_gravity",)),
    Kind("prior_dist", "gclm_calibrate", model="simple_radial", cfg={"estimate_dist": 0}, priors=("prior_dist",)),
    Kind("scales", "gclm_calibrate", model="simple_radial", priors=("scales",)),
    Kind("training", "gclm_calibrate", cfg={"compute_uncertainty": 0, "heuristic_init": 1, "up_loss_fn_scale": SQUARED_LOSS_SCALE,
                                            "lat_loss_fn_scale": SQUARED_LOSS_SCALE}),
    Kind("release", "gclm_release_workspace", cfg=None, result=False),
    Kind("linear_focal_fixlambda", "gclm_calibrate", model="radial", cfg={"use_log_focal": 0, "fix_lambda": 1}),
    Kind("zero_images", "gclm_solve", B=0, result=False),
    Kind("solve_offcentre", "gclm_solve_ex", model="radial", knobs={**_TWO, "row_pairs": 1}),
    Kind("early_b5", "gclm_calibrate", model="radial", B=5, cfg={"num_steps": 30, "early_stop": 1, "atol": 1e-5, "rtol": 1e-5},
         knobs=_TWO),
    Kind("recorded", "gclm_calibrate_recorded"),
    Kind("system_loop", "gclm_system", model="radial", as_rpf=0),
    Kind("system_rpf", "gclm_system", model="radial", as_rpf=1),
    Kind("shared_full", "gclm_calibrate", B=8, groups=2, cfg=dict(_SHARED)),
    Kind("shared_split", "split", model="simple_radial", B=8, groups=2, cfg=dict(_SHARED)),
)
BY_NAME = {k.name: k for k in CATALOGUE}
RESULT_KINDS = tuple(k for k in CATALOGUE if k.result)
DISTURBANCE_KINDS = tuple(k for k in CATALOGUE if not k.result)
# all ordered pairs (A, B), A != B, B a result kind: A a result kind leaves 24 successors, a disturbance 25
N_PAIRS = len(RESULT_KINDS) * (len(RESULT_KINDS) - 1) + len(DISTURBANCE_KINDS) * len(RESULT_KINDS)


def inputs(kind: Kind) -> dict:
    """The host arrays of a kind's call (float32 / int32 numpy), a function of the kind alone: the field planes by their data
    keys, `sin_latitude`, the priors, `cam` / `grav` where the entry takes an explicit state, `group_of_frame`."""
    import torch
    from oracle import synth
    if kind.B == 0 or kind.entry == "gclm_release_workspace":
        return {}
    if kind.groups:
        frames = kind.B // kind.groups
        parts = [synth.make_shared_group(kind.seed, g, kind.model, kind.H, kind.W, frames=frames) for g in range(kind.groups)]
        data = {k: np.concatenate([p[0][k] for p in parts]) for k in parts[0][0]}
        gt_cam, gt_grav = (np.concatenate([p[j] for p in parts]) for j in (1, 2))
    else:
        data, gt_cam, gt_grav = synth.make_fields(kind.seed, range(kind.B), kind.model, kind.H, kind.W)
    if kind.planes == "four":
        data.pop("up_confidence")
    elif kind.planes == "latitude":
        data = {k: data[k] for k in ("latitude_field", "latitude_confidence")}
    if kind.sin_lat:
        data["sin_latitude"] = torch.sin(torch.from_numpy(data["latitude_field"])).numpy()
    for p in kind.priors:
        data[p] = {"scales": np.float32([1.25, 0.8]), "prior_focal": gt_cam[:, 3] * np.float32(1.1),
                   "prior_gravity": gt_grav, "prior_dist": gt_cam[:, 6:7] * np.float32(0.5)}[p].copy()
    # the trivial estimate with gravity straight down (lm_optimizer.py:20-58), the principal point where the kind wants it
    f = np.float32(0.7 * max(kind.H, kind.W))
    off = np.float32([1.5, -0.75]) if kind.name == "solve_offcentre" else np.float32([0, 0])
    trivial = np.tile(np.float32([kind.W, kind.H, f, f, kind.W / 2 + off[0], kind.H / 2 + off[1], 0, 0]), (kind.B, 1))
    down = np.tile(np.float32([0, -1, 0]), (kind.B, 1))
    if kind.entry == "gclm_system":                  # the system at the ground truth: every column of the model is live
        data["cam"], data["grav"] = gt_cam.copy(), gt_grav.copy()
    elif kind.entry in ("gclm_solve_ex", "split", "abandoned"):
        data["cam"], data["grav"] = trivial, down
    if kind.entry in ("split", "abandoned"):
        data["group_of_frame"] = (np.arange(kind.B) // (kind.B // kind.groups)).astype(np.int32)
    return {k: np.ascontiguousarray(v) for k, v in data.items()}


def sequences():
    """The orders test_long_sequences walks, each on one handle: the catalogue as listed, reversed, and six seeded
    permutations.  The seeds are fixed, so the orders are; tests/test_handle_reuse_host.py checks on the CPU that each order can
    show what the GPU test asserts of it (sequence_shows)."""
    names = [k.name for k in CATALOGUE]
    out = {"listed": list(names), "reversed": list(reversed(names))}
    for seed in PERMUTATION_SEEDS:
        out[f"seed{seed}"] = random.Random(seed).sample(names, len(names))
    return out


PERMUTATION_SEEDS = (2, 3, 4, 6, 7, 8)      # (1 and 5 give orders that release the planes before a call could show them kept)


def sequence_shows(order) -> dict:
    """What an order is able to show, from the order alone: a workspace that is given back and allocated again (`release`
    with a call on either side), a scratch plane and a packed plane still held when a call that must not use them runs, and a
    call after the abandoned session."""
    i = {n: order.index(n) for n in order}
    allocates = lambda n: BY_NAME[n].B > 0 and n != "release"      # noqa: E731

    def follows_before_release(name, wanted):
        after = order[i[name] + 1:]
        upto = after[:after.index("release")] if "release" in after else after
        return any(wanted(BY_NAME[n]) for n in upto)

    return {"regrowth": any(map(allocates, order[:i["release"]])) and any(map(allocates, order[i["release"] + 1:])),
            # (no pinhole kind of the catalogue asks for the plane of sin(latitude), and only pinhole_cpack packs)
            "kept_slat_plane": follows_before_release("sr_slat", lambda k: k.result and k.model == "pinhole"),
            "kept_conf_pack": follows_before_release("pinhole_cpack", lambda k: k.result),
            "call_after_abandoned": i["abandoned_session"] < len(order) - 1}
