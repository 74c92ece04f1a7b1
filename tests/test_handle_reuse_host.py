"""CPU: how LMOptimizer keeps and reconfigures its gclm_handles, with the library replaced by the recorder of
tests/test_host_calls.py -- and the catalogue of tests/handle_sequences.py, as far as it can be checked without a GPU.

A stale configuration on a kept handle is impossible only if `_config_signature` covers everything `_config` reads: the
handle is reconfigured when the signature changes, and only then."""
import ctypes as C

import pytest
import torch

import handle_sequences as hs
from geocalib_amd import _lib
from geocalib_amd.lm_optimizer import LMOptimizer
from test_host_calls import rec  # noqa: F401  (the fixture)

DEV = torch.device("cuda", 0)


def _set(key, value):
    return lambda opt: setattr(opt.conf, key, value)


# (what a caller changes, the gclm_config fields it reaches)
MUTATIONS = {
    "set_camera_model": (lambda o: o.set_camera_model("radial"), {"camera_model"}),
    "shared_intrinsics": (lambda o: setattr(o, "shared_intrinsics", True), {"shared_intrinsics"}),     # as GeoCalib.calibrate sets it
    "group_size": (_set("group_size", 4), {"group_size"}),
    "num_steps": (lambda o: setattr(o, "num_steps", 7), {"num_steps"}),
    "lambda_": (_set("lambda_", 0.5), {"lambda0"}),
    "fix_lambda": (_set("fix_lambda", True), {"fix_lambda"}),
    "early_stop": (_set("early_stop", False), {"early_stop"}),
    "atol": (_set("atol", 1e-6), {"atol"}),
    "rtol": (_set("rtol", 1e-6), {"rtol"}),
    "use_spherical_manifold": (_set("use_spherical_manifold", False), {"use_spherical_manifold"}),
    "use_log_focal": (_set("use_log_focal", False), {"use_log_focal"}),
    "up_loss_fn_scale": (_set("up_loss_fn_scale", 0.5), {"up_loss_fn_scale"}),
    "lat_loss_fn_scale": (_set("lat_loss_fn_scale", 0.5), {"lat_loss_fn_scale"}),
    "loss_fn": (_set("loss_fn", "squared_loss"), {"up_loss_fn_scale", "lat_loss_fn_scale"}),
    "init_conf": (_set("init_conf", {"name": "heuristic"}), {"heuristic_init"}),
    "prior_gravity": (lambda o: o.setup_optimization_and_priors({"prior_gravity": 0}), {"estimate_gravity"}),
    "prior_focal": (lambda o: o.setup_optimization_and_priors({"prior_focal": 0}), {"estimate_focal"}),
    "prior_dist": (lambda o: o.setup_optimization_and_priors({"prior_dist": 0}), {"estimate_dist"}),
    "train": (lambda o: o.train(), {"compute_uncertainty"}),
    # read by neither
    "verbose": (_set("verbose", True), set()),
    "loss_weight": (_set("loss_weight", 2.0), set()),
    "paced_launches": (lambda o: setattr(o, "paced_launches", 3), set()),
}


def _optimizer():
    return LMOptimizer({"camera_model": "simple_radial"}).eval()


def _fields_of(cfg):
    return {f: getattr(cfg, f) for f, _ in cfg._fields_}


@pytest.mark.parametrize("what", list(MUTATIONS))
def test_the_signature_changes_exactly_when_the_configuration_does(rec, what):
    mutate, reaches = MUTATIONS[what]
    opt = _optimizer()
    sig0, cfg0 = opt._config_signature(0), _fields_of(opt._config(0))
    mutate(opt)
    sig1, cfg1 = opt._config_signature(0), _fields_of(opt._config(0))
    assert {f for f in cfg0 if cfg0[f] != cfg1[f]} == reaches
    assert (sig1 != sig0) == bool(reaches)


def test_the_mutations_reach_every_field_config_fills(rec):
    opt = _optimizer()
    assert opt._config_signature(0) != opt._config_signature(1) and opt._config(0).key() != opt._config(1).key()
    reached = set().union(*(r for _, r in MUTATIONS.values())) | {"device"}
    # (struct_size and abi_version are the library's stamp, set by gclm_default_config)
    assert reached == {f for f, _ in _lib.GclmConfig._fields_} - {"struct_size", "abi_version"}


def test_a_finer_signature_costs_one_comparison_and_no_call(rec):
    """init_conf ransac is the trivial estimate to the library (the RANSAC estimate is handed to gclm_solve): the signature
    changes, the configuration does not, and the handle is not configured again."""
    opt = _optimizer()
    h = opt._handle(DEV, 5)
    del rec.calls[:]
    key = opt._config(0).key()
    opt.conf.init_conf = {"name": "ransac"}
    assert opt._config(0).key() == key
    assert opt._handle(DEV, 5) is h
    assert [n for n, _ in rec.calls if n in ("gclm_configure", "gclm_create")] == []


def test_a_kept_handle_is_configured_once_per_change(rec):
    opt = _optimizer()
    h = opt._handle(DEV, 5)
    assert [n for n, _ in rec.calls].count("gclm_create") == 1
    del rec.calls[:]
    for _ in range(3):                                           # the serving loop's common case
        assert opt._handle(DEV, 5) is h
    assert [n for n, _ in rec.calls if n.startswith("gclm_c")] == []
    opt.set_camera_model("radial")
    opt.setup_optimization_and_priors({"prior_focal": 0})
    opt.train()
    del rec.calls[:]
    assert opt._handle(DEV, 5) is h and opt._handle(DEV, 5) is h
    calls = [(n, a) for n, a in rec.calls if n in ("gclm_configure", "gclm_create")]
    assert [n for n, _ in calls] == ["gclm_configure"]
    handle, struct = calls[0][1]
    assert handle is h.ptr
    want = opt._config(0)
    assert struct._obj.key() == want.key() == h.key
    assert (want.camera_model, want.estimate_focal, want.compute_uncertainty) == (2, 0, 0)
    assert len(opt._handles) == 1


def test_the_seventeenth_key_destroys_the_least_recently_used_handle(rec, monkeypatch):
    created = []

    def create(out, cfg):
        created.append(0x1000 * (len(created) + 1))
        out._obj.value = created[-1]
        rec.calls.append(("gclm_create", (created[-1],)))
        return 0

    rec.gclm_create = create
    monkeypatch.setattr(torch.cuda, "synchronize", lambda device=None: rec.calls.append(("synchronize", (device,))))
    opt = _optimizer()
    assert opt._MAX_HANDLES == 16
    device_of = lambda stream: torch.device("cuda", stream % 2)      # noqa: E731
    try:
        handles = {s: opt._handle(device_of(s), s) for s in range(1, 17)}
        assert len(opt._handles) == 16 and len(created) == 16
        assert opt._handle(device_of(1), 1) is handles[1]           # used again: stream 2 is now the least recently used
        victim = handles[2].ptr.value
        del rec.calls[:]
        opt._handle(device_of(17), 17)
        names = [n for n, _ in rec.calls]
        assert names.count("gclm_create") == 1 and names.count("gclm_destroy") == 1 and names.count("synchronize") == 1
        # its own device is synchronised first (the workspace may still be in flight), then it is destroyed, then the new one built
        order = [c for c in rec.calls if c[0] in ("synchronize", "gclm_destroy", "gclm_create")]
        assert order[0] == ("synchronize", (device_of(2),))
        assert order[1][0] == "gclm_destroy" and order[1][1][0].value == victim
        assert order[2][0] == "gclm_create"
        assert not handles[2].ptr and (0, 2) not in opt._handles and len(opt._handles) == 16
        del rec.calls[:]
        third = handles[3].ptr.value
        again = opt._handle(device_of(2), 2)                        # a return to that key builds a new one, in stream 3's place
        assert again is not handles[2] and again.ptr.value == created[-1] and len(created) == 18
        assert [n for n, _ in rec.calls if n == "gclm_create"] == ["gclm_create"]
        assert [c[1][0].value for c in rec.calls if c[0] == "gclm_destroy"] == [third]
    finally:
        for h in opt._handles.values():                             # the pointers are made up: nothing may destroy them later
            h.ptr = C.c_void_p()


# ------------------------------------------------------------------ the catalogue of tests/test_handle_reuse.py

def test_the_catalogue_is_complete():
    assert len(hs.RESULT_KINDS) == 25 and len(hs.DISTURBANCE_KINDS) == 3 and hs.N_PAIRS == 675
    assert len({k.name for k in hs.CATALOGUE}) == len(hs.CATALOGUE)
    for k in hs.CATALOGUE:                                          # every kind states every knob, and only those
        assert set(k.all_knobs()) == set(hs.KNOBS) and list(k.all_knobs()) == list(hs.KNOBS), k.name
        assert k.cfg is None or set(k.config()) <= {f for f, _ in _lib.GclmConfig._fields_}, k.name
    assert hs.SETTERS == ("gclm_set_sweep_iters", "gclm_set_fused_steps", "gclm_set_slat_plane", "gclm_set_conf_pack",
                          "gclm_set_row_pairs", "gclm_set_paced_launches", "gclm_set_timing")
    assert all(hasattr(_lib, "_SIGNATURES") and s in _lib._SIGNATURES for s in hs.SETTERS)


def test_every_sequence_can_show_what_the_gpu_test_asserts_of_it():
    orders = hs.sequences()
    assert list(orders)[:2] == ["listed", "reversed"] and len(orders) == 8
    assert len({tuple(o) for o in orders.values()}) == 8
    for name, order in orders.items():
        assert sorted(order) == sorted(k.name for k in hs.CATALOGUE), name
        assert all(hs.sequence_shows(order).values()), (name, hs.sequence_shows(order))


def test_the_inputs_are_a_function_of_the_kind():
    for name in ("sr_unaligned", "shared_split", "prior_dist", "solve_offcentre"):
        a, b = hs.inputs(hs.BY_NAME[name]), hs.inputs(hs.BY_NAME[name])
        assert list(a) == list(b) and all((a[k] == b[k]).all() and a[k].flags["C_CONTIGUOUS"] for k in a), name
    off = hs.inputs(hs.BY_NAME["solve_offcentre"])["cam"]
    assert (off[:, 4] != 32).all() and (off[:, 5] != 8).all()
    assert hs.inputs(hs.BY_NAME["zero_images"]) == {} == hs.inputs(hs.BY_NAME["release"])
