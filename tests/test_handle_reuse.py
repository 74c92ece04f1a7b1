"""-m gpu: a reused gclm_handle against a fresh one, over every call transition of tests/handle_sequences.py.

A handle owns the whole solve workspace, two scratch planes, the split shared-intrinsics session and seven sticky knobs, and
LMOptimizer keeps one per (device, stream), reconfigured in place: the library's normal life is one long sequence of different
calls on one handle.  The plan of a call depends on its arguments, the handle's configuration and its knobs, nothing else, so
a call on a used handle returns the BITS of the same call on a handle that has done nothing before -- no tolerance anywhere in
this file.  The float64 step, stage, update and early-stop gates hold the fresh handle; these tests tie every reused one to it.

Every output buffer is prefilled with the same canary bytes in every run: a slot a path does not write compares equal, a slot
it writes differently does not.  Every device buffer a sequence has handed to the handle stays allocated until the sequence
has ended and the device is synchronised, so a stale pointer would show as a bit difference, not as an illegal access."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import handle_sequences as hs

pytestmark = pytest.mark.gpu

CANARY = int(np.array([0xA5A5A5A5], np.uint32).view(np.int32)[0])
FIELD_KEYS = ("up_field", "latitude_field", "up_confidence", "latitude_confidence")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from geocalib_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def host_inputs(name):
    return hs.inputs(hs.BY_NAME[name])


def config_struct(fields):
    from geocalib_amd import _lib
    cfg = _lib.GclmConfig.default(0)
    for k, v in fields.items():
        assert hasattr(cfg, k), k
        setattr(cfg, k, v)
    return cfg


class Call:
    """One call made on a handle: its output tensors (int32 views of what the library wrote over the canary), what was
    read from the handle on the host right after it, and the bytes the handle held then."""

    def __init__(self, kind):
        self.kind, self.out, self.host = kind, {}, {}
        self.workspace = self.slat = self.cpack = 0


class Session:
    """One gclm_handle and every device buffer it was ever handed."""

    def __init__(self, dev):
        from geocalib_amd import _lib
        self._lib, self.lib, self.dev = _lib, _lib.load(), dev
        self.ptr, self.key, self.keep = None, None, []

    def check(self, rc, what):
        self._lib.check(rc, self.ptr, what)

    def bytes(self):
        if self.ptr is None:
            return 0, 0, 0
        return (self.lib.gclm_workspace_bytes(self.ptr), self.lib.gclm_slat_plane_bytes(self.ptr),
                self.lib.gclm_conf_pack_bytes(self.ptr))

    def _configure(self, kind):
        """gclm_create on the first call, gclm_configure only where the configuration differs (as _Handle.configure)."""
        fields = kind.config()
        if self.ptr is None:
            cfg = config_struct(fields if fields is not None else hs.BASE_CFG)
            self.ptr = C.c_void_p()
            self._lib.check(self.lib.gclm_create(C.byref(self.ptr), C.byref(cfg)), None, "gclm_create")
            self.key = cfg.key()
        elif fields is not None:
            cfg = config_struct(fields)
            if cfg.key() != self.key:
                self.check(self.lib.gclm_configure(self.ptr, C.byref(cfg)), "gclm_configure")
                self.key = cfg.key()
        for setter, value in zip(hs.SETTERS, kind.all_knobs().values()):
            self.check(getattr(self.lib, setter)(self.ptr, int(value)), setter)

    def _upload(self, kind):
        dev_in = {}
        for k, v in host_inputs(kind.name).items():
            t = torch.from_numpy(v)
            if kind.unaligned and k in FIELD_KEYS:               # a view 4 bytes into its allocation
                flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=self.dev)
                flat[1:].copy_(t.reshape(-1))
                d = flat[1:].view(t.shape)
                assert d.data_ptr() % 16 == 4
            else:
                d = t.to(self.dev)
                assert d.data_ptr() % 16 == 0
            dev_in[k] = d
            self.keep.append(d)
        return dev_in

    def _canary(self, *shape):
        t = torch.full(shape, CANARY, dtype=torch.int32, device=self.dev)
        self.keep.append(t)
        return t

    def run(self, kind) -> Call:
        lib, call = self.lib, Call(kind)
        self._configure(kind)
        d = self._upload(kind)
        P = lambda k: d[k].data_ptr() if k in d else None      # noqa: E731
        planes = [P(k) for k in FIELD_KEYS]
        B, H, W = kind.B, kind.H, kind.W
        steps = kind.config()["num_steps"] if kind.cfg is not None else 0
        o = call.out
        if kind.entry in ("gclm_calibrate", "gclm_calibrate_ex", "gclm_calibrate_recorded"):
            o["cam"], o["grav"], o["info"] = self._canary(B, 8), self._canary(B, 3), self._canary(B, self._lib.INFO_STRIDE)
            cols = d["prior_dist"].shape[1] if "prior_dist" in d else 0
            args = [self.ptr, *planes, B, H, W, P("scales"), P("prior_focal"), P("prior_gravity"), P("prior_dist"), cols,
                    o["cam"].data_ptr(), o["grav"].data_ptr(), o["info"].data_ptr()]
            if kind.entry == "gclm_calibrate_ex":
                args.append(P("sin_latitude"))
            elif kind.entry == "gclm_calibrate_recorded":
                o["record"] = self._canary(B, steps, self._lib.LM_RECORD_STRIDE)
                args.append(o["record"].data_ptr())
            self.check(getattr(lib, kind.entry)(*args, None), kind.entry)
        elif kind.entry == "gclm_solve_ex":
            o["cam"], o["grav"] = d["cam"].view(torch.int32), d["grav"].view(torch.int32)       # in: the state, out: the result
            o["info"] = self._canary(B, self._lib.INFO_STRIDE)
            self.check(lib.gclm_solve_ex(self.ptr, *planes, B, H, W, d["cam"].data_ptr(), d["grav"].data_ptr(), o["info"].data_ptr(),
                                         None, None), kind.entry)
        elif kind.entry == "gclm_solve":                         # the empty batch
            assert B == 0
            self.check(lib.gclm_solve(self.ptr, None, None, None, None, 0, H, W, None, None, None, None), kind.entry)
        elif kind.entry == "gclm_system":
            o["cost"], o["grad"], o["hess"] = self._canary(B, 2), self._canary(B, 5), self._canary(B, 25)
            self.check(lib.gclm_system(self.ptr, *planes, B, H, W, d["cam"].data_ptr(), d["grav"].data_ptr(), kind.as_rpf,
                                       o["cost"].data_ptr(), o["grad"].data_ptr(), o["hess"].data_ptr(), None), kind.entry)
        elif kind.entry in ("split", "abandoned"):
            part = self._canary(kind.groups, self._lib.SHARED_PARTIAL_STRIDE)
            self.check(lib.gclm_shared_begin(self.ptr, *planes, B, H, W, d["cam"].data_ptr(), d["grav"].data_ptr(),
                                             d["group_of_frame"].data_ptr(), kind.groups, None), "gclm_shared_begin")
            for step in range(steps if kind.entry == "split" else 2):       # the partials pass straight from reduce to apply
                self.check(lib.gclm_shared_reduce(self.ptr, step, part.data_ptr(), None), "gclm_shared_reduce")
                self.check(lib.gclm_shared_apply(self.ptr, step, part.data_ptr(), None), "gclm_shared_apply")
            if kind.entry == "split":
                o["info"] = self._canary(B, self._lib.INFO_STRIDE)
                self.check(lib.gclm_shared_finish(self.ptr, o["info"].data_ptr(), None), "gclm_shared_finish")
                o["cam"], o["grav"], o["partials"] = d["cam"].view(torch.int32), d["grav"].view(torch.int32), part
        elif kind.entry == "gclm_release_workspace":
            self.check(lib.gclm_release_workspace(self.ptr), kind.entry)
            assert self.bytes() == (0, 0, 0)
        else:
            raise AssertionError(kind.entry)
        if not kind.result:
            call.out = {}
        if kind.all_knobs()["timing"]:                          # the launch count is compared too (waits for the launches)
            n, ms = C.c_int(0), C.c_float(0)
            self.check(lib.gclm_last_pass_timing(self.ptr, C.byref(n), C.byref(ms)), "gclm_last_pass_timing")
            call.host["sweep_launches"] = n.value
        call.workspace, call.slat, call.cpack = self.bytes()
        return call

    def session_is_over(self):
        """gclm_shared_reduce return code with no session: -4, and nothing is launched."""
        part = self._canary(2, self._lib.SHARED_PARTIAL_STRIDE)
        return self.lib.gclm_shared_reduce(self.ptr, 0, part.data_ptr(), None)

    def results(self, calls):
        """The outputs of `calls` on the host, once everything the handle was asked to do has run."""
        torch.cuda.synchronize()
        return [{**{k: v.cpu() for k, v in c.out.items()}, **c.host} for c in calls]

    def close(self):
        torch.cuda.synchronize()
        if self.ptr is not None:
            self.lib.gclm_destroy(self.ptr)
            self.ptr = None
        self.keep.clear()


_FRESH = {}


def fresh(dev, kind):
    """The call of `kind` on a handle that has done nothing before: (outputs, Call).  Once per module, never changed."""
    if kind.name not in _FRESH:
        s = Session(dev)
        try:
            call = s.run(kind)
            out, = s.results([call])
        finally:
            s.close()
        assert kind.result and out, kind.name
        _FRESH[kind.name] = (out, call)
    return _FRESH[kind.name]


def differences(got: dict, want: dict) -> list:
    """The outputs that differ in any bit (int32 views: a NaN equals itself, +0 differs from -0)."""
    assert set(got) == set(want), (sorted(got), sorted(want))
    return [k for k in want if not (torch.equal(got[k], want[k]) if torch.is_tensor(want[k]) else got[k] == want[k])]


def test_the_fresh_calls_take_the_paths_they_name(dev):
    """The catalogue's fresh runs wrote every output over the canary and held the planes their kinds name."""
    for kind in hs.RESULT_KINDS:
        out, call = fresh(dev, kind)
        for k in ("cam", "grav", "cost", "grad", "hess"):
            if k in out:
                assert not (out[k] == CANARY).any(), (kind.name, k)
        if kind.name == "sr_slat":
            assert call.slat == kind.B * kind.H * kind.W * 4
        elif kind.model == "pinhole" or kind.sin_lat:           # never the library's plane of sin(latitude)
            assert call.slat == 0, (kind.name, call.slat)
        assert call.cpack == (kind.B * kind.H * kind.W * 4 if kind.name == "pinhole_cpack" else 0), (kind.name, call.cpack)
    assert fresh(dev, hs.BY_NAME["sr_slat"])[0]["sweep_launches"] == hs.BY_NAME["sr_slat"].config()["num_steps"] + 1
    info = fresh(dev, hs.BY_NAME["early_b5"])[0]["info"].view(torch.float32)
    assert 1 <= info[0, 0] <= 30


@pytest.mark.parametrize("first", [k.name for k in hs.CATALOGUE])
def test_every_ordered_pair(dev, first):
    """A on a new handle, then B on the same handle: B's outputs are fresh(B)'s bits, for every result kind B != A."""
    a = hs.BY_NAME[first]
    seconds = [b for b in hs.RESULT_KINDS if b.name != first]
    assert hs.N_PAIRS == 675 == sum(len(hs.RESULT_KINDS) - k.result for k in hs.CATALOGUE)
    compared, bad = 0, []
    for b in seconds:
        want, _ = fresh(dev, b)
        s = Session(dev)
        try:
            s.run(a)
            call = s.run(b)
            if a.entry == "abandoned":
                assert s.session_is_over() == -4, (first, b.name)
            got, = s.results([call])
        finally:
            s.close()
        diff = differences(got, want)
        compared += 1
        if diff:
            bad.append((b.name, diff))
    assert compared == len(hs.RESULT_KINDS) - a.result          # none skipped: 24 after a result kind, 25 after a disturbance
    assert not bad, (first, bad)


@pytest.mark.parametrize("order", list(hs.sequences()))
def test_long_sequences(dev, order):
    """The whole catalogue on ONE handle, in a given order: every result kind returns fresh's bits, and the sequence shows,
    from what the handle reports, that it really met a regrown workspace, a call below the high-water mark, planes kept
    across calls that must not use them, and a session abandoned before another call."""
    names = hs.sequences()[order]
    assert all(hs.sequence_shows(names).values())
    for kind in hs.RESULT_KINDS:
        fresh(dev, kind)
    s = Session(dev)
    rises, below, kept_slat, kept_cpack, after_abandoned, pending = 0, 0, 0, 0, 0, False
    calls = []
    try:
        for name in names:
            kind = hs.BY_NAME[name]
            ws0, slat0, cpack0 = s.bytes()
            call = s.run(kind)
            calls.append(call)
            rises += call.workspace > ws0
            if kind.result:
                alone = fresh(dev, kind)[1]
                below += call.workspace == ws0 and alone.workspace < ws0
                kept_slat += slat0 > 0 and alone.slat == 0
                kept_cpack += cpack0 > 0 and alone.cpack == 0
            if pending:
                assert s.session_is_over() == -4, (order, name)
                after_abandoned += 1
            pending = kind.entry == "abandoned"
        got = s.results(calls)
    finally:
        s.close()
    bad = [(c.kind.name, d) for c, g in zip(calls, got) if c.kind.result and (d := differences(g, fresh(dev, c.kind)[0]))]
    assert not bad, (order, names, bad)
    assert sum(c.kind.result for c in calls) == len(hs.RESULT_KINDS)
    assert rises >= 2 and below >= 1 and kept_slat >= 1 and kept_cpack >= 1 and after_abandoned == 1, \
        (order, rises, below, kept_slat, kept_cpack, after_abandoned)


@pytest.mark.parametrize("name", [k.name for k in hs.RESULT_KINDS])
def test_same_call_twice(dev, name):
    kind = hs.BY_NAME[name]
    want, _ = fresh(dev, kind)
    s = Session(dev)
    try:
        got = s.results([s.run(kind), s.run(kind)])
    finally:
        s.close()
    assert [differences(g, want) for g in got] == [[], []], name


def test_an_empty_call_ends_an_abandoned_session(dev):
    """A B = 0 solve (or gclm_system) plans nothing; it still is a call on the handle, and the session before it is over."""
    for entry in ("gclm_solve", "gclm_system"):
        s = Session(dev)
        try:
            s.run(hs.BY_NAME["abandoned_session"])
            one = s._canary(16)
            if entry == "gclm_solve":
                rc = s.lib.gclm_solve(s.ptr, None, None, None, None, 0, 16, 64, None, None, None, None)
            else:
                rc = s.lib.gclm_system(s.ptr, None, None, None, None, 0, 16, 64, *[one.data_ptr()] * 2, 0, *[one.data_ptr()] * 3, None)
            assert rc == 0, entry
            assert s.session_is_over() == -4, entry
        finally:
            s.close()


# ------------------------------------------------------------------ the Python layer: one handle, reconfigured

def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def _same_results(a: dict, b: dict) -> list:
    assert set(a) == set(b), (sorted(a), sorted(b))
    raw = lambda v: v._data if hasattr(v, "_data") else v      # noqa: E731
    return [k for k in a if torch.is_tensor(raw(a[k])) and not torch.equal(_bits(raw(a[k])), _bits(raw(b[k])))]


def test_one_geocalib_and_one_optimizer_reconfigure_one_handle(dev):
    from geocalib_amd import LMOptimizer
    from geocalib_amd.extractor import GeoCalib
    from oracle import synth
    H, W = 32, 64
    planes = {k: torch.from_numpy(v).to(dev) for k, v in synth.make_fields(41, range(3), "pinhole", H, W)[0].items()}

    def field_model(img_data):
        return {k: v[:img_data["image"].shape[0]] for k, v in planes.items()}

    def preprocess(img):
        return {"image": img, "scales": torch.ones(2, device=dev), "crop_pad": torch.zeros(2, device=dev)}

    one, three = torch.rand(1, 3, H, W, device=dev), torch.rand(3, 3, H, W, device=dev)
    serving = [dict(img=one, camera_model="pinhole"),
               dict(img=one, camera_model="radial", priors={"focal": torch.tensor(40.0, device=dev)}),
               dict(img=three, camera_model="pinhole", shared_intrinsics=True),
               dict(img=one, camera_model="pinhole")]
    kept = GeoCalib(field_model, preprocess)
    for i, kw in enumerate(serving):
        got = kept.calibrate(**kw)
        assert len(kept.optimizer._handles) == 1, i
        want = GeoCalib(field_model, preprocess).calibrate(**kw)
        torch.cuda.synchronize()
        assert _same_results(got, want) == [], (i, _same_results(got, want))
    data = {k: torch.from_numpy(v).to(dev) for k, v in synth.make_fields(43, range(3), "simple_radial", H, W)[0].items()}
    conf = {"camera_model": "simple_radial", "num_steps": 5, "early_stop": False}
    opt = LMOptimizer(conf)
    for i, mode in enumerate(("eval", "train", "eval")):
        got = getattr(opt, mode)()(dict(data))
        assert len(opt._handles) == 1, i
        want = getattr(LMOptimizer(conf), mode)()(dict(data))
        torch.cuda.synchronize()
        assert ("covariance" in got) == (mode == "eval")
        assert _same_results(got, want) == [], (i, mode, _same_results(got, want))
