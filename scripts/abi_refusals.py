"""Build container: do the seventeen entry points that take no handle (csrc/gclm_entry.hip) answer every argument tuple with the
return code they gave at git revision REV?  (The argument checks moved onto one checker, csrc/gclm_args.h; a refusal that
changed would be a kernel launched on ranges it was never meant to see, or a caller turned away.)

usage: python scripts/abi_refusals.py REV [--tuples N=20000] [--seed S=0] [--lib-at-rev PATH] [--cost]
Builds REV's library from `git archive` in a temporary directory (--lib-at-rev: takes one built before), loads it and the
working tree's with ctypes, and for each entry starts from a valid tuple of FAKE device addresses and mutates one to three
arguments (seeded): NULL, a pointer off by 1 / 2 / 4 / 8 bytes, a pointer placed on, against (abutting) or one element inside
the start or the end of another argument's range, sizes 0 / 1 / 2 / -1 / 2^31 - 1, the image limit and one more, H x W either
side of 2^31 and 2^32, models -1 .. 4, cam_batch 0 / 1 / B / B + 1, threshold counts -1 .. 9 with NaN and infinite
thresholds.  What the host dereferences is real host memory: the thresholds, the source and size tables of the panorama
entry, the tables of the multi-upsampler and the read probe.  A tuple whose byte counts reach 2^62 is drawn again: only there
may the two libraries differ (a count that wrapped at REV saturates now).
WITHOUT a device the return code classifies a call: a valid one answers -10 (the launch finds no device), an empty batch 0,
a refusal its code.  The script therefore EXITS AT ONCE WHERE A HIP DEVICE IS VISIBLE -- a tuple that passes the checks
would be launched on the fake addresses.  The log goes to profiles/abi_refusals.log; exit status 0 when no tuple differs.
--cost times 10^6 calls of gclm_perspective_fields and of gclm_field_errors that are refused late (a misaligned d_lat, a
misaligned latitude map; no HIP call is made), and of gclm_perspective_fields refused at its very last check, five
repetitions per library, alternating (scripts/probes/refusal_cost.c), into profiles/abi_refusals_cost.json; exit status 0
when no median exceeds REV's by more than the spread of REV's five."""
import ctypes as C
import glob
import json
import math
import os
import random
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join("geocalib_amd", "lib", "libgeocalib_hip.so")


def exit_if_a_device_is_visible():
    n = C.c_int(0)
    visible = os.path.exists("/dev/kfd") or bool(glob.glob("/dev/dri/renderD*"))
    if not visible:
        try:
            visible = C.CDLL("libamdhip64.so").hipGetDeviceCount(C.byref(n)) == 0 and n.value > 0
        except OSError:
            pass
    if visible:
        sys.exit("abi_refusals.py: a HIP device is visible here; this script passes fake device addresses and runs only without one")


exit_if_a_device_is_visible()
sys.path.insert(0, ROOT)
from geocalib_amd import _lib  # noqa: E402  (the bound signatures; nothing is loaded yet)

NAN, INF, I31 = math.nan, math.inf, 2 ** 31 - 1
LIMIT = 65535                                    # images per call
VALUES = {"batch": [0, 1, 2, -1, LIMIT, LIMIT + 1, I31], "dim": [0, 1, 2, 3, -1, LIMIT, LIMIT + 1, I31],
          "small": [0, 1, 2, -1, 4, 5, 6, I31], "flag": [0, 1, 2, -1], "model": [-1, 0, 1, 2, 3, 4], "count": [0, 1, 2, -1, 8, 9],
          "nthr": list(range(-1, 10)), "f32": [1.0, 0.01, 0.0, -1.0, NAN, INF], "size": [0, 4, 6, 1024, 2 ** 40], "word": [0, 1, 7, 2 ** 40]}
HW = [(32768, 65536), (32768, 65535), (46340, 46340), (46341, 46341), (65536, 65536), (65535, 65537), (65536, 32767), (I31, 1), (1, I31),
      (I31, 2), (2 ** 30, 4), (3, 2 ** 30)]
SRC_HW = [0, 1, 2, -1, 64, I31]


def A(i):
    return 0x10000000 * (i + 1)                  # fake device addresses, 256 MiB apart


# name -> (arguments in order as (name, kind, valid value), {pointer: the factors of its float count})
ENTRIES = {
    "gclm_gradient_hessian": ([("J", "ptr", A(0)), ("r", "ptr", A(1)), ("w", "ptr", A(2)), ("B", "batch", 2), ("N", "dim", 100), ("R", "small", 2),
                               ("P", "small", 3), ("acc", "flag", 0), ("G", "ptr", A(3)), ("Hs", "ptr", A(4)), ("stream", "stream", None)],
                              {"J": ("B", "N", "R", "P"), "r": ("B", "N", "R"), "w": ("B", "N"), "G": ("B", "P"), "Hs": ("B", "P", "P")}),
    "gclm_optimizer_step": ([("G", "ptr", A(0)), ("Hs", "ptr", A(1)), ("lam", "ptr", A(2)), ("scalar", "flag", 0), ("eps", "f32", 1e-6), ("B", "batch", 2),
                             ("P", "small", 3), ("delta", "ptr", A(3)), ("failed", "ptr", A(4)), ("stream", "stream", None)],
                            {"G": ("B", "P"), "Hs": ("B", "P", "P"), "lam": ("B",), "delta": ("B", "P"), "failed": ("B",)}),
    "gclm_residual_fields": ([("model", "model", 1), ("up", "ptr", A(0)), ("lat", "ptr", A(1)), ("cam", "ptr", A(2)), ("grav", "ptr", A(3)), ("B", "batch", 2),
                              ("H", "dim", 48), ("W", "dim", 64), ("r_up", "ptr", A(4)), ("r_lat", "ptr", A(5)), ("stream", "stream", None)],
                             {"up": (2, "B", "H", "W"), "lat": ("B", "H", "W"), "cam": ("B", 8), "grav": ("B", 3), "r_up": (2, "B", "H", "W"),
                              "r_lat": ("B", "H", "W")}),
    "gclm_huber_costs": ([("res", "ptr", A(0)), ("n", "size", 1024), ("dim", "small", 2), ("scale", "f32", 0.01), ("conf", "ptr", A(1)), ("cost", "ptr", A(2)),
                          ("weight", "ptr", A(3)), ("second", "ptr", A(4)), ("stream", "stream", None)],
                         {"res": ("n", "dim"), "conf": ("n",), "cost": ("n",), "weight": ("n",), "second": ("n",)}),
    "gclm_jacobian_fields": ([("model", "model", 1), ("cam", "ptr", A(0)), ("grav", "ptr", A(1)), ("B", "batch", 2), ("H", "dim", 48), ("W", "dim", 64),
                              ("spherical", "flag", 1), ("logf", "flag", 1), ("J_up", "ptr", A(2)), ("J_lat", "ptr", A(3)), ("stream", "stream", None)],
                             {"cam": ("B", 8), "grav": ("B", 3), "J_up": ("B", "H", "W", 2, 5), "J_lat": ("B", "H", "W", 5)}),
    "gclm_upsample_fields": ([("src", "ptr", A(0)), ("planes", "small", 3), ("h", "dim", 12), ("w", "dim", 16), ("H", "dim", 48), ("W", "dim", 64),
                              ("dst", "ptr", A(1)), ("stream", "stream", None)], {"src": ("planes", "h", "w"), "dst": ("planes", "H", "W")}),
    "gclm_upsample_fields_multi": ([("srcs", "ptrs", [A(0), A(1), A(2)] + [None] * 5), ("dsts", "ptrs", [A(3), A(4), A(5)] + [None] * 5),
                                    ("planes", "ints", [2, 1, 3, 0, 0, 0, 0, 0]), ("n", "count", 3), ("h", "dim", 12), ("w", "dim", 16), ("H", "dim", 48),
                                    ("W", "dim", 64), ("stream", "stream", None)], {}),
    "gclm_pack_fields": ([("up_raw", "ptr", A(0)), ("up_lc", "ptr", A(1)), ("lat_raw", "ptr", A(2)), ("lat_lc", "ptr", A(3)), ("B", "batch", 2), ("H", "dim", 48),
                          ("W", "dim", 64), ("up", "ptr", A(4)), ("upc", "ptr", A(5)), ("lat", "ptr", A(6)), ("latc", "ptr", A(7)), ("stream", "stream", None)],
                         {"up_raw": (2, "B", "H", "W"), "up": (2, "B", "H", "W"), **{k: ("B", "H", "W") for k in ("up_lc", "lat_raw", "lat_lc", "upc", "lat", "latc")}}),
    "gclm_undistort_image": ([("model", "model", 1), ("cam", "ptr", A(0)), ("nb", "nb", 1), ("src", "ptr", A(1)), ("B", "batch", 2), ("C", "small", 3),
                              ("Hin", "dim", 48), ("Win", "dim", 64), ("H", "dim", 48), ("W", "dim", 64), ("dst", "ptr", A(2)), ("stream", "stream", None)],
                             {"cam": ("nb", 8), "src": ("B", "C", "Hin", "Win"), "dst": ("B", "C", "H", "W")}),
    "gclm_perspective_fields": ([("model", "model", 1), ("cam", "ptr", A(0)), ("grav", "ptr", A(1)), ("B", "batch", 2), ("H", "dim", 48), ("W", "dim", 64),
                                 ("norm", "flag", 1), ("up", "ptr", A(2)), ("lat", "ptr", A(3)), ("stream", "stream", None)],
                                {"cam": ("B", 8), "grav": ("B", 3), "up": (2, "B", "H", "W"), "lat": ("B", "H", "W")}),
    "gclm_field_errors_workspace": ([("B", "batch", 2), ("H", "dim", 48), ("W", "dim", 64), ("nthr", "nthr", 4)], {}),
    "gclm_field_errors": ([("model", "model", 1), ("cam", "ptr", A(0)), ("grav", "ptr", A(1)), ("B", "batch", 2), ("H", "dim", 48), ("W", "dim", 64), ("up", "ptr", A(2)),
                           ("lat", "ptr", A(3)), ("upc", "ptr", A(4)), ("latc", "ptr", A(5)), ("nthr", "nthr", 4), ("thr", "floats", [1.0, 3.0, 5.0, 10.0]),
                           ("ws", "ptr", A(6)), ("ws_bytes", "ws_bytes", 1 << 24), ("stats", "ptr", A(7)), ("uerr", "ptr", A(8)), ("lerr", "ptr", A(9)),
                           ("stream", "stream", None)],
                          {"cam": ("B", 8), "grav": ("B", 3), "up": (2, "B", "H", "W"), "stats": ("B", 2, "nthr+2"), "ws": "workspace",
                           **{k: ("B", "H", "W") for k in ("lat", "upc", "latc", "uerr", "lerr")}}),
    "gclm_render_from_pano": ([("model", "model", 1), ("cam", "ptr", A(0)), ("nb", "nb", 1), ("rot", "ptr", A(1)), ("srcs", "ptrs", [A(2), A(2)]),
                               ("hw", "ints", [64, 128, 64, 128]), ("B", "batch", 2), ("C", "small", 3), ("H", "dim", 48), ("W", "dim", 64), ("dst", "ptr", A(3)),
                               ("stream", "stream", None)], {"cam": ("nb", 8), "rot": ("B", 9), "dst": ("B", "C", "H", "W"), "srcs": ("C", 64, 128)}),
    "gclm_read_probe": ([("planes", "ptrs", [A(k) for k in range(8)]), ("n", "count", 3), ("floats", "size", 1024), ("stream", "stream", None)], {}),
    "gclm_synth_fields": ([("model", "model", 1), ("seed", "word", 7), ("first", "word", 0), ("B", "batch", 2), ("H", "dim", 48), ("W", "dim", 64), ("sigma", "f32", 0.01),
                           ("up", "ptr", A(0)), ("lat", "ptr", A(1)), ("upc", "ptr", A(2)), ("latc", "ptr", A(3)), ("gt_cam", "ptr", A(4)), ("gt_grav", "ptr", A(5)),
                           ("stream", "stream", None)], {"up": (2, "B", "H", "W"), "lat": ("B", "H", "W"), "upc": ("B", "H", "W"), "latc": ("B", "H", "W"),
                                                        "gt_cam": ("B", 8), "gt_grav": ("B", 3)}),
}
ENTRIES["gclm_pack_fields_ex"] = (ENTRIES["gclm_pack_fields"][0][:-1] + [("slat", "ptr", A(8)), ("stream", "stream", None)],
                                  {**ENTRIES["gclm_pack_fields"][1], "slat": ("B", "H", "W")})
_s = ENTRIES["gclm_synth_fields"]
ENTRIES["gclm_synth_fields_grouped"] = (_s[0][:7] + [("group", "small", 1), ("run", "small", 0), ("stride", "small", 0)] + _s[0][7:], _s[1])
assert len(ENTRIES) == 17


def span(a, ranges, name):
    """Bytes of pointer argument `name` under the sizes in `a`, or None when a size is negative (the call is refused on it)."""
    n, factors = 4, ranges.get(name, (16,))
    if factors == "workspace":                   # gclm_field_errors: what the library asks for (0: sizes out of range)
        return WORKSPACE(a["B"], a["H"], a["W"], a["nthr"]) or None
    for f in factors:
        f = a["nthr"] + 2 if f == "nthr+2" else a[f] if isinstance(f, str) else f
        if not isinstance(f, int) or f < 0:
            return None
        n *= f
    return n


def mutate(rng, spec, ranges, a):
    """One mutation of the argument dict `a`, in place."""
    name, kind, _ = rng.choice([s for s in spec if s[1] != "stream"])
    if kind in VALUES:
        if name in ("H", "W") and rng.random() < 0.4:
            a["H"], a["W"] = rng.choice(HW)
        else:
            a[name] = rng.choice(VALUES[kind])
    elif kind == "nb":
        a[name] = rng.choice([0, 1, a["B"], a["B"] + 1])
    elif kind == "ws_bytes":
        a[name] = rng.choice([0, 1000, 1 << 24, 1 << 62])
    elif kind == "floats":
        v = a[name] or [1.0, 3.0, 5.0, 10.0]
        a[name] = rng.choice([None, v[:-1] + [NAN], [INF] + v[1:], [-INF] + v[1:], [1.0] * 9, [NAN] * 9, v])
    elif a[name] is None and kind in ("ints", "ptrs"):
        return                                   # (a table that is NULL has no element to change)
    elif kind == "ints":
        v = list(a[name])
        v[rng.randrange(len(v))] = rng.choice(SRC_HW)
        a[name] = rng.choice([None, v, v])
    elif kind in ("ptr", "ptrs"):
        others = [s[0] for s in spec if s[1] == "ptr" and s[0] != name and a[s[0]] is not None]
        own, new = span(a, ranges, name), None
        roll = rng.random()
        if roll < 0.15:
            new = None
        elif roll < 0.45 or not others or own is None:
            base = a[name] if kind == "ptr" else next((p for p in a[name] if p), None)
            new = (base or A(12)) + rng.choice([1, 2, 4, 8, 16])
        else:                                    # on, against, or one element inside the start or the end of another range
            q = rng.choice(others)
            lo, n = a[q], span(a, ranges, q)
            if n is None:
                return
            new = rng.choice([lo, lo + n, lo - own, lo + n - 4, lo - own + 4, lo + 4, lo + n // 2, lo - own // 2, lo + n + 4, lo - own - 4])
            if new <= 0 or new >= 1 << 63:
                return
        if kind == "ptr":
            a[name] = new
        elif rng.random() < 0.1:
            a[name] = None
        else:
            v = list(a[name])
            v[rng.randrange(len(v))] = new
            a[name] = v


def within_bounds(spec, ranges, a):
    """No byte count of the tuple reaches 2^62, no range passes 2^63, and no table is read past its end."""
    for name, kind, _ in spec:
        if kind in ("ptr", "ptrs"):
            n = span(a, ranges, name)
            tops = [a[name]] if kind == "ptr" else (a[name] or [])
            if n is not None and (n >= 1 << 62 or any(p and p + n >= 1 << 63 for p in tops)):
                return False
    if "hw" in a and a["hw"] is not None:       # the panorama's sources: C x Hs x Ws floats each
        C_ = a["C"]
        if C_ > 0 and any(h > 0 and w > 0 and 4 * C_ * h * w >= 1 << 62 for h, w in zip(a["hw"][::2], a["hw"][1::2])):
            return False
    if "nthr" in a and "B" in a and a["B"] > 0 and a["nthr"] > 0 and 4 * a["B"] * 2 * (2 + a["nthr"]) >= 1 << 62:
        return False
    return True


def marshal(spec, a):
    """The ctypes arguments of one call; tables are as long as the call's count claims (up to the image limit + 1)."""
    out = []
    count = a.get("B", 0) if "hw" in a else 8
    count = min(max(count, 2), LIMIT + 1)
    for name, kind, _ in spec:
        v = a[name]
        if v is None or kind in ("ptr", "stream") or kind in VALUES or kind in ("nb", "ws_bytes"):
            out.append(v)
        elif kind == "floats":
            out.append((C.c_float * max(len(v), 9))(*v))
        elif kind == "ptrs":
            out.append((C.c_void_p * max(count, len(v)))(*(list(v) + [v[0]] * (count - len(v)))))
        elif kind == "ints":
            reps = 2 if name == "hw" else 1
            out.append((C.c_int * max(reps * count, len(v)))(*(list(v) + list(v[:reps]) * (count - len(v) // reps))))
    return out


def load(path):
    lib = C.CDLL(path)
    for name in ENTRIES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._SIGNATURES[name]
    return lib


def lib_at(rev, tmp):
    for path in ("geocalib_amd/csrc", "include"):
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, path], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
    subprocess.run(["make", "-C", os.path.join(tmp, "geocalib_amd", "csrc"), "-j8"], check=True, capture_output=True)
    return os.path.join(tmp, LIB)


def compare(old, new, tuples, seed, log):
    global WORKSPACE
    WORKSPACE, total_diff = new.gclm_field_errors_workspace, 0
    for k, (name, (spec, ranges)) in enumerate(sorted(ENTRIES.items())):
        rng = random.Random(seed * 1000 + k)
        base = {s[0]: s[2] for s in spec}
        codes, diff, drawn = {}, 0, 0
        f_old, f_new = getattr(old, name), getattr(new, name)
        assert f_old(*marshal(spec, base)) == f_new(*marshal(spec, base)) != -3 or "workspace" in name, name
        while drawn < tuples:
            a = dict(base)
            for _ in range(rng.randint(1, 3)):
                mutate(rng, spec, ranges, a)
            if not within_bounds(spec, ranges, a):
                continue
            drawn += 1
            args = marshal(spec, a)
            r_old, r_new = f_old(*args), f_new(*args)
            key = r_new if r_new in (0, -1, -2, -3, -10) else "size"
            codes[key] = codes.get(key, 0) + 1
            if r_old != r_new:
                diff += 1
                if diff <= 20:
                    print(f"    DIFFERENT {name}: {rev_name} answers {r_old}, the working tree {r_new}: {a}", file=log)
        total_diff += diff
        line = f"{name}: {drawn} tuples, answers {dict(sorted(codes.items(), key=str))}: {'IDENTICAL' if not diff else f'{diff} DIFFERENT'}"
        print(line, file=log)
        print(line)
        log.flush()
    return total_diff


def cost(old_path, new_path, out_path):
    """ns per refused call (the refusal is each entry's last check) of both libraries: scripts/probes/refusal_cost.c, which
    calls the entries directly -- a ctypes call costs fifty times the checks it would be timing."""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "refusal_cost")
        subprocess.run(["cc", "-O2", os.path.join(ROOT, "scripts", "probes", "refusal_cost.c"), "-o", exe, "-ldl"], check=True)
        result = json.loads(subprocess.run([exe, old_path, new_path], check=True, capture_output=True, text=True).stdout)
    result["unit"] = "ns per call"
    for name, series in result.items():
        if not isinstance(series, dict):
            continue
        spread = max(series["rev"]) - min(series["rev"])
        m_old, m_new = statistics.median(series["rev"]), statistics.median(series["tree"])
        series.update(median_rev=m_old, median_tree=m_new, spread_rev=round(spread, 2), within=m_new <= m_old + spread)
        print(f"{name}: {rev_name} {series['rev']} median {m_old}; working tree {series['tree']} median {m_new}; spread of {rev_name} "
              f"{spread:.2f} ns: {'WITHIN' if series['within'] else 'OVER'}")
    json.dump(result, open(out_path, "w"), indent=1)
    return all(v["within"] for v in result.values() if isinstance(v, dict))


def main():
    global rev_name
    args = sys.argv[1:]
    opt = {"--tuples": "20000", "--seed": "0", "--lib-at-rev": None}
    for key in opt:
        if key in args:
            opt[key] = args[args.index(key) + 1]
            del args[args.index(key):args.index(key) + 2]
    do_cost = "--cost" in args
    rev_name = [x for x in args if x != "--cost"][0]
    with tempfile.TemporaryDirectory() as tmp:
        old_path, new_path = opt["--lib-at-rev"] or lib_at(rev_name, tmp), os.path.join(ROOT, LIB)
        if do_cost:
            ok = cost(old_path, new_path, os.path.join(ROOT, "profiles", "abi_refusals_cost.json"))
        else:
            old, new = load(old_path), load(new_path)
            with open(os.path.join(ROOT, "profiles", "abi_refusals.log"), "w") as log:
                print(f"abi_refusals.py {rev_name} --tuples {opt['--tuples']} --seed {opt['--seed']}", file=log)
                ok = compare(old, new, int(opt["--tuples"]), int(opt["--seed"]), log) == 0
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
