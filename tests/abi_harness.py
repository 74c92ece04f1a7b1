"""What the *_abi.py tests share (a plain module, like the *_gate.py files): the parser of include/gclm.h's declarations, the
assertion that an entry point is declared with given types, bound in _lib._SIGNATURES, exported by the built library and of
ABI 610, and the path of the LLVM tools.  Each test file keeps its own ARGS list and its own table of refused calls."""
import ctypes as C
import os
import re

from conftest import ROOT

from geocalib_amd import _lib

HEADER = os.path.join(ROOT, "include", "gclm.h")
LLVM = "/opt/rocm/lib/llvm/bin"
SCALARS = {"int": C.c_int, "size_t": C.c_size_t}


def declared(name, ret="int", names=False):
    """The parameter types of `name` as include/gclm.h declares it (names=True: the parameters as written, with their names)."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} not declared in include/gclm.h"
    params = [a.strip() for a in m.group(1).split(",")]
    return params if names else [re.sub(r"\s*\b\w+$", "", a).replace(" *", "*") for a in params]


def assert_declared_exported_and_bound(name, arg_types, ret="int"):
    """`name` is declared with `arg_types` and result `ret`, bound with as many arguments -- every int and size_t as such, the
    result likewise -- listed as exported and found in the built library, whose ABI is 610.  Returns the bound argument types."""
    types = declared(name, ret)
    assert types == arg_types, types
    res, args = _lib._SIGNATURES[name]
    assert res is SCALARS[ret] and len(args) == len(arg_types)
    for a, t in zip(args, arg_types):
        assert (a is SCALARS[t]) if t in SCALARS else (a not in SCALARS.values()), (name, a, t)
    assert name in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    assert hasattr(C.CDLL(_lib.LIB_PATH), name)
    assert lib.gclm_version() == 610 == _lib.ABI_VERSION
    return args
