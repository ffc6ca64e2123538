"""topolow_scale_objective, its _ex twin and topolow_scale_to_original_distances without a device: declared, exported,
every TOPOLOW_ERR_BAD_ARGUMENT / TOPOLOW_ERR_UNSUPPORTED case (found before any device call, so this runs with or
without a GPU), and where the kernels live."""
import ctypes as C
import glob
import math
import os
import re

import numpy as np
import pytest

from topolow_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("topolow_scale_objective", "topolow_scale_objective_ex", "topolow_scale_to_original_distances")
BAD, UNSUPPORTED = _native.ERR_BAD_ARGUMENT, _native.ERR_UNSUPPORTED


def test_symbols_are_declared_exported_and_wrapped():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "topolow_relax.h")).read(), flags=re.S)
    lib = _native.load()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in _native.PROTOTYPES, name
        assert getattr(lib, name).restype is C.c_int
    assert callable(_native.scale_objective) and callable(_native.scale_to_original_distances)
    with pytest.raises(ValueError):
        _native.scale_objective(np.zeros((4, 2)), np.zeros((3, 2)), [1.0])
    with pytest.raises(ValueError):
        _native.scale_to_original_distances(np.zeros(4), np.zeros((4, 1)))


class Args:
    """A valid call's arguments; a case replaces some."""

    def __init__(self, **kw):
        self.pos = np.arange(10.0).reshape(5, 2, order="F") ** 1.5
        self.red = np.arange(5.0).reshape(5, 1, order="F")
        self.scales = np.array([1.0, 2.0])
        self.F, self.G, self.H = np.full(8, -7.0), C.c_double(-7.0), C.c_double(-7.0)
        self.scale, self.objective, self.evals = C.c_double(-7.0), C.c_double(-7.0), C.c_int32(-7)
        self.ts, self.tf = np.full(4, -7.0), np.full(4, -7.0)
        a = dict(positions=_native._dp(self.pos), reduced=_native._dp(self.red), n=5, ndim=2, k=1,
                 scales=_native._dp(self.scales), m=2, objective=_native._dp(self.F), chunk=0, lower=0.01, upper=40.0,
                 tol=1e-4, scale=C.byref(self.scale), trace_scale=_native._dp(self.ts), trace_objective=_native._dp(self.tf),
                 trace_len=4)
        for key, value in kw.items():
            if key in ("pos", "red", "scales"):             # replace the array itself
                setattr(self, key, value)
                a[{"pos": "positions", "red": "reduced", "scales": "scales"}[key]] = _native._dp(value)
            else:
                a[key] = value
        self.a = a

    def untouched(self):
        return ((self.F == -7.0).all() and self.G.value == -7.0 and self.H.value == -7.0 and self.scale.value == -7.0
                and self.objective.value == -7.0 and self.evals.value == -7 and (self.ts == -7.0).all()
                and (self.tf == -7.0).all())


def call_objective(lib, ex, **kw):
    x = Args(**kw)
    a = x.a
    err = C.create_string_buffer(256)
    head = (a["positions"], a["reduced"], a["n"], a["ndim"], a["k"], a["scales"], a["m"], a["objective"], C.byref(x.G),
            C.byref(x.H), -1)
    if ex:
        rc = lib.topolow_scale_objective_ex(*head, a["chunk"], None, err, len(err))
    else:
        rc = lib.topolow_scale_objective(*head, err, len(err))
    assert x.untouched()                                            # nothing was written
    return rc, err.value


def call_minimiser(lib, **kw):
    x = Args(**kw)
    a = x.a
    err = C.create_string_buffer(256)
    rc = lib.topolow_scale_to_original_distances(
        a["positions"], a["reduced"], a["n"], a["ndim"], a["k"], a["lower"], a["upper"], a["tol"], a["scale"],
        C.byref(x.objective), C.byref(x.evals), a["trace_scale"], a["trace_objective"], a["trace_len"], -1, err, len(err))
    assert x.untouched()
    return rc, err.value


def nonfinite(shape, value, at):
    a = np.ones(shape, order="F")
    a[at] = value
    return a


SHARED = [dict(positions=None), dict(reduced=None), dict(n=1), dict(n=0), dict(n=-3), dict(k=0), dict(k=-1), dict(k=3)]
SHARED += [dict(pos=nonfinite((5, 2), v, (4, 1))) for v in (math.nan, math.inf, -math.inf)]
SHARED += [dict(red=nonfinite((5, 1), v, (2, 0))) for v in (math.nan, math.inf)]


@pytest.mark.parametrize("ex", [False, True])
def test_objective_argument_errors_come_before_any_device_call(ex):
    lib = _native.load()
    cases = SHARED + [dict(scales=None), dict(objective=None), dict(m=0), dict(m=-1), dict(m=9)]
    cases += [dict(scales=np.array([1.0, v])) for v in (math.nan, math.inf, -math.inf)]
    for kw in cases:
        rc, msg = call_objective(lib, ex, **kw)
        assert rc == BAD and msg.startswith(b"topolow_scale_objective: ") and len(msg) > 30, (kw, rc, msg)
    wide = np.ones((5, 17), order="F")
    rc, msg = call_objective(lib, ex, pos=wide, ndim=17)
    assert rc == UNSUPPORTED and b"between 1 and 16" in msg
    rc, msg = call_objective(lib, ex, pos=wide, ndim=17, k=18)       # k > ndim is the caller's mistake at any ndim
    assert rc == BAD and msg
    if ex:
        for chunk in (-64, 1, 63, 100, 192, 1024):
            rc, msg = call_objective(lib, True, chunk=chunk)
            assert rc == BAD and b"64, 128, 256 or 512" in msg, chunk


def test_minimiser_argument_errors_come_before_any_device_call():
    lib = _native.load()
    cases = SHARED + [dict(scale=None), dict(lower=1.0, upper=1.0), dict(lower=2.0, upper=1.0), dict(tol=0.0),
                      dict(tol=-1e-4), dict(trace_len=-1), dict(trace_scale=None), dict(trace_objective=None)]
    for name in ("lower", "upper", "tol"):
        cases += [{name: v} for v in (math.nan, math.inf, -math.inf)]
    for kw in cases:
        rc, msg = call_minimiser(lib, **kw)
        assert rc == BAD and msg.startswith(b"topolow_scale_to_original_distances: ") and len(msg) > 45, (kw, rc, msg)
    rc, msg = call_minimiser(lib, pos=np.ones((5, 17), order="F"), ndim=17)
    assert rc == UNSUPPORTED and b"between 1 and 16" in msg


def test_the_kernels_live_in_a_header_of_their_own():
    csrc = os.path.join(ROOT, "topolow_amd", "csrc")
    sources = glob.glob(os.path.join(csrc, "*.hip"))                 # exactly one source compiles the kernels
    assert sum('#include "relax_reduce.h"' in open(s).read() for s in sources) == 1
    assert '#include "relax_reduce.h"' in open(os.path.join(csrc, "topolow_reduce.hip")).read()
    text = open(os.path.join(csrc, "relax_reduce.h")).read()
    for kernel in ("scale_objective_partial_kernel", "scale_objective_combine_kernel"):
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, text), kernel
    code = re.sub(r"//[^\n]*", "", text)
    assert code.count("::sqrt(") == 2                                # two square roots per pair, written once
    assert "float" not in code                                       # everything is f64
    assert not re.search(r"\batomic\w*\s*\(", code)                  # no atomic of any kind
    assert "unsafeAtomicAdd" not in code and "__hip_atomic" not in code and "__atomic" not in code
    assert "asm" not in code
    make = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRC\s*=.*\btopolow_reduce\.hip\b", make, re.M)
