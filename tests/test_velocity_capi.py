"""topolow_kernel_velocity and its _ex twin without a device: declared, exported, ctypes signatures, every
TOPOLOW_ERR_BAD_ARGUMENT case (found before any device call, so this runs with or without a GPU), and where the
kernels live."""
import ctypes as C
import glob
import math
import os
import re

import numpy as np
import pytest

from topolow_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("topolow_kernel_velocity", "topolow_kernel_velocity_ex")


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "topolow_relax.h")).read()
    assert "between about 700 and 760" in header                 # the one-exp deviation is stated where the entry is
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _native.load()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name


def test_ctypes_signatures_and_the_python_surface():
    lib = _native.load()
    dp, u64p = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    head = [dp, dp, C.c_int32, C.c_int32, C.c_double, C.c_double, u64p, dp, dp, C.c_int32]
    assert lib.topolow_kernel_velocity.argtypes == head + [C.c_char_p, C.c_size_t]
    assert lib.topolow_kernel_velocity_ex.argtypes == head + [C.c_int32, dp, C.c_char_p, C.c_size_t]
    for name in SYMBOLS:
        assert getattr(lib, name).restype is C.c_int
    assert callable(_native.kernel_velocity)
    with pytest.raises(ValueError):
        _native.kernel_velocity(np.zeros((4, 2)), np.zeros(3), 1.0, 1.0)
    with pytest.raises(ValueError):
        _native.kernel_velocity(np.zeros((4, 2)), np.zeros(4), 1.0, 1.0, excluded_bits=np.zeros((4, 2), np.uint64))


def _call(lib, ex, **kw):
    pos = np.zeros((3, 2), order="F")
    t = np.arange(3.0)
    out, w = np.full((3, 2), -7.0, order="F"), np.full(3, -7.0)
    a = dict(positions=_native._dp(pos), times=_native._dp(t), n=3, ndim=2, sigma_t=1.0, sigma_x=1.0, bits=None,
             velocity=_native._dp(out), weight_sum=_native._dp(w), chunk=0)
    a.update(kw)
    err = C.create_string_buffer(256)
    head = (a["positions"], a["times"], a["n"], a["ndim"], a["sigma_t"], a["sigma_x"], a["bits"], a["velocity"],
            a["weight_sum"], -1)
    if ex:
        rc = lib.topolow_kernel_velocity_ex(*head, a["chunk"], None, err, len(err))
    else:
        rc = lib.topolow_kernel_velocity(*head, err, len(err))
    assert (out == -7.0).all() and (w == -7.0).all()             # nothing was written
    return rc, err.value


@pytest.mark.parametrize("ex", [False, True])
def test_argument_errors_come_before_any_device_call(ex):
    lib = _native.load()
    bad = _native.ERR_BAD_ARGUMENT
    cases = [dict(positions=None), dict(times=None), dict(velocity=None), dict(n=0), dict(n=-2), dict(ndim=0),
             dict(ndim=-1)]
    for sigma in ("sigma_t", "sigma_x"):
        cases += [{sigma: v} for v in (0.0, -1.0, math.inf, -math.inf, math.nan)]
    for kw in cases:
        rc, msg = _call(lib, ex, **kw)
        assert rc == bad and b"topolow_kernel_velocity" in msg, (kw, rc, msg)
    rc, msg = _call(lib, ex, ndim=17)
    assert rc == _native.ERR_UNSUPPORTED and b"between 1 and 16" in msg
    if ex:
        for chunk in (-64, 1, 63, 100):
            rc, msg = _call(lib, True, chunk=chunk)
            assert rc == bad and b"multiple of 64" in msg, chunk


def test_the_kernels_live_in_a_header_of_their_own():
    csrc = os.path.join(ROOT, "topolow_amd", "csrc")
    sources = glob.glob(os.path.join(csrc, "*.hip"))               # exactly one source compiles the kernels
    assert sum('#include "relax_velocity.h"' in open(s).read() for s in sources) == 1
    text = open(os.path.join(csrc, "relax_velocity.h")).read()
    for kernel in ("velocity_partial_kernel", "velocity_combine_kernel"):
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, text), kernel
    assert "between about 700 and 760" in text                     # the header comment states the one-exp deviation
    code = re.sub(r"//[^\n]*", "", text)
    assert code.count("::exp(") == 1                               # one exp per pair, written once
    # no floating-point atomic: the only atomic is the integer maximum of a workgroup's prefix lengths, in LDS
    atomics = re.findall(r"\batomic\w*\s*\(([^;]*);", code)
    assert len(atomics) == 1 and atomics[0].startswith("&block_past"), atomics
    assert re.search(r"__shared__ int block_past;", code)
    assert "unsafeAtomicAdd" not in code and "__hip_atomic" not in code and "__atomic" not in code
    make = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRC\s*=.*\btopolow_velocity\.hip\b", make, re.M)
