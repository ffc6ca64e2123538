"""The three spectrum entries without a device: declared, exported, ctypes signatures, the Python surface, and every
TOPOLOW_ERR_BAD_ARGUMENT case -- each found before any device call, so this runs on a box with or without a GPU."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

from topolow_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("topolow_tridiagonal_eigenvalues", "topolow_symmetric_eigenvalues", "topolow_layout_prep_spectrum")
BAD = _native.ERR_BAD_ARGUMENT


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "topolow_relax.h")).read()
    assert "typedef struct topolow_spectrum_info" in header
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _native.load()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name


def test_ctypes_signatures_and_the_python_surface():
    lib = _native.load()
    assert len(lib.topolow_tridiagonal_eigenvalues.argtypes) == 7
    assert len(lib.topolow_symmetric_eigenvalues.argtypes) == 8
    assert len(lib.topolow_layout_prep_spectrum.argtypes) == 6
    for name in SYMBOLS:
        assert getattr(lib, name).restype is C.c_int
    assert callable(_native.tridiagonal_eigenvalues) and callable(_native.symmetric_eigenvalues)
    assert callable(_native.PreparedHandle.spectrum)
    # median .. dims_90 + reserved32, four phase times, four reserved words
    assert C.sizeof(_native.TopolowSpectrumInfo) == 9 * 8 + 2 * 4 + 4 * 8 + 4 * 8


def test_the_kernels_live_in_a_header_of_their_own():
    csrc = os.path.join(ROOT, "topolow_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "relax_spectrum.h"))
    sources = glob.glob(os.path.join(csrc, "*.hip"))   # exactly one source compiles the kernels
    assert sum('#include "relax_spectrum.h"' in open(s).read() for s in sources) == 1
    text = open(os.path.join(csrc, "relax_spectrum.h")).read()
    assert "atomicAdd(" in text                        # the histograms
    for line in text.splitlines():                      # ... and nothing else: no floating-point atomic anywhere
        if "atomicAdd(" in line:
            assert "h[" in line or "hist[" in line, line
    assert "solver" not in open(os.path.join(csrc, "Makefile")).read().lower()


def _err():
    return C.create_string_buffer(256)


def test_tridiagonal_argument_errors():
    lib = _native.load()
    d, e, out = np.array([1.0, 2.0, 3.0]), np.array([0.5, 0.5]), np.zeros(3)
    dp = _native._dp
    for args, word in (((None, dp(e), 3, -1, dp(out)), b"NULL"),
                       ((dp(d), dp(e), 3, -1, None), b"NULL"),
                       ((dp(d), None, 3, -1, dp(out)), b"NULL"),
                       ((dp(d), dp(e), 0, -1, dp(out)), b"n >= 1"),
                       ((dp(d), dp(e), -4, -1, dp(out)), b"n >= 1")):
        err = _err()
        assert lib.topolow_tridiagonal_eigenvalues(*args, err, len(err)) == BAD
        assert word in err.value, err.value
    for bad_d, bad_e in ((np.array([1.0, np.nan, 3.0]), e), (d, np.array([0.5, np.inf])), (np.array([-np.inf, 0, 0]), e)):
        err = _err()
        assert lib.topolow_tridiagonal_eigenvalues(dp(bad_d), dp(bad_e), 3, -1, dp(out), err, len(err)) == BAD
        assert b"infinite or missing" in err.value
    with pytest.raises(ValueError, match="n - 1 entries"):
        _native.tridiagonal_eigenvalues(d, [0.5])


def test_symmetric_argument_errors():
    lib = _native.load()
    a = np.asfortranarray(np.eye(3))
    out = np.zeros(3)
    dp = _native._dp
    for args, word in (((None, 3, -1, None, None, dp(out)), b"NULL"),
                       ((dp(a), 0, -1, None, None, dp(out)), b"n >= 1"),
                       ((dp(a), -1, -1, None, None, dp(out)), b"n >= 1")):
        err = _err()
        assert lib.topolow_symmetric_eigenvalues(*args, err, len(err)) == BAD
        assert word in err.value, err.value
    for r, c, v in ((2, 0, np.nan), (1, 1, np.inf), (2, 2, -np.inf)):      # cells of the lower triangle
        b = np.asfortranarray(np.eye(3))
        b[r, c] = v
        err = _err()
        assert lib.topolow_symmetric_eigenvalues(dp(b), 3, -1, None, None, dp(out), err, len(err)) == BAD
        assert b"infinite or missing values in 'x'" in err.value
    with pytest.raises(ValueError, match="n x n"):
        _native.symmetric_eigenvalues(np.zeros((3, 2)))


def test_spectrum_argument_errors():
    lib = _native.load()
    mem = np.zeros(4096, dtype=np.int32)      # a stand-in handle: nothing of it may be read
    handle = mem.ctypes.data_as(C.c_void_p)
    info = _native.TopolowSpectrumInfo()
    for h, i in ((None, C.byref(info)), (handle, None), (None, None)):
        err = _err()
        assert lib.topolow_layout_prep_spectrum(h, None, None, i, err, len(err)) == BAD
        assert b"NULL" in err.value
