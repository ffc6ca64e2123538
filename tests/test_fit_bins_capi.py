"""The three entries of the fit's binned diagnostics without a device: declared, exported, where their kernels live, the
Python surface, and every TOPOLOW_ERR_BAD_ARGUMENT case that is found before any device call -- so this runs on a box
with or without a GPU."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

from topolow_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("topolow_layout_prep_fit_extent", "topolow_layout_prep_fit_hist2d", "topolow_layout_prep_fit_linear_bins")
BAD = _native.ERR_BAD_ARGUMENT
i64p = C.POINTER(C.c_int64)


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "topolow_relax.h")).read()
    for name, value in (("TOPOLOW_FIT_AXIS_TRUE", 0), ("TOPOLOW_FIT_AXIS_PREDICTED", 1), ("TOPOLOW_FIT_AXIS_ERROR", 2),
                        ("TOPOLOW_FIT_AXIS_RESIDUAL", 3), ("TOPOLOW_FIT_MAX_BINS", 8192), ("TOPOLOW_FIT_MAX_GRID", 4096)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
        assert getattr(_native, name[len("TOPOLOW_"):]) == value
    # the two deviations are stated where the entries are
    assert "masks the diagonal" in header and "at most 2^-32 of itself" in header
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _native.load()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name) and getattr(lib, name).restype is C.c_int, name
    assert [len(getattr(lib, name).argtypes) for name in SYMBOLS] == [10, 17, 16]
    for method in ("fit_extent", "fit_hist2d", "fit_linear_bins"):
        assert callable(getattr(_native.PreparedHandle, method))


def test_the_kernels_are_compiled_once_and_use_integer_atomics_only():
    csrc = os.path.join(ROOT, "topolow_amd", "csrc")
    sources = [s for s in glob.glob(os.path.join(csrc, "*.hip")) if '#include "relax_fit_bins.h"' in open(s).read()]
    assert [os.path.basename(s) for s in sources] == ["topolow_fit_bins.hip"]
    host = open(sources[0]).read()
    # ... which takes relax_fit.h's cell function without the report's kernels: those stay the fold source's alone
    assert host.index("#define TOPOLOW_FIT_CELL_ONLY") < host.index('#include "relax_fit_bins.h"')
    assert '#include "relax_fit.h"' not in host and '#include "relax_prep_fold.h"' not in host
    fit = open(os.path.join(csrc, "relax_fit.h")).read()
    guard = fit.index("#ifndef TOPOLOW_FIT_CELL_ONLY")
    assert fit.index("fit_block_reduce(T") < guard < fit.index("__global__") and "__global__" not in fit[fit.index("#endif"):]
    make = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRC\s*=.*\btopolow_fit_bins\.hip\b", make, re.M)
    text = open(os.path.join(csrc, "relax_fit_bins.h")).read()
    for kernel in ("bins_extent_kernel", "bins_hist2d_kernel", "bins_linear_kernel"):
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, text), kernel
    assert len(re.findall(r"= fit_cell\(", text)) == 3 and "post_distance" not in text and "sqrt" not in text
    code = re.sub(r"//[^\n]*", "", text)
    adds = [ln.strip() for ln in code.splitlines() if "atomic" in ln]
    assert len(adds) == 7 and all("atomicAdd(" in ln for ln in adds), adds
    for ln in adds:      # every one adds an unsigned integer: a counter of LDS or a 64-bit word of the zeroed buffer
        assert re.search(r"atomicAdd\(&(h|count|frac|out)\[[^\]]+\], (1u|g\.q|frac\[q\]|\(unsigned long long\)\w+\[\w+\])\)", ln), ln
    # the entries check their arguments with the fit report's function and mark through the report's path: both are
    # defined once, in the fold source, and no source but that one launches the marking kernel
    fold = open(os.path.join(csrc, "topolow_prep_fold.hip")).read()
    assert fold.count("int fit_check_arguments(") == 1 and fold.count("int fit_run(") == 1
    assert "int fit_check_arguments(" not in host and "int fit_run(" not in host and "fold_mark_kernel" not in host
    assert host.count("fit_check_arguments(entry, p, positions") == 3 and host.count("fit_run(p, positions") == 3
    assert host.count("fit_check_series(entry, series") == 3
    assert fold.count("fold_mark_kernel,") == 2           # the folds' and fit_run's, as before


def _err():
    return C.create_string_buffer(256)


def _args():
    mem = np.zeros(4096, dtype=np.int32)      # a stand-in handle: nothing of it may be read
    pos = np.zeros((4, 2), order="F")
    picks = np.zeros(3, dtype=np.int64)
    return mem, mem.ctypes.data_as(C.c_void_p), _native._dp(pos), picks.ctypes.data_as(i64p)


def _refused(fn, name, cases):
    for args, word in cases:
        err = _err()
        assert fn(*args, err, len(err)) == BAD, (args, err.value)
        assert word in err.value and name in err.value, err.value


def test_fit_extent_argument_errors():
    lib = _native.load()
    mem, h, posp, pkp = _args()
    out, m = np.full(8, 7.0), C.c_int64(-7)
    op, mp = _native._dp(out), C.byref(m)
    _refused(lib.topolow_layout_prep_fit_extent, b"topolow_layout_prep_fit_extent", (
        ((None, posp, 2, None, 0, 2, op, mp), b"NULL"),
        ((h, None, 2, None, 0, 2, op, mp), b"NULL"),
        ((h, posp, 2, None, 0, 2, None, mp), b"NULL"),
        ((h, posp, 2, None, 0, 2, op, None), b"NULL"),
        ((h, posp, 0, None, 0, 2, op, mp), b"ndim >= 1"),
        ((h, posp, 2, pkp, -1, 2, op, mp), b"n_picks >= 0"),
        ((h, posp, 2, None, 3, 2, op, mp), b"picks must not be NULL"),
        ((h, posp, 2, None, 0, 3, op, mp), b"unknown series 3"),
        ((h, posp, 2, None, 0, -1, op, mp), b"unknown series -1")))
    assert m.value == -7 and (out == 7.0).all() and not mem.any()


def test_fit_hist2d_argument_errors():
    lib = _native.load()
    mem, h, posp, pkp = _args()
    xe, ye = np.array([0.0, 1.0, 2.0, 4.0]), np.array([-1.0, 0.0, 1.0])
    big = np.arange(8194, dtype=np.float64)
    counts = np.full(8192, -3, dtype=np.int64)
    outside, m = C.c_int64(-7), C.c_int64(-7)
    xp, yp, bp, cp, op, mp = (_native._dp(xe), _native._dp(ye), _native._dp(big), counts.ctypes.data_as(i64p),
                              C.byref(outside), C.byref(m))

    def edges(values):
        a = np.array(values, dtype=np.float64)
        keep.append(a)
        return _native._dp(a)
    keep = []
    _refused(lib.topolow_layout_prep_fit_hist2d, b"topolow_layout_prep_fit_hist2d", (
        ((None, posp, 2, None, 0, 2, 0, xp, 3, 1, yp, 2, cp, op, mp), b"NULL"),
        ((h, None, 2, None, 0, 2, 0, xp, 3, 1, yp, 2, cp, op, mp), b"NULL"),
        ((h, posp, 2, None, 0, 2, 0, None, 3, 1, yp, 2, cp, op, mp), b"NULL"),
        ((h, posp, 2, None, 0, 2, 0, xp, 3, 1, None, 2, cp, op, mp), b"NULL"),
        ((h, posp, 2, None, 0, 2, 0, xp, 3, 1, yp, 2, None, op, mp), b"NULL"),
        ((h, posp, 2, None, 0, 2, 0, xp, 3, 1, yp, 2, cp, None, mp), b"NULL"),
        ((h, posp, 2, None, 0, 2, 0, xp, 3, 1, yp, 2, cp, op, None), b"NULL"),
        ((h, posp, 0, None, 0, 2, 0, xp, 3, 1, yp, 2, cp, op, mp), b"ndim >= 1"),
        ((h, posp, -1, None, 0, 2, 0, xp, 3, 1, yp, 2, cp, op, mp), b"ndim >= 1"),
        ((h, posp, 2, pkp, -1, 2, 0, xp, 3, 1, yp, 2, cp, op, mp), b"n_picks >= 0"),
        ((h, posp, 2, None, 2, 2, 0, xp, 3, 1, yp, 2, cp, op, mp), b"picks must not be NULL"),
        ((h, posp, 2, None, 0, 3, 0, xp, 3, 1, yp, 2, cp, op, mp), b"unknown series 3"),
        ((h, posp, 2, None, 0, 2, 4, xp, 3, 1, yp, 2, cp, op, mp), b"unknown x_axis 4"),
        ((h, posp, 2, None, 0, 2, 0, xp, 3, -1, yp, 2, cp, op, mp), b"unknown y_axis -1"),
        ((h, posp, 2, None, 0, 2, 0, xp, 0, 1, yp, 2, cp, op, mp), b"nx >= 1"),
        ((h, posp, 2, None, 0, 2, 0, xp, -2, 1, yp, 2, cp, op, mp), b"nx >= 1"),
        ((h, posp, 2, None, 0, 2, 0, xp, 3, 1, yp, 0, cp, op, mp), b"ny >= 1"),
        ((h, posp, 2, None, 0, 2, 0, bp, 8193, 1, yp, 1, cp, op, mp), b"nx * ny <= 8192"),
        ((h, posp, 2, None, 0, 2, 0, bp, 4097, 1, yp, 2, cp, op, mp), b"nx * ny <= 8192"),
        ((h, posp, 2, None, 0, 2, 0, bp, 65536, 1, bp, 65536, cp, op, mp), b"nx * ny <= 8192"),     # 2^32: no int overflow
        ((h, posp, 2, None, 0, 2, 0, edges([0.0, 1.0, 1.0, 2.0]), 3, 1, yp, 2, cp, op, mp), b"x_edges must be finite and strictly increasing (entry 2)"),
        ((h, posp, 2, None, 0, 2, 0, edges([0.0, 2.0, 1.0, 3.0]), 3, 1, yp, 2, cp, op, mp), b"x_edges must be finite and strictly increasing (entry 2)"),
        ((h, posp, 2, None, 0, 2, 0, edges([np.nan, 2.0, 3.0, 4.0]), 3, 1, yp, 2, cp, op, mp), b"x_edges must be finite and strictly increasing (entry 0)"),
        ((h, posp, 2, None, 0, 2, 0, xp, 3, 1, edges([0.0, 1.0, np.inf]), 2, cp, op, mp), b"y_edges must be finite and strictly increasing (entry 2)"),
        ((h, posp, 2, None, 0, 2, 0, xp, 3, 1, edges([-np.inf, 1.0, 2.0]), 2, cp, op, mp), b"y_edges must be finite and strictly increasing (entry 0)"),
        ((h, posp, 2, None, 0, 2, 0, xp, 3, 1, edges([0.0, 1.0, np.nan]), 2, cp, op, mp), b"y_edges must be finite and strictly increasing (entry 2)")))
    assert m.value == -7 and outside.value == -7 and (counts == -3).all() and not mem.any()


def test_fit_linear_bins_argument_errors():
    lib = _native.load()
    mem, h, posp, pkp = _args()
    count, frac = np.full(4096, -3, dtype=np.int64), np.full(4096, 5, dtype=np.uint64)
    outside, total = C.c_int64(-7), C.c_int64(-7)
    cp, fp, op, tp = count.ctypes.data_as(i64p), frac.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(outside), C.byref(total)
    _refused(lib.topolow_layout_prep_fit_linear_bins, b"topolow_layout_prep_fit_linear_bins", (
        ((None, posp, 2, None, 0, 2, 3, -1.0, 1.0, 512, cp, fp, op, tp), b"NULL"),
        ((h, None, 2, None, 0, 2, 3, -1.0, 1.0, 512, cp, fp, op, tp), b"NULL"),
        ((h, posp, 2, None, 0, 2, 3, -1.0, 1.0, 512, None, fp, op, tp), b"NULL"),
        ((h, posp, 2, None, 0, 2, 3, -1.0, 1.0, 512, cp, None, op, tp), b"NULL"),
        ((h, posp, 2, None, 0, 2, 3, -1.0, 1.0, 512, cp, fp, None, tp), b"NULL"),
        ((h, posp, 2, None, 0, 2, 3, -1.0, 1.0, 512, cp, fp, op, None), b"NULL"),
        ((h, posp, 0, None, 0, 2, 3, -1.0, 1.0, 512, cp, fp, op, tp), b"ndim >= 1"),
        ((h, posp, 2, pkp, -4, 2, 3, -1.0, 1.0, 512, cp, fp, op, tp), b"n_picks >= 0"),
        ((h, posp, 2, None, 1, 2, 3, -1.0, 1.0, 512, cp, fp, op, tp), b"picks must not be NULL"),
        ((h, posp, 2, None, 0, 5, 3, -1.0, 1.0, 512, cp, fp, op, tp), b"unknown series 5"),
        ((h, posp, 2, None, 0, 2, 4, -1.0, 1.0, 512, cp, fp, op, tp), b"unknown axis 4"),
        ((h, posp, 2, None, 0, 2, -1, -1.0, 1.0, 512, cp, fp, op, tp), b"unknown axis -1"),
        ((h, posp, 2, None, 0, 2, 3, -1.0, 1.0, 1, cp, fp, op, tp), b"2 <= m <= 4096"),
        ((h, posp, 2, None, 0, 2, 3, -1.0, 1.0, 0, cp, fp, op, tp), b"2 <= m <= 4096"),
        ((h, posp, 2, None, 0, 2, 3, -1.0, 1.0, 4097, cp, fp, op, tp), b"2 <= m <= 4096"),
        ((h, posp, 2, None, 0, 2, 3, 1.0, 1.0, 512, cp, fp, op, tp), b"lo < up"),
        ((h, posp, 2, None, 0, 2, 3, 2.0, 1.0, 512, cp, fp, op, tp), b"lo < up"),
        ((h, posp, 2, None, 0, 2, 3, float("nan"), 1.0, 512, cp, fp, op, tp), b"lo < up"),
        ((h, posp, 2, None, 0, 2, 3, -1.0, float("inf"), 512, cp, fp, op, tp), b"lo < up"),
        ((h, posp, 2, None, 0, 2, 3, -1.7e308, 1.7e308, 2, cp, fp, op, tp), b"must be finite and positive")))
    assert total.value == -7 and outside.value == -7 and (count == -3).all() and (frac == 5).all() and not mem.any()


def test_python_surface_checks_before_the_library():
    class Stub(_native.PreparedHandle):
        def __init__(self):
            self.n = 4
    pos = np.zeros((4, 2))
    with pytest.raises(ValueError, match="one row per point"):
        Stub().fit_extent(np.zeros((3, 2)), "all")
    with pytest.raises(ValueError, match="series"):
        Stub().fit_extent(pos, "both")
    with pytest.raises(ValueError, match="axis"):
        Stub().fit_hist2d(pos, "all", "truth", [0, 1], "error", [0, 1])
    with pytest.raises(ValueError, match="axis"):
        Stub().fit_linear_bins(pos, "in", 7, 0.0, 1.0)
