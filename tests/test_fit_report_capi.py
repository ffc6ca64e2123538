"""The two fit-report entries without a device: declared, exported, ctypes signatures, the Python surface, where the
kernels live, and every TOPOLOW_ERR_BAD_ARGUMENT case that is found before any device call -- so this runs on a box
with or without a GPU."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

from topolow_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("topolow_layout_prep_fit_report", "topolow_layout_prep_fit_order_stats")
BAD = _native.ERR_BAD_ARGUMENT


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "topolow_relax.h")).read()
    assert "typedef struct topolow_fit_report" in header and "typedef struct topolow_fit_series" in header
    for name, value in (("TOPOLOW_FIT_IN", 0), ("TOPOLOW_FIT_OUT", 1), ("TOPOLOW_FIT_ALL", 2), ("TOPOLOW_FIT_MAX_RANKS", 8)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert (_native.FIT_IN, _native.FIT_OUT, _native.FIT_ALL, _native.FIT_MAX_RANKS) == (0, 1, 2, 8)
    assert "+-Inf cells are left out" in header                              # the deviation is stated where the entry is
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _native.load()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name


def test_ctypes_signatures_and_the_python_surface():
    lib = _native.load()
    assert len(lib.topolow_layout_prep_fit_report.argtypes) == 8
    assert len(lib.topolow_layout_prep_fit_order_stats.argtypes) == 12
    for name in SYMBOLS:
        assert getattr(lib, name).restype is C.c_int
    assert callable(_native.PreparedHandle.fit_report) and callable(_native.PreparedHandle.fit_order_stats)
    # per series: count, 4 error words, pct_count, 2 percentage sums, sum_v, sum_r, 4 centred sums
    assert C.sizeof(_native.TopolowFitSeries) == 14 * 8
    # three series, three times, four reserved words
    assert C.sizeof(_native.TopolowFitReport) == 3 * 14 * 8 + 3 * 8 + 4 * 8
    header = open(os.path.join(ROOT, "include", "topolow_relax.h")).read()
    body = header[header.index("typedef struct topolow_fit_series {"):header.index("} topolow_fit_series;")]
    for field, _ in _native.TopolowFitSeries._fields_:                       # every field is there, and documented
        line = [ln for ln in body.splitlines() if re.search(r"\b%s\b" % field, ln.split("/*")[0])]
        assert len(line) == 1 and "/*" in line[0], field


def test_the_kernels_live_in_a_header_of_their_own():
    csrc = os.path.join(ROOT, "topolow_amd", "csrc")
    sources = glob.glob(os.path.join(csrc, "*.hip"))   # exactly one source compiles the kernels
    assert sum('#include "relax_fit.h"' in open(s).read() for s in sources) == 1
    text = open(os.path.join(csrc, "relax_fit.h")).read()
    for kernel in ("fit_sums_kernel", "fit_centred_kernel", "fit_select_kernel"):
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, text), kernel
    assert "atomicAdd(" in text                        # the histograms
    for line in text.splitlines():                      # ... and nothing else: no floating-point atomic anywhere
        if "atomicAdd(" in line:
            assert "h[" in line or "hist[" in line, line
    # one cell function, called by all three kernels; the distance's arithmetic is written once, in relax_common.h,
    # and the two post-metrics kernels call it as well
    assert len(re.findall(r"= fit_cell\(", text)) == 3
    common = open(os.path.join(csrc, "relax_common.h")).read()
    post = open(os.path.join(csrc, "relax_post.h")).read()
    assert "sqrt" not in text and text.count("post_distance(") == 1
    assert common.count("s += dev * dev;") == 1 and common.count("post_distance(") == 1
    assert post.count("post_distance(") == 2


def _err():
    return C.create_string_buffer(256)


def _args():
    mem = np.zeros(4096, dtype=np.int32)      # a stand-in handle: nothing of it may be read
    pos = np.zeros((4, 2), order="F")
    picks = np.zeros(3, dtype=np.int64)
    return mem, mem.ctypes.data_as(C.c_void_p), _native._dp(pos), pos, picks, picks.ctypes.data_as(C.POINTER(C.c_int64))


def test_fit_report_argument_errors():
    lib = _native.load()
    mem, handle, posp, pos, picks, pkp = _args()
    rep = _native.TopolowFitReport()
    out = C.byref(rep)
    for args, word in (((None, posp, 2, None, 0, out), b"NULL"),
                       ((handle, None, 2, None, 0, out), b"NULL"),
                       ((handle, posp, 2, None, 0, None), b"NULL"),
                       ((handle, posp, 0, None, 0, out), b"ndim >= 1"),
                       ((handle, posp, -3, None, 0, out), b"ndim >= 1"),
                       ((handle, posp, 2, pkp, -1, out), b"n_picks >= 0"),
                       ((handle, posp, 2, None, 3, out), b"picks must not be NULL")):
        err = _err()
        assert lib.topolow_layout_prep_fit_report(*args, err, len(err)) == BAD
        assert word in err.value and b"topolow_layout_prep_fit_report" in err.value, err.value


def test_fit_order_stats_argument_errors():
    lib = _native.load()
    mem, handle, posp, pos, picks, pkp = _args()
    ranks = np.array([0, 1], dtype=np.int64)
    rkp = ranks.ctypes.data_as(C.POINTER(C.c_int64))
    vals, m = np.zeros(8), C.c_int64(-7)
    vp, mp = _native._dp(vals), C.byref(m)
    for args, word in (((None, posp, 2, None, 0, 0, rkp, 2, vp, mp), b"NULL"),
                       ((handle, None, 2, None, 0, 0, rkp, 2, vp, mp), b"NULL"),
                       ((handle, posp, 2, None, 0, 0, None, 2, vp, mp), b"NULL"),
                       ((handle, posp, 2, None, 0, 0, rkp, 2, None, mp), b"NULL"),
                       ((handle, posp, 2, None, 0, 0, rkp, 2, vp, None), b"NULL"),
                       ((handle, posp, 0, None, 0, 0, rkp, 2, vp, mp), b"ndim >= 1"),
                       ((handle, posp, 2, pkp, -2, 0, rkp, 2, vp, mp), b"n_picks >= 0"),
                       ((handle, posp, 2, None, 1, 0, rkp, 2, vp, mp), b"picks must not be NULL"),
                       ((handle, posp, 2, None, 0, 3, rkp, 2, vp, mp), b"unknown series 3"),
                       ((handle, posp, 2, None, 0, -1, rkp, 2, vp, mp), b"unknown series -1"),
                       ((handle, posp, 2, None, 0, 2, rkp, 0, vp, mp), b"1 <= n_ranks <= 8"),
                       ((handle, posp, 2, None, 0, 2, rkp, 9, vp, mp), b"1 <= n_ranks <= 8")):
        err = _err()
        assert lib.topolow_layout_prep_fit_order_stats(*args, err, len(err)) == BAD
        assert word in err.value and b"topolow_layout_prep_fit_order_stats" in err.value, err.value
    for bad_rank in (-1 - 1000001, -1 - (_native.FIT_RANK_UPPER - 1), -1 - (_native.FIT_RANK_UPPER + 1000001)):
        ranks[1] = bad_rank
        err = _err()
        assert lib.topolow_layout_prep_fit_order_stats(handle, posp, 2, None, 0, 0, rkp, 2, vp, mp, err, len(err)) == BAD
        assert b"rank 1" in err.value and b"0 .. 1000000" in err.value, err.value
    assert m.value == -7 and not vals.any() and not mem.any()


def test_python_surface_checks_before_the_library():
    class Stub(_native.PreparedHandle):
        def __init__(self):
            self.n = 4
    with pytest.raises(ValueError, match="one row per point"):
        Stub().fit_report(np.zeros((3, 2)))
    with pytest.raises(ValueError, match="series"):
        Stub().fit_order_stats(np.zeros((4, 2)), "both", [0])
