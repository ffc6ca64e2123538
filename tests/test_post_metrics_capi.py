"""topolow_post_metrics without a device: the symbol, its argument errors, the wrapper's NaN, and the R shim's
routine `_topolow_post_metrics` compiled against the test double of R's C API (tests/fake_r/post_harness.c)."""
import ctypes as C
import math
import os
import re
import warnings

import numpy as np
import pytest

from tests import post_metrics_helpers as pm
from topolow_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "topolow_relax.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+topolow_post_metrics\s*\(", header)
    lib = _native.load()
    assert hasattr(lib, "topolow_post_metrics") and hasattr(lib, "topolow_post_metrics_ex")


def test_argument_errors_come_before_any_device_call():
    """NULL positions, values, sum_abs or count, n < 1, ndim < 1: TOPOLOW_ERR_BAD_ARGUMENT whether or not a device
    is present (a valid call on a box without one answers TOPOLOW_ERR_NO_DEVICE instead)."""
    lib = _native.load()
    p = np.zeros((3, 2), order="F")
    v = np.zeros((3, 3), order="F")
    s, c = C.c_double(0.0), C.c_int64(0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    err = C.create_string_buffer(256)

    def call(pos=dp(p), n=3, ndim=2, values=dp(v), sum_abs=C.byref(s), count=C.byref(c)):
        return lib.topolow_post_metrics(pos, n, ndim, values, None, None, sum_abs, count, -1, err, len(err))

    assert call(pos=None) == _native.ERR_BAD_ARGUMENT
    assert call(values=None) == _native.ERR_BAD_ARGUMENT
    assert call(sum_abs=None) == _native.ERR_BAD_ARGUMENT
    assert call(count=None) == _native.ERR_BAD_ARGUMENT
    assert call(n=0) == _native.ERR_BAD_ARGUMENT
    assert call(ndim=0) == _native.ERR_BAD_ARGUMENT
    with pytest.raises(ValueError):
        _native.post_metrics(p, np.zeros((4, 4)))


def test_no_counting_cell_is_nan_without_a_warning():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert math.isnan(_native.mae_of(0.0, 0))
        assert _native.mae_of(3.0, 2) == 1.5


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return pm.build_harness(tmp_path_factory.mktemp("rpost"))


def test_shim_registers_the_routine_and_raises_r_errors_balanced(harness, tmp_path):
    """Registered with arity 4 (the harness looks it up by name and arity); positions and values of different n
    become an R error with the protect stack balanced, before the library is called."""
    p = np.zeros((3, 2))
    out = pm.run_harness(harness, tmp_path, p, np.zeros((4, 4)), None, True)
    assert out["registration"] == "ok"
    assert out["error"] == "values must be a numeric n x n matrix with one row per position"
    assert out["protect_depth"] == 0
    out = pm.run_harness(harness, tmp_path, p, np.zeros((3, 3)), np.zeros((4, 4), np.int32), False)
    assert out["error"] == "codes must be NULL or an integer n x n matrix" and out["protect_depth"] == 0
