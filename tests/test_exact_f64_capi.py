"""precision = "f64_exact" at the call boundary, without a GPU: the name, the header's constant, and -- on a machine
without a device -- that the entry gets as far as looking for one (TOPOLOW_ERR_NO_DEVICE, not a bad argument)."""
import os
import re

import numpy as np
import pytest

from topolow_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_the_name_and_the_header_constant_agree():
    assert _native._PRECISIONS["f64_exact"] == 3 == _native.PRECISION_F64_EXACT
    assert _native._PRECISION_NAMES[3] == "f64_exact" and _native._PRECISION_NAMES[2] == "f64"
    header = open(os.path.join(ROOT, "include", "topolow_relax.h")).read()
    assert int(re.search(r"^#define TOPOLOW_PRECISION_F64_EXACT (\d+)", header, re.M).group(1)) == 3
    for name, value in (("AUTO", 0), ("F32", 1), ("F64", 2)):       # the existing values did not move
        assert int(re.search(r"^#define TOPOLOW_PRECISION_%s (\d+)" % name, header, re.M).group(1)) == value
    shim = open(os.path.join(ROOT, "topolow_amd", "r", "topolow_shim.c")).read()
    assert '"f64_exact"' in shim and "TOPOLOW_PRECISION_F64_EXACT" in shim


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device error path")
def test_exact_precision_reaches_the_device_lookup():
    D = np.array([[np.inf, 1.0], [1.0, np.inf]])
    T = np.zeros((2, 2), np.int32)
    for schedule in ("auto", "slab", "gs"):
        with pytest.raises(_native.NativeError) as ei:
            _native.optimize_layout_exact_arrays(np.zeros((2, 2)), D, T, [1, 1], [0], [1], [1.0], [0], 5, 1.0, 0.1, 0.1,
                                                 1e-4, 5, 3, seed=1, schedule=schedule, precision="f64_exact")
        assert ei.value.code == _native.ERR_NO_DEVICE
    with pytest.raises(_native.NativeError) as ei:
        _native.Session(10, 3, precision="f64_exact")
    assert ei.value.code == _native.ERR_NO_DEVICE
