"""The prepared-layout C ABI without a device: the symbols, the info struct, the argument errors, and the ordering
rule (topolow_layout_order_from_sums) against core.spectral_order on sums computed with NumPy."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import prepare_layout_helpers as ph
from topolow_amd import _native, core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("topolow_layout_prep_create", "topolow_layout_prep_fetch", "topolow_layout_prep_destroy",
           "topolow_layout_order_from_sums")


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "topolow_relax.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _native.load()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name


def test_info_struct_size_matches_the_header(tmp_path):
    """72 bytes: four int64, one double, eight int32 -- in the ctypes twin and in the header as a C compiler reads it."""
    assert C.sizeof(_native.TopolowLayoutPrepInfo) == 72
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "topolow_relax.h"\n'
                   'int main(void) { printf("%zu %zu\\n", sizeof(topolow_layout_prep_info), '
                   '(size_t)&((topolow_layout_prep_info*)0)->order_route); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True,
                   capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["72", str(_native.TopolowLayoutPrepInfo.order_route.offset)]


def test_argument_errors_come_before_any_device_call():
    """NULL out, values or info, n < 2, an order_in that is no permutation: TOPOLOW_ERR_BAD_ARGUMENT whether or not a
    device is present (a valid call on a box without one answers TOPOLOW_ERR_NO_DEVICE instead)."""
    lib = _native.load()
    v = np.zeros((3, 3))
    info = _native.TopolowLayoutPrepInfo()
    handle = C.c_void_p()
    err = C.create_string_buffer(256)
    dp = v.ctypes.data_as(C.POINTER(C.c_double))

    def create(out=C.byref(handle), values=dp, n=3, info_=C.byref(info), order_in=None):
        return lib.topolow_layout_prep_create(out, values, None, n, 1, 0, order_in, -1, info_, err, len(err))

    assert create(out=None) == _native.ERR_BAD_ARGUMENT
    assert create(values=None) == _native.ERR_BAD_ARGUMENT
    assert create(info_=None) == _native.ERR_BAD_ARGUMENT
    assert create(n=1) == _native.ERR_BAD_ARGUMENT
    assert create(n=0) == _native.ERR_BAD_ARGUMENT
    bad = np.array([0, 0, 2], dtype=np.int32)
    assert create(order_in=bad.ctypes.data_as(C.POINTER(C.c_int32))) == _native.ERR_BAD_ARGUMENT
    assert b"permutation" in err.value
    assert handle.value is None
    assert lib.topolow_layout_prep_fetch(None, None, None, None, None, None, None, None, None, None, None, err,
                                         len(err)) == _native.ERR_BAD_ARGUMENT
    lib.topolow_layout_prep_destroy(None)   # a no-op
    with pytest.raises(ValueError):
        _native.prepare_layout(np.zeros((3, 4)))


def _route_and_order(D):
    values = D.values if isinstance(D, core.CodedMatrix) else D
    return _native.order_from_sums(*ph.numpy_sums(values), ph.sums_flag(values))


@pytest.mark.parametrize("n,dim,missing,seed", ph.SYNTHETIC)
def test_gap_rule_orders_the_synthetic_problems_as_numpy_does(n, dim, missing, seed):
    """Smallest neighbouring key gaps of these five: 7.2e-4 .. 5.7e-8 relative, against the rule's 8 n 2^-53
    (1.8e-12 at n = 2049): none may be declined."""
    D = ph.synthetic_matrix(n, dim, missing, seed)
    assert ph.sums_flag(D) == 0
    route, order = _route_and_order(D)
    assert route == _native.ORDER_DEVICE_GAP
    assert np.array_equal(order, core.spectral_order(D))


def test_exact_sums_keep_numpys_ties():
    D = ph.tied_integers()
    ref = core.spectral_order(D)
    keys = np.nanmean(np.where(np.eye(len(D), dtype=bool), np.nan, D), axis=1)
    assert len(np.unique(keys)) < len(D) // 2          # many tied keys
    assert ph.sums_flag(D) == 1
    route, order = _route_and_order(D)
    assert route == _native.ORDER_DEVICE_EXACT
    assert np.array_equal(order, ref)
    # the same sums without the promise of exactness: ties cannot be told from near-ties
    assert _native.order_from_sums(*ph.numpy_sums(D), 0)[0] == _native.ORDER_DECLINED


def test_near_tie_and_negative_cell_are_declined():
    D = ph.same_values_other_columns()
    assert ph.sums_flag(D) == 0
    assert _route_and_order(D) == (_native.ORDER_DECLINED, None)
    D = ph.one_negative()
    assert ph.sums_flag(D) == -1
    assert _route_and_order(D) == (_native.ORDER_DECLINED, None)
    D = ph.synthetic_matrix(33, 2, 0.3, 1).copy()
    D[4, 9] = np.inf
    assert ph.sums_flag(D) == -1
    assert _route_and_order(D)[0] == _native.ORDER_DECLINED


def test_at_most_one_positive_key_keeps_the_input_order():
    for D in (ph.single_positive_key(), ph.no_positive_key()):
        assert core.spectral_order(D) is None
        route, order = _route_and_order(D)
        assert route in (_native.ORDER_DEVICE_EXACT, _native.ORDER_DEVICE_GAP) and order is None
    s = ph.numpy_sums(ph.single_positive_key())
    assert _native.order_from_sums(*s, 0) == (_native.ORDER_DEVICE_GAP, None)


def test_a_point_without_measurements_has_key_zero():
    D = ph.unmeasured_point(40, 7)
    route, order = _route_and_order(D)
    assert route == _native.ORDER_DEVICE_GAP
    assert order[0] == 7
    assert np.array_equal(order, core.spectral_order(D))


def test_the_environment_forces_the_choice_per_call(monkeypatch):
    D = np.zeros((8, 8))
    monkeypatch.setenv("TOPOLOW_DEVICE_PREP", "1")
    assert core._device_prep_wanted(D)
    monkeypatch.setenv("TOPOLOW_DEVICE_PREP", "0")
    assert not core._device_prep_wanted(D)
    monkeypatch.delenv("TOPOLOW_DEVICE_PREP")
    monkeypatch.setattr(core, "_DEVICE_PREP_MIN_N", 8)
    assert core._device_prep_wanted(D) and core._device_prep_wanted(core.RMatrix(D))
    assert not core._device_prep_wanted(D[:7, :7])
    monkeypatch.setattr(core, "_DEVICE_PREP_MIN_N", None)
    assert not core._device_prep_wanted(D)
