"""The pre-processing on the device (topolow_layout_prep_*, core.prepare_layout_call_device) against its host mirror
core.prepare_layout_call: every field of the LayoutCall, bit for bit."""
import numpy as np
import pytest

import topolow_amd
from tests import prepare_layout_helpers as ph
from topolow_amd import _native, core

pytestmark = pytest.mark.gpu

PARAMS = dict(ndim=3, mapping_max_iter=50, k0=5.0, cooling_rate=0.01, c_repulsion=0.01, relative_epsilon=1e-4,
              convergence_counter=5, initial_positions=None, verbose=True, convergence_check_freq=3)
ARRAYS = ("initial_positions", "dissimilarity_matrix", "threshold_matrix", "degrees", "edge_i", "edge_j", "edge_dist",
          "edge_thresh")
SCALARS = ("n_iter", "k0", "cooling_rate", "c_repulsion", "relative_epsilon", "convergence_window",
           "convergence_check_freq", "verbose", "names")


@pytest.fixture(autouse=True)
def _device_prep(monkeypatch):
    monkeypatch.setenv("TOPOLOW_DEVICE_PREP", "1")


def _both(D, capsys, preserve_order=False, **over):
    kw = dict(PARAMS, **over)
    host = core.prepare_layout_call(D, preserve_order=preserve_order, rng=np.random.default_rng(5), **kw)
    host_lines = capsys.readouterr().out
    route = []
    dev = core.prepare_layout_call_device(D, preserve_order=preserve_order, rng=np.random.default_rng(5), route=route,
                                          **kw)
    dev_lines = capsys.readouterr().out
    assert dev_lines == host_lines
    return host, dev, route[0]


def _same(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and \
        np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()


def _assert_field_for_field(host, dev):
    for f in ARRAYS:
        assert _same(getattr(host, f), getattr(dev, f)), f
        assert getattr(host, f).flags.c_contiguous and getattr(dev, f).flags.c_contiguous, f
    for f in SCALARS:
        assert getattr(host, f) == getattr(dev, f), f
    assert (host.order is None) == (dev.order is None)
    if host.order is not None:
        assert np.array_equal(host.order, dev.order)
    hm, dm = host.reordered_matrix, dev.reordered_matrix
    assert _same(hm.values, dm.values) and _same(hm.codes, dm.codes)
    assert hm.values.flags.c_contiguous == dm.values.flags.c_contiguous
    assert hm.codes.flags.c_contiguous == dm.codes.flags.c_contiguous
    assert hm.names == dm.names and hm.character == dm.character
    assert _same(hm.as_numeric(), dm.as_numeric())


def _host_rule(D):
    """The route the rule gives on NumPy's sums (checked without a device in test_prepare_layout_capi.py)."""
    return _native.order_from_sums(*ph.numpy_sums(D), ph.sums_flag(D))[0]


@pytest.mark.parametrize("n", [2, 5, 63, 64, 65, 129, 1000])
def test_sizes_around_the_tile(n, capsys):
    D = ph.synthetic_matrix(n, 3, 0.3 if n > 5 else 0.0, 100 + n)
    host, dev, route = _both(D, capsys)
    assert route == _host_rule(D)
    if n == 2:
        assert route == _native.ORDER_DECLINED    # two points share their one distance: a tie of inexact keys
    _assert_field_for_field(host, dev)


@pytest.mark.parametrize("n,dim,missing,seed", ph.SYNTHETIC)
def test_synthetic_problems_are_ordered_on_the_device(n, dim, missing, seed, capsys):
    host, dev, route = _both(ph.synthetic_matrix(n, dim, missing, seed), capsys)
    assert route == _native.ORDER_DEVICE_GAP
    assert host.order is not None
    _assert_field_for_field(host, dev)


@pytest.mark.parametrize("case,expected", [
    ("asymmetric_na", _native.ORDER_DEVICE_GAP), ("with_codes", _native.ORDER_DEVICE_GAP),
    ("unmeasured_point", _native.ORDER_DEVICE_GAP), ("tied_integers", _native.ORDER_DEVICE_EXACT),
    ("same_values_other_columns", _native.ORDER_DECLINED), ("one_negative", _native.ORDER_DECLINED),
    ("single_positive_key", _native.ORDER_DEVICE_EXACT), ("quickstart", None)])
def test_named_cases(case, expected, capsys):
    D = getattr(ph, case)()
    host, dev, route = _both(D, capsys)
    if expected is None:   # the quick-start matrix: symmetric points share keys, whichever way the rule answers
        expected = _host_rule(D)
    assert route == expected
    _assert_field_for_field(host, dev)
    if case == "unmeasured_point":
        assert dev.degrees[0] == 0 and dev.order[0] == 7
    if case == "with_codes":
        assert (dev.edge_thresh == 1).any() and (dev.edge_thresh == -1).any()
    if case == "single_positive_key":
        assert dev.order is None


def test_preserve_order_and_given_positions(capsys):
    D = ph.synthetic_matrix(65, 3, 0.5, 2)
    host, dev, route = _both(D, capsys, preserve_order=True)
    assert route == _native.ORDER_PRESERVED and dev.order is None
    _assert_field_for_field(host, dev)
    init = core.RMatrix(np.random.default_rng(1).normal(size=(65, 3)), ["s%d" % q for q in range(65)])
    named = core.RMatrix(D, ["s%d" % q for q in range(65)])
    host, dev, route = _both(named, capsys, initial_positions=init)
    assert route == _native.ORDER_DEVICE_GAP
    _assert_field_for_field(host, dev)


def test_no_measurement_is_the_references_error(capsys):
    D = np.full((6, 6), np.nan)
    np.fill_diagonal(D, 0.0)
    for fn in (core.prepare_layout_call, core.prepare_layout_call_device):
        with pytest.warns(UserWarning, match="No finite non-zero"):
            with pytest.raises(ValueError, match="No valid off-diagonal measurements"):
                fn(D, preserve_order=False, **PARAMS)


def _outputs(p):
    return {f: getattr(p, f) for f in ("order", "degrees", "edge_i", "edge_j", "edge_dist", "edge_thresh", "dense",
                                       "tdense", "values_reordered", "codes_reordered")}


def _assert_same_outputs(a, b, skip=()):
    assert a.info.keys() == b.info.keys()
    for k, x in a.info.items():
        y = b.info[k]
        assert x == y or (k == "numeric_max" and np.isnan(x) and np.isnan(y)), k
    for f, x in _outputs(a).items():
        if f in skip:
            continue
        y = getattr(b, f)
        assert (x is None) == (y is None), f
        if x is not None:
            assert np.array_equal(x, y, equal_nan=(x.dtype.kind == "f")) and x.dtype == y.dtype, f


@pytest.mark.parametrize("case", ["asymmetric_na", "with_codes"])
def test_transposed_reading(case):
    m = core.coded_matrix(getattr(ph, case)())
    vc, cc = np.ascontiguousarray(m.values), np.ascontiguousarray(m.codes)
    row_major = _native.prepare_layout(vc, cc)
    col_major = _native.prepare_layout(np.asfortranarray(vc), np.asfortranarray(cc))
    assert row_major.values_reordered.flags.c_contiguous and col_major.values_reordered.flags.f_contiguous
    assert row_major.info["reordered"] == 1
    _assert_same_outputs(row_major, col_major)
    order = row_major.order
    assert _same(row_major.values_reordered, vc[np.ix_(order, order)])
    assert _same(np.ascontiguousarray(col_major.codes_reordered), cc[np.ix_(order, order)])


def test_optional_outputs_and_reproducibility():
    m = ph.with_codes()
    full = _native.prepare_layout(m.values, m.codes)
    again = _native.prepare_layout(m.values, m.codes)
    _assert_same_outputs(full, again)
    for f, x in _outputs(full).items():
        assert _same(x, getattr(again, f)), f
    bare = _native.prepare_layout(m.values, m.codes, want_dense=False, want_reordered=False)
    assert bare.dense is None and bare.tdense is None and bare.values_reordered is None
    _assert_same_outputs(full, bare, skip=("dense", "tdense", "values_reordered", "codes_reordered"))
    no_dense = _native.prepare_layout(m.values, m.codes, want_dense=False)
    _assert_same_outputs(full, no_dense, skip=("dense", "tdense"))


def test_given_order_is_taken_and_reported_as_the_callers():
    D = ph.synthetic_matrix(65, 3, 0.5, 2)
    order = np.random.default_rng(3).permutation(65)
    p = _native.prepare_layout(D, None, order=order)
    assert p.info["order_route"] == _native.ORDER_DECLINED and np.array_equal(p.order, order)
    assert np.array_equal(p.values_reordered, D[np.ix_(order, order)], equal_nan=True)
    kept = _native.prepare_layout(D, None, order=[-1])
    assert kept.order is None and kept.info["reordered"] == 0
    with pytest.raises(_native.NativeError) as e:
        _native.prepare_layout(D, None, order=np.zeros(65, dtype=np.int32))
    assert e.value.code == _native.ERR_BAD_ARGUMENT


def test_public_entry_gives_the_same_embedding_either_way(monkeypatch):
    D = ph.synthetic_matrix(257, 5, 0.7, 3)
    routes = []
    real = core.prepare_layout_call_device

    def counted(*a, **k):
        route = []
        call = real(*a, route=route, **k)
        routes.append(route[0])    # only a call that came back from the device is counted
        return call

    monkeypatch.setattr(core, "prepare_layout_call_device", counted)
    results = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("TOPOLOW_DEVICE_PREP", flag)
        topolow_amd.set_seed(7)
        results[flag] = topolow_amd.euclidean_embedding(D, ndim=3, mapping_max_iter=30, k0=5.0, cooling_rate=0.01,
                                                        c_repulsion=0.01)
    topolow_amd.set_seed(None)
    assert routes == [_native.ORDER_DEVICE_GAP]
    a, b = results["1"], results["0"]
    assert np.array_equal(a.positions, b.positions) and np.array_equal(a.est_distances, b.est_distances)
    assert a.mae == b.mae and a.iter == b.iter


def test_fortran_input_and_kept_order_give_the_hosts_layout_and_copies(capsys):
    D = ph.synthetic_matrix(65, 3, 0.5, 2)
    F = np.asfortranarray(D)
    host, dev, route = _both(F, capsys)
    assert route == _native.ORDER_DEVICE_GAP
    _assert_field_for_field(host, dev)
    for M in (D, F):
        host, dev, route = _both(M, capsys, preserve_order=True)
        _assert_field_for_field(host, dev)
        assert not np.shares_memory(dev.reordered_matrix.values, M)
        assert not np.shares_memory(host.reordered_matrix.values, M)


def test_a_bad_scalar_argument_is_refused_before_the_device_is_asked(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was asked")

    monkeypatch.setattr(_native, "prepare_layout", no_device)
    D = ph.synthetic_matrix(33, 2, 0.3, 1)
    for over, message in ((dict(ndim=0), "ndim must be a positive integer"), (dict(k0=-1.0), "k0 must be a positive")):
        for fn in (core.prepare_layout_call, core.prepare_layout_call_device):
            with pytest.raises(ValueError, match=message):
                fn(D, preserve_order=False, **dict(PARAMS, **over))
