"""topolow_post_metrics on the device: est_distances and the terms of mae in one fused pass (R/core.R:474-481).
count exactly, est bit for bit against topolow_est_distances, sum_abs against an exactly rounded sum to the project's
f64 band of 1e-12 (a column's partial is a tree over <= n terms and the columns are added one after another: the
worst case is about n * 2^-53 <= 1.3e-13 relative at these sizes); the same bits whatever the tiling and whether or
not est is asked for; both forms of the input; the public entry point; the R shim's routine."""
import math

import numpy as np
import pytest

from tests import post_metrics_helpers as pm
from tests.helpers import quickstart_matrix
from topolow_amd import _native, core

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 2), (5, 2), (255, 5), (256, 10), (257, 3), (300, 17), (1111, 5)]


@pytest.mark.parametrize("n,ndim", SHAPES)
def test_against_numpy(n, ndim):
    p, values, codes = pm.make_inputs(n, ndim, seed=1000 + n)
    want_est = _native.est_distances(p)
    for cds in (None, codes):
        est, sum_abs, count = _native.post_metrics(p, values, cds)
        mask = pm.counting_cells(values, cds)
        ref = pm.reference_sum(values, want_est, mask)
        print(f"n={n} ndim={ndim} codes={cds is not None}: count {count}, sum_abs {sum_abs!r}, fsum {ref!r}, "
              f"rel {abs(sum_abs - ref) / ref if ref else 0.0:.3e}")
        assert count == np.count_nonzero(mask)
        assert np.array_equal(est, want_est)
        assert abs(sum_abs - ref) <= 1e-12 * abs(ref)
    if n > 2:
        assert 0 < np.count_nonzero(pm.counting_cells(values, codes)) < np.count_nonzero(pm.counting_cells(values))


def test_tiling_and_options_change_no_bit(monkeypatch):
    """n = 300 through 300 tiles, 43 tiles (the last one partial: 300 = 42 * 7 + 6) and one tile, with and without
    est: buffer reuse, event order, the last partial tile."""
    p, values, codes = pm.make_inputs(300, 5, seed=7)
    runs = []
    for cap in ("1", "7", None):
        if cap is None:
            monkeypatch.delenv("TOPOLOW_POST_TILE_COLS", raising=False)
        else:
            monkeypatch.setenv("TOPOLOW_POST_TILE_COLS", cap)
        for want in (True, False):
            runs.append((cap, want) + _native.post_metrics(p, values, codes, want_est=want))
    _, _, est0, sum0, count0 = runs[0]
    assert count0 == np.count_nonzero(pm.counting_cells(values, codes)) and count0 > 0
    for cap, want, est, s, c in runs:
        assert (s, c) == (sum0, count0), (cap, want, s, sum0)
        assert (est is None) == (not want)
        if want:
            assert np.array_equal(est, est0), (cap, want)
    assert np.array_equal(est0, _native.est_distances(p))


def test_nothing_counts():
    rng = np.random.default_rng(3)
    p = rng.normal(size=(40, 3))
    for values, codes in ((np.full((40, 40), np.nan), None),
                          (rng.uniform(1, 2, size=(40, 40)), np.ones((40, 40), np.int32))):
        est, sum_abs, count = _native.post_metrics(p, values, codes)
        assert count == 0 and sum_abs == 0.0 and math.copysign(1.0, sum_abs) == 1.0
        assert math.isnan(_native.mae_of(sum_abs, count))
        assert np.array_equal(est, _native.est_distances(p))


def test_nonfinite_positions_propagate():
    p = np.random.default_rng(4).normal(size=(20, 2))
    p[7, 1] = np.nan
    est, sum_abs, count = _native.post_metrics(p, np.ones((20, 20)))
    assert count == 400 and math.isnan(sum_abs) and np.isnan(est[7]).all() and np.isnan(est[:, 7]).all()


def test_the_two_input_forms_agree():
    """The matrices of the 16-argument call (+Inf = unmeasured, threshold_mask) against as.numeric of the reordered
    input with codes = NULL: same cells, same bits."""
    rng = np.random.default_rng(11)
    n = 200
    pts = rng.normal(size=(n, 3)) * 2.0
    D = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1))
    M = D.astype(object)
    for a in range(n):
        for b in range(a + 1, n):
            u = rng.random()
            if u < 0.5:
                M[a, b] = M[b, a] = None
            elif u < 0.6:
                M[a, b] = M[b, a] = ">" + repr(float(D[a, b]))
            elif u < 0.65:
                M[a, b] = M[b, a] = "<" + repr(float(D[a, b]))
    call = core.prepare_layout_call(M, 3, 10, 5.0, 0.03, 0.7, 1e-4, 5, None, False, 3, False,
                                    np.random.default_rng(0))
    p = rng.normal(size=(n, 3))
    numeric = call.reordered_matrix.as_numeric()
    _, s_call, c_call = _native.post_metrics(p, call.dissimilarity_matrix, call.threshold_matrix, want_est=False)
    est, s_num, c_num = _native.post_metrics(p, numeric, None)
    assert c_call == c_num == np.count_nonzero(~np.isnan(numeric)) and 0 < c_num < n * n
    assert np.count_nonzero(call.threshold_matrix) > 0
    assert s_call == s_num
    assert _native.mae_of(s_num, c_num) == pytest.approx(core.post_mae(call.reordered_matrix, est), rel=1e-12, abs=0)


def test_end_to_end_through_the_public_entry_point():
    import topolow_amd
    topolow_amd.set_seed(123)
    thr = np.array([["0", ">2", "3"], [">2", "0", "4"], ["3", "4", "0"]], dtype=object)
    thr[0, 2] = thr[2, 0] = None
    for matrix, args in ((quickstart_matrix(), (2, 200, 5.0, 0.03, 0.7)), (thr, (2, 10, 1.0, 0.01, 0.01))):
        r = topolow_amd.euclidean_embedding(matrix, *args)
        assert np.array_equal(r.est_distances, _native.est_distances(r.positions))
        # the matrix as the driver reordered it (the order is a function of the matrix alone)
        call = core.prepare_layout_call(matrix, args[0], args[1], args[2], args[3], args[4], 1e-4, 5, None, False, 3,
                                        False, np.random.default_rng(0))
        want = core.post_mae(call.reordered_matrix, r.est_distances)
        print(f"mae {r.mae!r} post_mae {want!r}")
        assert math.isfinite(want) and r.mae == pytest.approx(want, rel=1e-12, abs=0)
    topolow_amd.set_seed(None)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return pm.build_harness(tmp_path_factory.mktemp("rpost"))


def test_shim_equals_the_library(harness, tmp_path):
    p, values, codes = pm.make_inputs(23, 3, seed=23)
    values, codes = np.asfortranarray(values), np.asfortranarray(codes)
    est, sum_abs, count = _native.post_metrics(p, values, codes)
    out = pm.run_harness(harness, tmp_path, p, values, codes, True)
    assert out["error"] is None and out["names"] == ["est_distances", "mae", "sum_abs", "count"]
    assert out["protect_depth"] == 0 and out["est_dim"] == [23, 23]
    assert np.array_equal(np.array(out["est_distances"]).reshape((23, 23), order="F"), est)
    assert out["sum_abs"] == sum_abs and out["count"] == count and out["mae"] == sum_abs / count and count > 0
    bare = pm.run_harness(harness, tmp_path, p, values, None, False)
    _, s2, c2 = _native.post_metrics(p, values, None, want_est=False)
    assert bare["est_distances"] is None and bare["error"] is None and bare["protect_depth"] == 0
    assert (bare["sum_abs"], bare["count"]) == (s2, c2) and c2 > count
    none = pm.run_harness(harness, tmp_path, p, np.full((23, 23), np.nan), None, False)
    assert none["count"] == 0 and none["sum_abs"] == 0.0 and math.isnan(none["mae"])
