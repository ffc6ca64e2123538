"""Host side of the CV sweep on resident sessions (no GPU): the fold routine without the edge list
(topolow_cv_fold_pairs, topolow_amd/csrc/relax_fold.h) against topolow_cv_fold, the symmetric-list condition, the
routing predicate (topolow_batch_problem_fits), and topolow_cv_fold itself against its NumPy twin after the
refactoring that lets the two routines share their steps."""
import csv
import os

import numpy as np
import pytest

from topolow_amd import _native, antigenic, core, cv

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _symmetric_coded(n, seed, named):
    """Symmetric coded matrix: about 40 % NA pairs, ">" / "<" pairs, a non-NA diagonal."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.5, 6.0, (n, n)); d = np.triu(d, 1); d = d + d.T
    codes = np.zeros((n, n), dtype=np.int32)
    iu, ju = np.triu_indices(n, 1)
    u = rng.uniform(size=iu.size)
    na = u < 0.40
    d[iu[na], ju[na]] = np.nan; d[ju[na], iu[na]] = np.nan
    thr = (u >= 0.40) & (u < 0.52)
    c = np.where(rng.uniform(size=iu.size) < 0.5, 1, -1)
    codes[iu[thr], ju[thr]] = c[thr]; codes[ju[thr], iu[thr]] = c[thr]
    names = [f"p{q}" for q in range(n)] if named else None
    return core.CodedMatrix(d, codes, names, True)


def _picks(m, rng):
    """Linear (column-major) held-out cells: numeric and threshold cells, a diagonal cell, a cell AND its mirror, an NA
    cell."""
    n = m.values.shape[0]
    r, c = np.nonzero(~np.isnan(m.values) & ~np.eye(n, dtype=bool))
    take = rng.choice(r.size, size=r.size // 8, replace=False)
    lin = (r[take] + c[take] * n).tolist()
    lin.append(5 + 5 * n)                                   # a diagonal cell
    lin.append(int(c[take[0]] + r[take[0]] * n))            # the mirror of a picked cell
    nr, ncol = np.nonzero(np.isnan(m.values))
    lin.append(int(nr[0] + ncol[0] * n))                    # an NA cell
    return np.array(lin, dtype=np.int64)


@pytest.mark.parametrize("named", [True, False])
@pytest.mark.parametrize("preserve_order", [False, True])
def test_fold_pairs_is_the_fold_of_cv_fold(named, preserve_order):
    n = 37
    m = _symmetric_coded(n, 11, named)
    fb = cv.FoldBuilder(m)
    picks = _picks(m, np.random.default_rng(4))
    order, deg, ei, ej, ed, et, hi, hj, ht, vmax = _native.cv_fold(fb.cells(), picks, preserve_order, named)
    order2, deg2, vmax2, n_edges, (pi, pj), (si, sj, st) = _native.cv_fold_pairs(fb.cells(), picks, preserve_order, named)
    assert (order is None) == (order2 is None) == preserve_order
    to_caller = np.arange(n) if order is None else order
    if order is not None:
        assert np.array_equal(order, order2)
    assert np.array_equal(deg, deg2[to_caller])             # cv_fold's degrees are those of the points order[q]
    assert vmax == vmax2 and n_edges == ei.size
    # the scored cells give cv_fold's score on arbitrary positions: cv_fold's lists index the reordered problem
    pos_caller = np.random.default_rng(2).normal(size=(n, 3))
    pos_fold = pos_caller[to_caller]
    want = np.abs(ht - np.linalg.norm(pos_fold[hi] - pos_fold[hj], axis=1)).sum()
    got = np.abs(st - np.linalg.norm(pos_caller[si] - pos_caller[sj], axis=1)).sum()
    assert si.size == hi.size and got == pytest.approx(want, rel=1e-15)
    assert sorted(st.tolist()) == sorted(ht.tolist())
    # the held-out pairs are what the fold's edges leave of the full edge set
    fr, fc = np.nonzero(np.triu(~np.isnan(m.values), 1))
    full = set(zip(fr.tolist(), fc.tolist()))
    a, b = to_caller[ei], to_caller[ej]
    kept = set(zip(np.minimum(a, b).tolist(), np.maximum(a, b).tolist()))
    held = list(zip(pi.tolist(), pj.tolist()))
    assert len(set(held)) == len(held) and all(i < j for i, j in held)
    assert set(held) == full - kept and kept <= full


def test_fold_pairs_refuses_an_asymmetric_cell_list():
    m = _symmetric_coded(20, 3, True)
    r, c = np.nonzero(np.triu(~np.isnan(m.values), 1))
    m.values[c[0], r[0]] = np.nan                            # the lower mirror of a measured cell is NA
    fb = cv.FoldBuilder(m)
    with pytest.raises(_native.NativeError) as e:
        _native.cv_fold_pairs(fb.cells(), np.array([int(r[1] + c[1] * 20)]), False, True)
    assert e.value.code == _native.ERR_UNSUPPORTED and "symmetric" in str(e.value)
    m2 = _symmetric_coded(20, 3, True)
    m2.codes[c[0], r[0]] = 1 if m2.codes[r[0], c[0]] != 1 else -1     # ... or carries another code
    with pytest.raises(_native.NativeError) as e:
        _native.cv_fold_pairs(cv.FoldBuilder(m2).cells(), np.array([int(r[1] + c[1] * 20)]), False, True)
    assert e.value.code == _native.ERR_UNSUPPORTED


def test_batch_problem_fits():
    assert _native.batch_problem_fits(335, 2, "f64", 1700)
    assert not _native.batch_problem_fits(4000, 5, "f64", 0)
    assert not _native.batch_problem_fits(4000, 5, "f64", 2_000_000)
    assert _native.batch_problem_fits(2048, 5, "f64", 600_000)      # the dense form: the edge count does not matter
    assert not _native.batch_problem_fits(500, 17, "f64", 100)      # wider than the kernel's instances


def test_cv_fold_is_unchanged_on_the_hiv_panel():
    rows = list(csv.DictReader(open(os.path.join(GOLD, "hiv_distances.csv"))))
    m = core.coded_matrix(antigenic.titers_list_to_matrix(rows, "Virus", "virusYear", "Antibody", None, "distance",
                                                          sort=True))
    fb = cv.FoldBuilder(m)
    for q, h in enumerate(fb.folds(3, np.random.default_rng(8))):
        for preserve in (False, True):
            lib_call, lib_hold = fb.fold(h, 2, 50, 2.0, 0.02, 0.01, 1e-4, 5, 3, preserve, np.random.default_rng(q))
            np_call, np_hold = fb.fold_numpy(h, 2, 50, 2.0, 0.02, 0.01, 1e-4, 5, 3, preserve, np.random.default_rng(q))
            assert (lib_call.order is None) == (np_call.order is None)
            if np_call.order is not None:
                assert np.array_equal(lib_call.order, np_call.order)
            for f in ("initial_positions", "degrees", "edge_i", "edge_j", "edge_dist", "edge_thresh"):
                assert np.array_equal(getattr(lib_call, f), getattr(np_call, f)), f
            assert all(np.array_equal(a, b) for a, b in zip(lib_hold, np_hold))
