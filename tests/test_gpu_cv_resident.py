"""Cross-validation folds prepared on the device from a prepared handle (run with -m gpu): topolow_layout_prep_fold
against the host's topolow_cv_fold_pairs, topolow_layout_prep_cv_sweep against topolow_cv_sweep_session -- bit for bit --
and cv.likelihood_sweep(path="resident") against path="session" (topolow_amd/csrc/relax_prep_fold.h).

The shapes are small where the kernels can go wrong: one pair, the edges of the 64 x 64 tiles of the masked sums,
ragged last tiles, more than one workgroup per compacted column only at the one large case."""
import functools

import numpy as np
import pytest

from tests import parity_problems as pp
from tests import resident_helpers as rh
from tests import test_gpu_cv_session as base
from topolow_amd import _native, core, cv, synthetic

pytestmark = pytest.mark.gpu

N = base.N
SWEEP_OUTPUTS = ("holdout_sum_abs", "holdout_count", "iterations", "converged", "error_code")


def fold_matrix(n, form, seed=0):
    """Symmetric, 30-70 % NA, '>' / '<' codes on about 15 % of the cells, some diagonal cells NA and some not.
    form "exact": every value a multiple of 1/1024 (the device sums are exact); "generic": doubles as they come."""
    rng = np.random.default_rng(1000 * n + seed)
    pts = rng.normal(size=(n, 3)) * 3.0
    D = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1)) + 0.25
    if form == "exact":
        D = np.round(D * 1024.0) / 1024.0
    na = np.triu(rng.random((n, n)) < rng.uniform(0.3, 0.7), 1)
    if n == 2:
        na[:] = False                       # the one pair is measured
    D[na | na.T] = np.nan
    diag = np.where(rng.random(n) < 0.5, 0.0, np.nan)
    diag[0] = 0.0
    diag[n - 1] = np.nan
    D[np.arange(n), np.arange(n)] = diag
    u = np.triu(rng.random((n, n)), 1)
    u = u + u.T
    codes = np.zeros((n, n), dtype=np.int8)
    codes[(u > 0) & (u < 0.10)] = 1
    codes[(u >= 0.10) & (u < 0.15)] = -1
    assert np.array_equal(np.isnan(D), np.isnan(D.T)) and np.array_equal(codes, codes.T)
    return D, codes


def fold_picks(D, seed=0):
    """About a tenth of the cells, with diagonal cells (NA and not), duplicates, a cell together with its mirror, and
    NA cells."""
    n = D.shape[0]
    rng = np.random.default_rng(seed + 7)
    lin = rng.choice(n * n, size=max(1, n * n // 10), replace=False)
    measured = np.flatnonzero(~np.isnan(D.T).ravel())          # column-major linear indices
    missing = np.flatnonzero(np.isnan(D.T).ravel())
    r, c = measured[-1] % n, measured[-1] // n
    extra = [0, (n - 1) * (n + 1), lin[0], lin[0], r + c * n, c + r * n]
    extra += missing[:3].tolist()
    return np.concatenate([lin, np.array(extra, dtype=np.int64)]).astype(np.int64)


def cell_list(D, codes, names=None):
    m = core.CodedMatrix(np.asarray(D), np.zeros(D.shape, np.int32) if codes is None else codes.astype(np.int32), names)
    return m, cv.FoldBuilder(m)


def assert_same_fold(got, want, what):
    """PreparedHandle.fold against cv_fold_pairs: the pairs as sets, everything else exactly."""
    order, deg, vmax, n_edges, (pi, pj), (si, sj, st), route = got
    w_order, w_deg, w_vmax, w_edges, (w_pi, w_pj), (w_si, w_sj, w_st) = want
    assert route != _native.ORDER_DECLINED, what
    assert (order is None) == (w_order is None), what
    assert order is None or np.array_equal(order, w_order), what
    assert np.array_equal(deg, w_deg) and n_edges == w_edges, what
    assert rh.same_bits(np.float64(vmax), np.float64(w_vmax)), what
    assert np.all(pi < pj) and len(set(zip(pi.tolist(), pj.tolist()))) == pi.size, what
    assert set(zip(pi.tolist(), pj.tolist())) == set(zip(w_pi.tolist(), w_pj.tolist())), what
    assert np.array_equal(np.lexsort((pi, pj)), np.arange(pi.size)), what          # sorted by (j, i)
    assert np.array_equal(si, w_si) and np.array_equal(sj, w_sj) and rh.same_bits(st, w_st), what


# ---- 1. the fold preparation equals the host's -----------------------------------------------------------------------

def crosses_a_pass(rows, cols, rows_per_pass=256):
    """Some column lists rows of two different passes of the compaction kernels (kPrepThreads rows each)."""
    first, last = {}, {}
    for r, c in zip((np.asarray(rows) // rows_per_pass).tolist(), np.asarray(cols).tolist()):
        first[c] = min(first.get(c, r), r)
        last[c] = max(last.get(c, r), r)
    return any(first[c] != last[c] for c in first)


@pytest.mark.parametrize("form", ["exact", "generic"])
@pytest.mark.parametrize("n", [2, 63, 64, 65, 130, 203, 256, 257, 300, 513])
def test_fold_from_the_handle_equals_the_fold_from_the_cell_list(n, form):
    """fold_compact_count_kernel / fold_compact_write_kernel walk a column in passes of 256 rows with running bases.
    Up to n = 256 a column is one pass; 257 is the smallest n with a second one (one row: the column's scored cells
    only, a pair of column j lies in a row below j), 300 a ragged second pass that holds pairs too, 513 a third pass
    of one row."""
    D, codes = fold_matrix(n, form)
    m, fb = cell_list(D, codes)
    every = fb.rows + fb.cols * n                               # holds out every measured cell
    folds = dict(mixed=fold_picks(D), empty=np.zeros(0, np.int64), everything=every)
    if n > 256:         # the lists of the mixed fold do cross a pass: a change of fold_picks cannot quietly undo that
        _, _, _, _, (w_pi, w_pj), (w_si, w_sj, _) = _native.cv_fold_pairs(fb.cells(), folds["mixed"], True, True)
        assert crosses_a_pass(w_si, w_sj), n
        assert n == 257 or crosses_a_pass(w_pi, w_pj), n
    for layout in ("C", "F"):
        Dl = np.asfortranarray(D) if layout == "F" else np.ascontiguousarray(D)
        cl = np.asfortranarray(codes) if layout == "F" else np.ascontiguousarray(codes)
        with _native.PreparedHandle(Dl, cl, preserve_order=True) as h:
            for which, picks in folds.items():
                for named in (False, True):
                    for preserve in (False, True):
                        what = (n, form, layout, which, named, preserve)
                        got = h.fold(picks, preserve, named)
                        want = _native.cv_fold_pairs(fb.cells(), picks, preserve, named)
                        if n == 2 and form == "generic" and want[3] > 0 and not preserve:
                            # two points, one pair: both keys are that value, a tie on inexact sums -- declined, and
                            # everything that does not hang on the order is still the host's
                            assert got[6] == _native.ORDER_DECLINED and got[0] is None, what
                            assert np.array_equal(got[1], want[1]) and got[2:4] == want[2:4], what
                            assert rh.same_bits(got[5][2], want[5][2]), what
                            continue
                        assert_same_fold(got, want, what)
                        want_route = _native.ORDER_PRESERVED if preserve else (
                            _native.ORDER_DEVICE_EXACT if form == "exact" else _native.ORDER_DEVICE_GAP)
                        assert got[6] == want_route, what
                        if which == "everything":
                            assert got[3] == 0 and got[0] is None, what
                        if which == "mixed" and not preserve and n > 2:
                            assert got[0] is not None, what             # the order is exercised, not skipped
            assert folds["mixed"].size > 0 and h.fold(folds["empty"], False, True)[4][0].size == 0


# ---- 2. the sweep equals the session sweep, bit for bit ----------------------------------------------------------------

@functools.lru_cache(maxsize=2)
def sweep_problem(thresholds):
    """The 203-point problem of tests/test_gpu_cv_session.py as a matrix: plain, or with its '>' codes."""
    p = base.problem()
    D = np.ascontiguousarray(synthetic.make_problem(N, latent_dim=5, missing=0.6, seed=5).dissimilarity)
    codes = None
    if thresholds:
        codes = np.zeros((N, N), dtype=np.int8)
        codes[p["ei"], p["ej"]] = p["et"]
        codes[p["ej"], p["ei"]] = p["et"]
    m, fb = cell_list(D, codes)
    assert np.array_equal(fb.rows[fb.rows < fb.cols], p["ei"][np.lexsort((p["ei"], p["ej"]))])
    return D, codes, m, fb


def draw_folds(fb, ndims, seed, folds=None):
    rng = np.random.default_rng(seed)
    picks = fb.folds(len(ndims) if folds is None else folds, rng)[:len(ndims)]
    draws = [rng.random((d, fb.n - 1)) for d in ndims]
    seeds = [int(rng.integers(0, 2 ** 63 - 1)) for _ in ndims]
    return picks, draws, seeds


def both_sweeps(h, fb, named, preserve, ndims, picks, draws, seeds, n_iter, precision, schedule):
    nf = len(ndims)
    args = (named, preserve, ndims, [5.0] * nf, [0.02] * nf, [0.01] * nf, picks, draws, seeds, n_iter, 1e-4, 5, 3)
    got = h.cv_sweep(*args, precision=precision, schedule=schedule)
    want = _native.cv_sweep_session(fb.cells(), *args, precision=precision, schedule=schedule)
    return got, want


def assert_same_sweep(got, want, what):
    for name, a, b in zip(SWEEP_OUTPUTS, got[:5], want[:5]):
        assert rh.same_bits(a, b), (name, a, b) + what


@pytest.mark.parametrize("thresholds", [False, True], ids=["plain", "thresholds"])
@pytest.mark.parametrize("precision,schedule,ndim,env", base.CASES, ids=base.CASE_IDS)
def test_sweep_from_the_handle_equals_the_session_sweep(monkeypatch, precision, schedule, ndim, env, thresholds):
    for k in ("TOPOLOW_SYMMETRIC", "TOPOLOW_SYMMETRIC_MIN_N", "TOPOLOW_SYMMETRIC_STAGE_MIN_TILES"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    D, codes, m, fb = sweep_problem(thresholds)
    named = ndim == 5
    picks, draws, seeds = draw_folds(fb, [ndim] * 3, 31 + ndim)
    with _native.PreparedHandle(D, codes, preserve_order=True) as h:
        got, want = both_sweeps(h, fb, named, False, [ndim] * 3, picks, draws, seeds, 40, precision, schedule)
    what = (precision, schedule, ndim, thresholds)
    assert_same_sweep(got, want, what)
    assert not got[4].any() and got[1].min() > 0 and np.all(got[2] > 0), what
    assert np.all(got[6] == _native.ORDER_DEVICE_GAP), what


def test_two_ndim_groups_and_two_calls_on_one_handle_give_the_same_numbers():
    D, codes, m, fb = sweep_problem(True)
    ndims = [2, 5, 2, 5]
    picks, draws, seeds = draw_folds(fb, ndims, 77)
    with _native.PreparedHandle(D, codes, preserve_order=True) as h:
        got, want = both_sweeps(h, fb, True, False, ndims, picks, draws, seeds, 30, "auto", "auto")
        again = h.cv_sweep(True, False, ndims, [5.0] * 4, [0.02] * 4, [0.01] * 4, picks, draws, seeds, 30, 1e-4, 5, 3)
    assert_same_sweep(got, want, ("two groups",))
    assert_same_sweep(again, want, ("second call",))
    assert not got[4].any() and set(got[6].tolist()) == {_native.ORDER_DEVICE_GAP}


def test_bad_folds_in_the_middle_of_a_group_leave_the_others_and_the_handle_alone():
    """One ndim-2 group around a fold that fails its check (every measured cell picked), one that goes non-finite
    (k0 = 1e30: the library's own NaN detection) and one of ndim < 1: both sweeps report the same five outputs, the
    ordinary folds are what they are without the bad ones, and the mask is empty afterwards."""
    D, codes, m, fb = sweep_problem(True)
    ndims = [2, 2, 2, 0, 2, 2]
    picks, draws, seeds = draw_folds(fb, ndims, 41)
    picks = list(picks)
    picks[1] = fb.rows + fb.cols * N
    k0 = [5.0, 5.0, 1e30, 5.0, 5.0, 5.0]
    good = [0, 4, 5]

    def args(which):
        return (True, False, [ndims[f] for f in which], [k0[f] for f in which], [0.02] * len(which),
                [0.01] * len(which), [picks[f] for f in which], [draws[f] for f in which], [seeds[f] for f in which],
                30, 1e-4, 5, 3)
    with _native.PreparedHandle(D, codes, preserve_order=True) as h:
        got = h.cv_sweep(*args(range(6)))
        want = _native.cv_sweep_session(fb.cells(), *args(range(6)))
        clean = h.cv_sweep(*args(good))
        after = h.fold(picks[0], False, True)
    assert_same_sweep(got, want, ("bad folds",))
    assert got[4].tolist() == [_native.OK, _native.ERR_BAD_ARGUMENT, _native.ERR_NONFINITE, _native.ERR_BAD_ARGUMENT,
                               _native.OK, _native.OK]
    for name, a, b in zip(SWEEP_OUTPUTS, got[:5], clean[:5]):
        assert rh.same_bits(a[good], b), (name, a, b)
    assert got[1][good].min() > 0 and np.all(got[2][good] > 0)
    assert_same_fold(after, _native.cv_fold_pairs(fb.cells(), picks[0], False, True), ("after the bad folds",))


def test_the_handle_is_untouched_by_a_sweep():
    """The mask is cleared and vals / codes were never written: post_metrics and optimize on the handle give the bits
    they gave before the sweep, and a fold prepared afterwards is the fold prepared before."""
    D, codes, m, fb = sweep_problem(True)
    picks, draws, seeds = draw_folds(fb, [3, 3], 5)
    init = rh.start_positions(N, 3, 9)
    with _native.PreparedHandle(D, codes, preserve_order=True) as h:
        def observe():
            res = h.optimize(init, 3, 25, 5.0, 0.02, 0.01, seed=4)
            est, s, c = h.post_metrics(res.positions)
            return res.positions, res.iterations, res.final_mae, est, s, c, h.fold(picks[0], False, True)
        before = observe()
        out = h.cv_sweep(True, False, [3, 3], [5.0] * 2, [0.02] * 2, [0.01] * 2, picks, draws, seeds, 30, 1e-4, 5, 3)
        after = observe()
    assert not out[4].any()
    for a, b in zip(before[:6], after[:6]):
        assert rh.same_bits(a, b)
    assert_same_fold(after[6], before[6][:6], ("after the sweep",))


# ---- 3. a fold the device declines to order ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def tied_problem():
    """Generic values; points 3 and 17 are interchangeable -- each has one measurement, of the same value, to point 9 --
    so their keys are equal and not zero as long as a fold leaves both cells in: the ordering is declined."""
    n = 40
    D, _ = fold_matrix(n, "generic", seed=3)
    for a in (3, 17):
        D[a, :] = np.nan
        D[:, a] = np.nan
        D[a, 9] = D[9, a] = 2.7182818284590451
    m, fb = cell_list(D, None)
    return D, m, fb


def test_a_tied_fold_is_declined_and_the_others_run():
    D, m, fb = tied_problem()
    n = fb.n
    rng = np.random.default_rng(2)
    free = np.array([x for x in fb.rows + fb.cols * n if not {x % n, x // n} & {3, 17}], dtype=np.int64)
    tied = rng.choice(free, 60, replace=False)
    broken = np.concatenate([rng.choice(free, 60, replace=False), [3 + 9 * n]])
    picks = [tied, broken, tied[:30]]
    draws = [rng.random((2, n - 1)) for _ in picks]
    seeds = [11, 12, 13]
    with _native.PreparedHandle(D, None, preserve_order=True) as h:
        got = h.fold(tied, False, True)
        want = _native.cv_fold_pairs(fb.cells(), tied, False, True)
        assert got[6] == _native.ORDER_DECLINED and got[0] is None and want[0] is not None
        assert np.array_equal(got[1], want[1]) and got[2:4] == want[2:4]
        assert set(zip(*map(np.ndarray.tolist, got[4]))) == set(zip(*map(np.ndarray.tolist, want[4])))
        assert h.fold(tied, True, True)[6] == _native.ORDER_PRESERVED
        sweep, want = both_sweeps(h, fb, True, False, [2, 2, 2], picks, draws, seeds, 30, "auto", "auto")
    assert sweep[6].tolist() == [_native.ORDER_DECLINED, _native.ORDER_DEVICE_GAP, _native.ORDER_DECLINED]
    assert sweep[4].tolist() == [_native.ERR_UNSUPPORTED, _native.OK, _native.ERR_UNSUPPORTED]
    assert not want[4].any()
    for a, b in zip(sweep[:4], want[:4]):
        assert rh.same_bits(a[1], b[1]) and a[0] == 0 and a[2] == 0       # fold 1 ran, the declined ones report nothing
    # the whole route: the declined folds are rerun through the session sweep and merged in fold order
    sets = [dict(N=2, k0=5.0, cooling_rate=0.02, c_repulsion=0.01)]
    ra, rb = np.random.default_rng(4), np.random.default_rng(4)
    a = cv.likelihood_sweep(D, sets, 30, 1e-4, folds=4, rng=ra, path="resident")
    b = cv.likelihood_sweep(D, sets, 30, 1e-4, folds=4, rng=rb, path="session")
    assert a[0] == b[0] and a[2] == b[2] == 4 and 1 <= a[3] <= 4
    assert ra.bit_generator.state == rb.bit_generator.state


# ---- 4. the routing in cv.likelihood_sweep, and a matrix beyond one workgroup -----------------------------------------

def test_resident_path_returns_what_the_session_path_returns_on_the_hiv_panel():
    hv = pp.hiv_matrix()
    sets = [base.HIV, dict(N=3, k0=5.0, cooling_rate=0.02, c_repulsion=0.005)]
    r1, r2 = np.random.default_rng(9), np.random.default_rng(9)
    a = cv.likelihood_sweep(hv, sets, 60, 1e-4, folds=5, rng=r1, path="resident")
    b = cv.likelihood_sweep(hv, sets, 60, 1e-4, folds=5, rng=r2, path="session")
    assert len(a) == 4 and len(b) == 3 and a[3] == 0
    assert a[0] == b[0] and a[2] == b[2] == 10
    assert all(len(x["fold_n_samples"]) == 5 and np.isfinite(x["Holdout_MAE"]) for x in a[0])
    assert r1.bit_generator.state == r2.bit_generator.state


def test_sweep_beyond_one_workgroup_equals_the_session_sweep():
    n = 2973
    D = np.ascontiguousarray(synthetic.make_problem(n, latent_dim=5, missing=0.7, seed=4).dissimilarity)
    assert not _native.batch_problem_fits(n, 5, "f64", 0)
    m, fb = cell_list(D, None)
    picks, draws, seeds = draw_folds(fb, [5] * 3, 6, folds=20)
    with _native.PreparedHandle(D, None, preserve_order=True) as h:
        got, want = both_sweeps(h, fb, False, False, [5] * 3, picks, draws, seeds, 30, "f32", "slab")
    assert_same_sweep(got, want, ("n = 2973",))
    assert not got[4].any() and got[1].min() > 0


# ---- 5. refusals --------------------------------------------------------------------------------------------------------

def refused(code, match, fn, *a, **kw):
    with pytest.raises(_native.NativeError, match=match) as e:
        fn(*a, **kw)
    assert e.value.code == code, e.value


def test_refusals_leave_the_handle_usable():
    D, codes, m, fb = sweep_problem(True)
    picks, draws, seeds = draw_folds(fb, [2, 2], 13)
    args = (True, False, [2, 2], [5.0] * 2, [0.02] * 2, [0.01] * 2)
    tail = (draws, seeds, 30, 1e-4, 5, 3)
    with _native.PreparedHandle(D, codes, preserve_order=True) as h:
        want = _native.cv_sweep_session(fb.cells(), *args, picks, *tail)
        refused(_native.ERR_UNSUPPORTED, "f64_exact", h.cv_sweep, *args, picks, *tail, precision="f64_exact")
        assert_same_sweep(h.cv_sweep(*args, picks, *tail), want, ("after f64_exact",))
        beyond = [picks[0], np.concatenate([picks[1], [N * N]])]
        refused(_native.ERR_BAD_ARGUMENT, "outside the matrix", h.cv_sweep, *args, beyond, *tail)
        assert_same_sweep(h.cv_sweep(*args, picks, *tail), want, ("after a pick beyond the matrix",))
        refused(_native.ERR_BAD_ARGUMENT, "outside the matrix", h.fold, beyond[1], False, True)
        refused(_native.ERR_BAD_ARGUMENT, "outside the matrix", h.fold, np.array([-1]), False, True)
        assert_same_fold(h.fold(picks[0], False, True), _native.cv_fold_pairs(fb.cells(), picks[0], False, True), ("after",))
        assert_same_sweep(h.cv_sweep(*args, picks, *tail), want, ("after the refused folds",))
    # an asymmetric matrix: one mirror with another value, one with another code, one missing
    for change in ("value", "code", "na"):
        A, ac = D.copy(), codes.copy()
        i, j = int(fb.rows[fb.rows < fb.cols][5]), int(fb.cols[fb.rows < fb.cols][5])
        if change == "value":
            A[i, j] = np.nextafter(A[i, j], np.inf)
        elif change == "code":
            ac[i, j] = -1 if ac[i, j] == 0 else 0
        else:
            A[i, j] = np.nan
        with _native.PreparedHandle(A, ac, preserve_order=True) as h:
            for _ in range(2):      # decided once per handle, refused every time
                refused(_native.ERR_UNSUPPORTED, "not symmetric", h.cv_sweep, *args, picks, *tail)
            refused(_native.ERR_UNSUPPORTED, "not symmetric", h.fold, picks[0], False, True)
    # a reordered handle and one that declined to order: the fold's labels are the caller's
    with _native.PreparedHandle(D, codes) as h:
        assert h.order is not None
        order = h.order.copy()
        refused(_native.ERR_BAD_ARGUMENT, "preserve_order", h.cv_sweep, *args, picks, *tail)
        refused(_native.ERR_BAD_ARGUMENT, "preserve_order", h.fold, picks[0], False, True)
        assert np.array_equal(h.fetch(want_dense=False, want_reordered=False).order, order)
    T = tied_problem()[0]
    with _native.PreparedHandle(T, None) as h:
        assert h.declined
        refused(_native.ERR_BAD_ARGUMENT, "preserve_order", h.fold, np.array([1]), False, True)
