"""Cross-validation folds past the first chunk of every kernel that works in chunks (run with -m gpu): the scan of the
edge-list compaction (cv_scan_kernel, 1 024 counts of 256 edges per chunk), the float instance of the compaction, the
score past its grid of 1 024 workgroups (topolow_amd/csrc/relax_cv.h), the fold lists of columns longer than one pass of
256 rows (topolow_amd/csrc/relax_prep_fold.h), folds with held-out pairs but no scored cell and the other way round,
and hold-outs on padded (ndim 11) and wide (ndim 17) sessions.

The comparisons are those of tests/test_gpu_cv_session.py and tests/test_gpu_cv_resident.py, imported; the sizes are the
smallest that reach the second chunk: 262 145 edges or pairs, 1 025 count blocks.  Everything is compared bit for bit
except the score, which is held to a derived 1e-12 against a long-double reference."""
import functools
import math

import numpy as np
import pytest

from tests import test_gpu_cv_resident as resident
from tests import test_gpu_cv_session as base
from topolow_amd import _native, synthetic

pytestmark = pytest.mark.gpu

N = base.N
BIG = 760
EDGES_PER_COUNT = 256                           # kThreads: edges per workgroup of cv_edges_count_kernel
SCAN_CHUNK = 1024 * EDGES_PER_COUNT             # edges behind one chunk of cv_scan_kernel; the stride of cv_score_kernel
FULL_SYMMETRIC = base.FULL_SYMMETRIC
EDGE_MAE = dict(FULL_SYMMETRIC, TOPOLOW_EDGE_MAE="1")
ROW_OWNER = dict(TOPOLOW_SYMMETRIC="0")


@functools.lru_cache(maxsize=1)
def big_matrix():
    """760 points, 5 % missing: 273 999 measured pairs, 1 071 count blocks -- a full scan chunk and one of 47."""
    D = np.ascontiguousarray(synthetic.make_problem(BIG, latent_dim=5, missing=0.05, seed=4).dissimilarity)
    assert np.array_equal(np.isnan(D), np.isnan(D.T)) and not np.isnan(np.diag(D)).any()
    assert np.count_nonzero(np.triu(~np.isnan(D), 1)) > SCAN_CHUNK + EDGES_PER_COUNT
    return D


@functools.lru_cache(maxsize=1)
def big_problem():
    """big_matrix() as base.problem(): one hold set of 3 000 random edges, the edges on either side of the chunk
    boundary of the list, the first and the last one, and the oddities of every hold set."""
    D = big_matrix()
    m = np.count_nonzero(np.triu(~np.isnan(D), 1))
    p = base.problem(BIG, D, n_hold=3000, always=(0, SCAN_CHUNK - 1, SCAN_CHUNK, m - 1), which=("plain",))
    assert p["ei"].size == m and not p["holds"]["plain"]["keep"][[0, SCAN_CHUNK - 1, SCAN_CHUNK, m - 1]].any()
    return p


def clear_symmetric_env(monkeypatch):
    for k in ("TOPOLOW_SYMMETRIC", "TOPOLOW_SYMMETRIC_MIN_N", "TOPOLOW_SYMMETRIC_STAGE_MIN_TILES", "TOPOLOW_EDGE_MAE"):
        monkeypatch.delenv(k, raising=False)


# ---- 1. edge-list compaction past one scan chunk ----------------------------------------------------------------------

@pytest.mark.parametrize("precision,env", [("f64", FULL_SYMMETRIC), ("f32", EDGE_MAE)], ids=["f64", "f32-edge-mae"])
def test_compaction_across_scan_chunks(monkeypatch, precision, env):
    """cv_edges_count_kernel / cv_scan_kernel / cv_edges_compact_kernel (<double>, and <float> under
    TOPOLOW_EDGE_MAE=1) on a list of 273 999 edges: 1 071 counts, so the scan carries its first chunk's total over
    sh[1023] into a second, partial chunk and writes offset[n_blocks] after it.  A second chunk needs more than
    1 024 x 256 edges, and a symmetric matrix without NA holds that many from 725 points on; 760 leaves the generator
    room.  The f64 session runs the symmetric sweep, whose tile-major copy and delta tiles span 12 tile-rows here.  An
    edge dropped, doubled or moved changes the summation of the edge MAE and with it the bits of the check trace."""
    p = big_problem()
    assert p["ei"].size > SCAN_CHUNK + EDGES_PER_COUNT

    def inspect(s, ran):
        assert not s.uses_dense_mae
        assert not ran or precision != "f64" or s.symm_grid > 0
    base.check_held_out_session(monkeypatch, p, p["holds"]["plain"], precision, "slab", 2, env, thresholds_left=True,
                                run_first=True, inspect=inspect)


# ---- 2. the chunk boundary itself ------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("m", [SCAN_CHUNK, SCAN_CHUNK + 1])
def test_list_that_ends_at_the_scan_chunk_boundary(monkeypatch, precision, m):
    """cv_scan_kernel at exactly 1 024 counts (one full chunk, offset[1024] is the carry alone) and at 1 025 (a second
    chunk for one count of one edge), both instances of cv_edges_compact_kernel: the session's list is the first m
    edges of the block's, which is not the block, so either precision gathers.  Row-owner stages: only the list path
    differs between the sessions.  One hold set takes the last listed edge and the last edge of the first chunk, the
    other neither; both take edges of the block that are not listed.  The reference is a fresh session loaded with the
    fold's block and given the list without the held-out edges, in list order."""
    p = big_problem()
    full = base.full_edges(p)
    total = p["ei"].size
    assert total >= m + 16
    rng = np.random.default_rng(m)
    ends = np.unique([SCAN_CHUNK - 1, m - 1])
    inner = np.setdiff1d(rng.choice(m, 500, replace=False), ends)
    unlisted = np.arange(m + 3, m + 9)
    takes = dict(ends=np.concatenate([inner, ends, unlisted]), neither=np.concatenate([inner, unlisted]))
    init = synthetic.initial_positions(np.full((BIG, BIG), 6.0), 2, 3)

    def session(keep, deg):
        s = base.make_session(monkeypatch, precision, "slab", 2, ROW_OWNER, tuple(a[keep] for a in full), deg, n=BIG)
        s.set_edges(*(a[:m][keep[:m]] for a in full))
        assert not s.uses_dense_mae
        return s
    everything = np.ones(total, dtype=bool)
    s, never = session(everything, p["deg"]), session(everything, p["deg"])
    try:
        original = base.block(s)
        unheld = base.run(never, init, 2)
        for name, take in takes.items():
            keep = everything.copy()
            keep[take] = False
            fdeg = (p["deg"] - np.bincount(p["ei"][take], minlength=BIG) - np.bincount(p["ej"][take], minlength=BIG)).astype(np.int32)
            fresh = session(keep, fdeg)
            try:
                s.hold_out(p["ei"][take], p["ej"][take], fdeg)
                assert np.array_equal(base.block(s), base.block(fresh)), name
                held = base.run(s, init, 2)
                base.same_run(held, base.run(fresh, init, 2))
                assert not np.array_equal(held[1], unheld[1]), name
                s.restore_held_out(p["deg"])
                assert np.array_equal(base.block(s), original), name
                base.same_run(base.run(s, init, 2), unheld)
            finally:
                fresh.close()
    finally:
        s.close()
        never.close()


# ---- 3. the score past its grid ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("ndim", [2, 5, 11])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_score_past_its_grid(monkeypatch, precision, ndim):
    """cv_score_kernel<float> / <double> with more pairs than its 1 024 workgroups of 256 threads hold: 262 144 pairs
    are one per thread, 262 145 is the smallest count at which a thread strides (thread 0, twice), 600 001 has threads
    of two and of three pairs.  ndim 11 is stored as 12: the kernel reads rows of the stored width.

    The reference is math.fsum of |truth - r|, r from the positions finish() returned, in long double, rounded to
    double.  The bound 1e-12 * ref is derived: every term is non-negative; the longest chain of additions is 3 per
    thread + 6 shuffle steps + 4 waves + 1 024 partials on the host, about 1 040 * 2^-53 = 1.2e-13 relative; the
    rounding of each term adds a few 2^-53 * sum(truth + r) / sum|truth - r|, a ratio asserted below 10 on the
    reference."""
    p = base.problem()
    init = synthetic.initial_positions(np.full((N, N), 6.0), ndim, 3)
    s = base.make_session(monkeypatch, precision, "slab", ndim, FULL_SYMMETRIC, base.full_edges(p), p["deg"])
    try:
        pos = base.run(s, init, ndim)[0].positions.astype(np.longdouble)
        rng = np.random.default_rng(100 + ndim)
        for n_pairs in (SCAN_CHUNK, SCAN_CHUNK + 1, 600_001):
            pi = rng.integers(0, N, n_pairs).astype(np.int32)
            pj = rng.integers(0, N, n_pairs).astype(np.int32)
            truth = rng.uniform(0.0, 8.0, n_pairs)
            assert (pi == pj).any()
            d2 = np.zeros(n_pairs, dtype=np.longdouble)
            for d in range(ndim):
                diff = pos[pi, d] - pos[pj, d]
                d2 += diff * diff
            r = np.sqrt(d2).astype(np.float64)
            ref = math.fsum(np.abs(truth - r))
            ratio = math.fsum(truth + r) / ref
            got = s.score_pairs(pi, pj, truth)
            print(precision, ndim, n_pairs, "score", got[0], "reference", ref, "relative", abs(got[0] - ref) / ref,
                  "term ratio", ratio)
            assert ratio < 10
            assert got[1] == n_pairs
            assert abs(got[0] - ref) <= 1e-12 * ref
            assert s.score_pairs(pi, pj, truth) == got
    finally:
        s.close()


# ---- 4. one-sided folds from the handle (columns longer than one pass: resident.test_fold_from_the_handle_...) -----------

def one_sided_picks(D, codes):
    """Two valid folds no random draw gives: (a third of) the non-NA diagonal cells, which score and hold out no pair,
    and every other measured cell with a '>' or '<' code, which hold out pairs and score nothing."""
    n = D.shape[0]
    k = np.flatnonzero(~np.isnan(np.diag(D)))[::3]
    r, c = np.nonzero(~np.isnan(D) & (codes != 0))
    assert not (r == c).any()
    return (k * (n + 1)).astype(np.int64), (r + c * n)[::2].astype(np.int64)


@pytest.mark.parametrize("form", ["exact", "generic"])
@pytest.mark.parametrize("n", [65, 300])
def test_fold_with_pairs_or_scored_cells_only(n, form):
    """prep_fold_prepare with n_pairs == 0 and n_scored > 0, and the other way round: fold_compact_write_kernel runs
    with one of its lists empty (buffers grown to 0 elements).  65 points are one pass of two waves, 300 a second,
    ragged pass, in which the coded fold has pairs."""
    D, codes = resident.fold_matrix(n, form)
    m, fb = resident.cell_list(D, codes)
    diagonal, coded = one_sided_picks(D, codes)
    with _native.PreparedHandle(D, codes, preserve_order=True) as h:
        for named in (False, True):
            for preserve in (False, True):
                got = h.fold(diagonal, preserve, named)
                assert got[4][0].size == 0 and got[5][0].size == diagonal.size > 0
                resident.assert_same_fold(got, _native.cv_fold_pairs(fb.cells(), diagonal, preserve, named),
                                          (n, form, "diagonal", named, preserve))
                got = h.fold(coded, preserve, named)
                assert got[4][0].size > 0 and got[5][0].size == 0
                assert n <= 256 or resident.crosses_a_pass(*got[4])
                resident.assert_same_fold(got, _native.cv_fold_pairs(fb.cells(), coded, preserve, named),
                                          (n, form, "coded", named, preserve))


# ---- 5. the same through the sweeps --------------------------------------------------------------------------------------

def test_sweep_compacts_across_scan_chunks(monkeypatch):
    """topolow_layout_prep_cv_sweep against topolow_cv_sweep_session on the 760-point matrix, f64: the session gathers
    its 273 999 edges, and the fold's pairs reach cv_hold_out_pairs from the device, sorted by the caller's (j, i) and
    so unsorted in the session's labels, then go through the compaction of two scan chunks.  The fold lists come from
    columns of three passes."""
    clear_symmetric_env(monkeypatch)
    D = big_matrix()
    m, fb = resident.cell_list(D, None)
    picks, draws, seeds = resident.draw_folds(fb, [2] * 2, 8, folds=20)
    with _native.PreparedHandle(D, None, preserve_order=True) as h:
        got, want = resident.both_sweeps(h, fb, False, False, [2] * 2, picks, draws, seeds, 20, "f64", "slab")
    resident.assert_same_sweep(got, want, ("n = 760",))
    assert not got[4].any() and got[1].min() > 0
    assert np.all(got[6] == _native.ORDER_DEVICE_GAP)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_sweep_with_one_sided_folds(monkeypatch, precision):
    """A sweep of three folds -- a drawn one, a diagonal-only one and a coded-only one -- on both routes:
    cv_hold_out_pairs with no pair (the f64 session still compacts its list, to itself), a score over i == j cells
    only, and a fold that is run and not scored."""
    clear_symmetric_env(monkeypatch)
    D, codes, m, fb = resident.sweep_problem(True)
    picks, draws, seeds = resident.draw_folds(fb, [2] * 3, 19)
    diagonal, coded = one_sided_picks(D, codes)
    picks = [picks[0], diagonal, coded]
    with _native.PreparedHandle(D, codes, preserve_order=True) as h:
        got, want = resident.both_sweeps(h, fb, True, False, [2] * 3, picks, draws, seeds, 40, precision, "slab")
    resident.assert_same_sweep(got, want, (precision, "one-sided"))
    assert not got[4].any() and np.all(got[2] > 0)
    assert got[1][0] > 0 and got[1][1] == diagonal.size > 0 and got[1][2] == 0
    assert got[0][2] == 0.0


# ---- 6. sessions that no other CV test creates ---------------------------------------------------------------------------

@pytest.mark.parametrize("precision,ndim,env,gathers", [("f32", 5, EDGE_MAE, True), ("f32", 11, FULL_SYMMETRIC, False),
                                                        ("f32", 17, FULL_SYMMETRIC, True), ("f64", 17, FULL_SYMMETRIC, True)],
                         ids=["f32-ndim5-edge-mae", "f32-ndim11", "f32-ndim17", "f64-ndim17"])
def test_hold_out_on_padded_and_wide_sessions(monkeypatch, precision, ndim, env, gathers):
    """check_held_out_session on the 203-point problem for cv_edges_compact_kernel<float> beside a live symmetric sweep
    (ndim 5, TOPOLOW_EDGE_MAE=1), for positions stored wider than ndim (11 as 12: the score reads the stored width)
    and for ndim 17, the plain stage kernel on rows of 32, which gathers its edge list in either precision."""
    p = base.problem()

    def inspect(s, ran):
        assert s.uses_dense_mae == (not gathers)
    base.check_held_out_session(monkeypatch, p, p["holds"]["plain"], precision, "slab", ndim, env, thresholds_left=True,
                                run_first=True, inspect=inspect)
