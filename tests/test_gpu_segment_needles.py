"""The caller-driven segments of the symmetric sweep (include/topolow_relax.h: topolow_session_symm_segment_build / _sweep /
_apply -- what sharded.HipBackend.symm_prepare and ShardedRelaxation drive, one process per GPU) at small sizes, P ranks on
one device in one process (tests/segment_helpers.py replaces the wire, nothing else).  Run with -m gpu.

What only this path runs: sym_segment_build (tiles from ONE staged window of rows, row_first > 0, rows of several owners),
one inbox slot that takes the folded partials of ALL n points, the apply over [0, n) on a session whose own block is a
slice, the ERR instance's share through reduce_total_kernel (only the total over the ranks is a count of anything), and the
stop flag in the sweep, the reduction and the apply.

Problems and bands are those of tests/test_gpu_symmetric_long_runs.py: the needle problem (c_repulsion 0: one lost, doubled
or misplaced pair is an error of the order of the move) and that file's dense problem, against the f64 CPU model; every
check's (sum, count) against the oracle's edge error of the model's positions.  Plans are capped to one workgroup
(TOPOLOW_SYMMETRIC_GRID=1) so that a wave's run holds several units of several tiles, as at production size."""
import numpy as np
import pytest

from oracle import topolow_oracle as orc
from tests.segment_helpers import SegmentRanks
from tests.test_gpu_symmetric import _Env, _model_iterations
from tests.test_gpu_symmetric_long_runs import COOLING, K0, _dense_case, _idle_and_moved, _needle, _shape
from topolow_amd import _native

pytestmark = pytest.mark.gpu

CASES = [(3, False), (5, True), (7, False), (10, True)]          # (ndim, thresholded): both kernels (ndim <= 6, 7..10)
SCHEDULE = ((3, True), (6, True), (7, False))                    # seven iterations, check_freq 3: (iteration, fused)


def _assert_segment_shapes(n, g, P):
    """Every segment's plan on g workgroups has the shape asserted for the engine's segments: a unit of five tiles or
    more, a run of two units or more, every wave at work."""
    for b in range(P):
        sh = _shape(n, g, segment=b, n_segments=P)
        assert sh["longest"] >= 5 and sh["run_units"].max() >= 2 and sh["run_tiles"].min() >= 1, (b, sh)


def _edge_error(call, pos):
    return orc.edge_error(pos, call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)


def _assert_checks(ranks, call, want, schedule=SCHEDULE):
    """Every check of the run: the ranks' (sum, count) shares summed against the oracle's edge error of the model's
    positions -- the count exactly (the sweep's ERR partials carry twice the sum and twice the count, the separate pass
    carries them once), the ratio to 2e-5 -- and the same for every rank's check_trace()."""
    totals = ranks.check_totals()
    assert [(i, f) for i, f, _ in totals] == list(schedule)
    traces = [bk.session.check_trace() for bk in ranks.backs]
    for q, (iter1, fused, shares) in enumerate(totals):
        sm, c = _edge_error(call, want[iter1 - 1])
        s_, c_ = shares.sum(axis=0)
        print("check %d (%s): count %d (oracle %d), MAE off by %.2e" % (iter1, "fused" if fused else "separate", c_, c,
                                                                        abs(s_ / c_ / (sm / c) - 1.0)))
        assert c_ == (2 if fused else 1) * c, (iter1, c_, c)
        assert s_ / c_ == pytest.approx(sm / c, rel=2e-5), (iter1, s_ / c_, sm / c)
        for trace in traces:
            assert trace.shape[0] == len(totals) and int(trace[q, 0]) == iter1
            assert trace[q, 1] == pytest.approx(sm / c, rel=2e-5), (iter1, trace[q], sm / c)


def _one_and_seven(call, want, n, dim, P, g, c_rep, active=None):
    """One run of seven iterations (check_freq 3: the checks of 3 and 6 ride on the sweeps of 4 and 7, the last one is
    a separate pass), looked at after the first and after the last: all ranks bit-identical; after one iteration (i) and
    (ii) of _idle_and_moved on every rank (active given) or the fp32 bands; after seven the fp32 bands of part A of
    tests/test_gpu_symmetric_long_runs.py (mean 5e-5, max 5e-3 of the displacement scale) and every check.  Returns the
    largest error / band of (ii)."""
    init = call.initial_positions
    scale = np.abs(want[-1] - init).max()
    worst = None
    with SegmentRanks(call, n, dim, P, grid=g) as ranks:
        assert [bk.session.symm_grid for bk in ranks.backs] == [g] * P
        assert all(bk.session.uses_dense_mae and bk.can_fuse_segment_checks for bk in ranks.backs)
        ranks.begin(7, K0, COOLING, c_rep)
        for iters in (1, 7):
            ranks.advance(iters - ranks.it)
            got = [ranks.positions(r) for r in range(P)]
            for r in range(1, P):
                assert np.array_equal(got[r], got[0]), (iters, r)
            err = np.abs(got[0] - want[iters - 1])
            print("P=%d dim=%d iters=%d: max %.3g mean %.3g of the scale" % (P, dim, iters, err.max() / scale,
                                                                            err.mean() / scale))
            if iters == 1 and active is not None:
                worst = max(_idle_and_moved(got[r], want[0], init, active, "f32") for r in range(P))
            else:
                assert err.mean() <= 5e-5 * scale and err.max() <= 5e-3 * scale, (err.mean() / scale, err.max() / scale)
        _assert_checks(ranks, call, want)
        assert all(bk.session.stage_launches == 7 for bk in ranks.backs)
    return worst


# ----------------------------------------------------------------------------------------
# a. the needle problem over caller-built segments
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [2, 3, 7])
@pytest.mark.parametrize("dim,thresholded", CASES)
def test_needle_problem_over_caller_built_segments(dim, thresholded, P):
    """1 000 points over two, three and seven ranks, every rank's segment on one workgroup: 136, 90 - 91 or 38 - 39 tiles
    per segment; at seven ranks six segments start in the middle of a tile-row, windows such as rows [64, 192) lie inside
    two owners' 144-row blocks and rows [640, 1000) inside three.  After one iteration every rank holds the model's
    positions ((i) and (ii) of _idle_and_moved: an apply over the session's own rows only, a window row read at the wrong
    offset, a dropped tile-column are errors of the order of the move), all ranks bit for bit the same; after seven the
    fp32 bands and every check's summed (sum, count).
    Measured on an MI355X, largest error / band of (ii) at P = 2, 3, 7: ndim 3 plain 0.112, 0.112, 0.114; ndim 5
    thresholded 0.050, 0.070, 0.087; ndim 7 plain 0.078, 0.073, 0.086; ndim 10 thresholded 0.051, 0.057, 0.064 -- the
    0.05 to 0.11 of the engine's segments (same arithmetic per pair).  After seven iterations: max 2.6e-7, mean 1.6e-8
    of the scale at the most; every check's count exact and its MAE within 1.6e-7 of the oracle's."""
    n, g = 1000, 1
    _assert_segment_shapes(n, g, P)
    call, call_r, active = _needle(n, dim, 0, thresholded, "segments", P)
    want = _model_iterations(call_r, 7, K0, COOLING, 0.0)
    ratio = _one_and_seven(call, want, n, dim, P, g, 0.0, active)
    print("needle dim=%d thr=%d P=%d: largest error / band %.3f" % (dim, thresholded, P, ratio))


# ----------------------------------------------------------------------------------------
# b. the smallest cut: eight tiles per segment
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, None])
@pytest.mark.parametrize("dim,thresholded", [(3, False), (10, True)])
def test_smallest_cut_of_seven_segments(dim, thresholded, grid):
    """385 points (7 tile-rows, 56 tiles) over seven ranks: eight tiles per segment, the fewest the library cuts -- on one
    workgroup (two tiles per wave) and on the resident grid (at most one tile per wave).  One iteration: (i) and (ii)
    on every rank, all ranks bit-identical, and the iteration's one check.  Eight segments are refused.
    Measured on an MI355X, largest error / band of (ii): 0.081 (ndim 3, plain) and 0.060 (ndim 10, thresholded), the
    same on either grid."""
    n, P = 385, 7
    call, call_r, active = _needle(n, dim, 0, thresholded, "segments", P)
    want = _model_iterations(call_r, 1, K0, COOLING, 0.0)
    with SegmentRanks(call, n, dim, P, grid=grid) as ranks:
        grids = [bk.session.symm_grid for bk in ranks.backs]
        assert grids == [1] * P if grid else min(grids) >= 256
        for b in range(P):
            tiles = _shape(n, grids[b], segment=b, n_segments=P)["run_tiles"]
            assert tiles.sum() == 8 and (set(tiles) == {2} if grid else tiles.max() == 1), tiles
        ranks.begin(1, K0, COOLING, 0.0)
        ranks.advance(1)
        got = [ranks.positions(r) for r in range(P)]
        for r in range(1, P):
            assert np.array_equal(got[r], got[0]), r
        ratio = max(_idle_and_moved(got[r], want[0], call.initial_positions, active, "f32") for r in range(P))
        print("smallest cut dim=%d thr=%d grid=%s: largest error / band %.3f" % (dim, thresholded, grid, ratio))
        _assert_checks(ranks, call, want, schedule=((1, False),))
        s = ranks.backs[0].session
        assert _native.symm_segment_rows(n, 0, 8) is None and not s.symm_segment_eligible(8)
        with pytest.raises(_native.NativeError) as ei:
            s.symm_segment_build(0, 8, s.encoded_ptr, 0, ranks.blocks[0][1], ranks.any_thr)
        assert ei.value.code == _native.ERR_UNSUPPORTED


# ----------------------------------------------------------------------------------------
# c. the row window
# ----------------------------------------------------------------------------------------
def test_segment_is_built_from_exactly_its_row_window():
    """Segment 2 of 3 at 1 000 points (thresholded, ndim 5; rows [384, 1000), the rows of three owners): the build from
    exactly the window and the build from all rows [0, n) give bit-identical moves after a sweep; a window one row short
    at either end is refused (BAD_ARGUMENT, "does not hold the rows"), the session then holds no segment, and a correct
    build works again and repeats the bits."""
    n, dim, P, r = 1000, 5, 3, 2
    call, _, active = _needle(n, dim, 0, True, "segments", P)
    first, end = _native.symm_segment_rows(n, r, P)
    assert (first, end) == (384, 1000)
    with SegmentRanks(call, n, dim, P, grid=1) as ranks:
        ranks.begin(1, K0, COOLING, 0.0)
        bk, pos = ranks.backs[r], ranks.pos[r][0]

        def sweep():
            bk.symm_sweep(pos, 0, K0, False)
            return ranks.moves(r)

        exact = sweep()
        assert np.abs(exact).max() > 0 and np.array_equal(sweep(), exact)
        ranks.build(r, 0, n)
        assert np.array_equal(sweep(), exact)
        for lo, hi in ((first + 1, end), (first, end - 1)):
            with pytest.raises(_native.NativeError, match="does not hold the rows") as ei:
                ranks.build(r, lo, hi)
            assert ei.value.code == _native.ERR_BAD_ARGUMENT
            assert bk.session.symm_moves_ptr == 0 and bk.session.symm_grid == 0
            with pytest.raises(_native.NativeError, match="no segment built"):
                bk.session.symm_segment_sweep(pos.data_ptr(), 0, K0)
            ranks.build(r)
            assert bk.session.symm_grid == 1 and np.array_equal(sweep(), exact)


# ----------------------------------------------------------------------------------------
# d. a dense problem: repulsion and satisfied thresholds take part
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 10])
def test_dense_problem_over_caller_built_segments(dim):
    """The dense problem of tests/test_gpu_symmetric_long_runs.py (1 000 points, 70 % missing, 15 % thresholds,
    c_repulsion 0.01) over three ranks on one workgroup each: one and seven iterations against the model in part A's fp32
    bands, all ranks bit-identical, every check's summed (sum, count) against the oracle.
    Measured on an MI355X, of the displacement scale after one / seven iterations: ndim 3 max 1.0e-6 / 3.1e-5, mean
    7.0e-8 / 2.2e-6; ndim 10 max 3.0e-7 / 1.2e-5, mean 5.1e-8 / 1.3e-6; every count exact (138 635 to 138 730 pairs
    of 149 850 count), every MAE within 1.4e-7 of the oracle's."""
    n, P, g = 1000, 3, 1
    _assert_segment_shapes(n, g, P)
    call, want = _dense_case(n, dim, 0.15)
    _one_and_seven(call, want, n, dim, P, g, 0.01)


# ----------------------------------------------------------------------------------------
# e. after a stop
# ----------------------------------------------------------------------------------------
def test_after_a_stop_sweeps_checks_and_applies_do_nothing():
    """The plain ndim-3 needle problem over two ranks with window 1 and epsilon 0.5: the model's MAE falls from 2.341 at
    iteration 3 to 1.711 at iteration 6 (0.731 of it: inside the plateau band [0.5, 1.5] by a quarter of the value on
    either side), so the controller stops at the check of iteration 6, which rides on the sweep of iteration 7.  That
    sweep's apply and three more iterations with fused checks leave both position tensors of every rank as they were,
    a sweep leaves the moves buffer alone, every d_out2 reads (0, 0), poll() names iteration 6 and every rank's finish()
    returns the positions of iteration 6."""
    n, dim, P = 1000, 3, 2
    window, eps = 1, 0.5
    call, call_r, _ = _needle(n, dim, 0, False, "segments", P)
    want = _model_iterations(call_r, 6, K0, COOLING, 0.0)
    maes = [np.divide(*_edge_error(call, want[i - 1])) for i in (3, 6)]
    ks = [K0 * (1.0 - COOLING) ** i for i in (3, 6)]
    for wobble in (0.8, 1.0, 1.25):          # the verdict with margin: the second MAE a fifth lower or a quarter higher
        script = _native.controller_script([maes[0], maes[1] * wobble], [3, 6], ks, K0, window, eps)
        assert script["stopped_at"] == 1 and script["best_iter"] == 6, (wobble, script)
    with SegmentRanks(call, n, dim, P, grid=1) as ranks:
        ranks.begin(12, K0, COOLING, 0.0, eps=eps, window=window)
        ranks.advance(7)
        assert [bk.poll() for bk in ranks.backs] == [(True, 6)] * P
        assert [(i, f) for i, f, _ in ranks.checks] == [(3, True), (6, True)]
        at_stop = [[ranks.positions(r, b) for b in (0, 1)] for r in range(P)]
        six = at_stop[0][ranks.cur ^ 1]          # the stopped apply wrote nothing: the other buffer holds iteration 6
        scale = np.abs(want[-1] - call.initial_positions).max()
        err = np.abs(six - want[5])
        assert err.mean() <= 5e-5 * scale and err.max() <= 5e-3 * scale
        moves = [ranks.moves(r) for r in range(P)]
        for r, bk in enumerate(ranks.backs):
            bk.symm_sweep(ranks.pos[r][ranks.cur ^ 1], ranks.it, ranks.k, True)
            assert np.array_equal(ranks.moves(r), moves[r]) and np.abs(moves[r]).max() > 0
        for _ in range(3):
            ranks.iteration((ranks.it, ranks.k, ranks.cur))
        for _, fused, shares in ranks.check_totals()[2:]:
            assert fused and np.array_equal(shares, np.zeros((P, 2)))
        for r in range(P):
            for b in (0, 1):
                assert np.array_equal(ranks.positions(r, b), at_stop[r][b]), (r, b)
                assert np.array_equal(at_stop[r][b], at_stop[0][b]), (r, b)
        assert [bk.poll() for bk in ranks.backs] == [(True, 6)] * P
        results = [bk.finish() for bk in ranks.backs]
        sm, c = _edge_error(call, want[5])
        for res in results:
            assert np.array_equal(res.positions, six)
            assert (res.converged, res.iterations) == (True, 6) and res.final_k == pytest.approx(ks[1], rel=1e-12)
            assert res.final_mae == results[0].final_mae == pytest.approx(sm / c, rel=2e-5)
        assert all(bk.session.check_trace().shape[0] == 2 for bk in ranks.backs)


# ----------------------------------------------------------------------------------------
# f. a second edge list on a session that holds its sweep buffers
# ----------------------------------------------------------------------------------------
def test_whole_matrix_session_takes_its_edge_list_again_between_two_runs():
    """An fp32 session keeps its sweep buffers across topolow_session_set_edges, and the sweep's ERR instance writes one
    partial per unit of the plan it holds: 272 units at 1 000 points on the resident grid, where the list alone asks for
    125 partials.  The run after the second set_edges repeats the first bit for bit, two fused checks each."""
    n, dim = 1000, 5
    call, want = _dense_case(n, dim, 0.15)
    with _Env(TOPOLOW_SYMMETRIC="1", TOPOLOW_SYMMETRIC_MIN_N="0"):
        s = _native.Session(n, dim, precision="f32")
    try:
        s.load_dense(call.dissimilarity_matrix, call.threshold_matrix, call.degrees)

        def run():
            s.set_edges(call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
            s.set_positions(call.initial_positions)
            s.set_profiling(True)
            s.begin(7, K0, COOLING, 0.01, 1e-12, 10 ** 9, 3, 5, 1)
            s.run()
            s.sync()
            return s.get_positions(), s.check_trace().copy(), s.profile_symmetric()[3]

        a = run()
        assert s.symm_grid >= 256 and len(_native.symm_plan(n, 4 * s.symm_grid)[0]) == 272
        b = run()
        assert a[2] == b[2] == 2
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert [int(t) for t in a[1][:, 0]] == [3, 6, 7]
        for row in a[1]:
            sm, c = _edge_error(call, want[int(row[0]) - 1])
            assert row[1] == pytest.approx(sm / c, rel=2e-5)
    finally:
        s.close()


def _parity_share(s, call):
    """The edges of the session's row block under the parity rule of the sharded MAE (include/topolow_relax.h)."""
    lo, hi = np.minimum(call.edge_i, call.edge_j), np.maximum(call.edge_i, call.edge_j)
    own = np.where((lo + hi) % 2 == 0, lo, hi)
    return np.flatnonzero((own >= s.row_begin) & (own < s.row_end))


def _set_edges(s, call, idx):
    s.set_edges(call.edge_i[idx], call.edge_j[idx], call.edge_dist[idx], call.edge_thresh[idx])


def test_caller_built_segment_takes_its_edge_list_again_after_the_build():
    """Two ranks at 1 000 points on the resident grid (136 units per segment, where a 504-row block's list asks for 63
    partials): build, then set_edges, then a sweep with d_out2 gives, bit for bit, the shares of the order the drivers use
    (set_edges, then build), and their total is the oracle's."""
    n, dim, P = 1000, 3, 2
    call, _, _ = _needle(n, dim, 0, False, "segments", P)
    shares = []
    for again in (False, True):
        with SegmentRanks(call, n, dim, P) as ranks:
            assert min(bk.session.symm_grid for bk in ranks.backs) >= 256
            if again:
                for bk in ranks.backs:
                    _set_edges(bk.session, call, _parity_share(bk.session, call))
                    assert bk.session.symm_moves_ptr != 0 and bk.can_fuse_segment_checks
            ranks.begin(2, K0, COOLING, 0.0)
            ranks.iteration((0, K0, 0))
            shares.append(ranks.check_totals()[0][2])
    assert np.array_equal(shares[0], shares[1])
    sm, c = _edge_error(call, call.initial_positions)
    s_, c_ = shares[1].sum(axis=0)
    assert c_ == 2 * c and s_ / c_ == pytest.approx(sm / c, rel=2e-5)


# ----------------------------------------------------------------------------------------
# the fused-check guard
# ----------------------------------------------------------------------------------------
def test_segment_sweep_refuses_a_check_it_would_reduce_over_other_cells():
    """A row-block session given every second edge of its parity-rule share gathers its list (uses_dense_mae false): a
    check reduced in its segment sweep would run over the block's cells, the separate pass over the list -- the session
    says that it cannot (can_fuse_segment_checks), symm_segment_sweep with d_out2 is refused (UNSUPPORTED) and launches
    nothing, and the separate check_partial reports the half list's error: the count exactly, the sum to 2e-5."""
    n, dim, P = 1000, 3, 2
    call, _, _ = _needle(n, dim, 0, False, "segments", P)
    halves = {}

    def load_half(s, call_):
        s.load_coo(call_.edge_i, call_.edge_j, call_.edge_dist, call_.edge_thresh, call_.degrees)
        halves[s.row_begin] = _parity_share(s, call_)[::2]
        _set_edges(s, call_, halves[s.row_begin])

    with SegmentRanks(call, n, dim, P, grid=1, load=load_half) as ranks:
        ranks.begin(3, K0, COOLING, 0.0)
        for r, bk in enumerate(ranks.backs):
            s, pos = bk.session, ranks.pos[r][0]
            assert not s.uses_dense_mae and not s.can_fuse_segment_checks and not bk.can_fuse_segment_checks
            assert s.symm_moves_ptr != 0
            with pytest.raises(_native.NativeError, match="cannot reduce a check in its segment sweep") as ei:
                bk.symm_sweep(pos, 0, K0, True)
            assert ei.value.code == _native.ERR_UNSUPPORTED
            assert s.stage_launches == 0 and not ranks.moves(r).any()        # nothing was launched
            bk.symm_sweep(pos, 0, K0, False)
            assert s.stage_launches == 1 and ranks.moves(r).any()
            idx = halves[s.row_begin]
            sm, c = orc.edge_error(call.initial_positions, call.edge_i[idx], call.edge_j[idx], call.edge_dist[idx],
                                   call.edge_thresh[idx])
            got = bk.check_partial(pos).cpu().numpy()
            assert got[1] == c and c >= 200 and got[0] == pytest.approx(sm, rel=2e-5), (got, sm, c)


def test_fuse_checks_off_answers_the_segment_query_too():
    """TOPOLOW_FUSE_CHECKS=0 at session creation: the MAE still comes from the block, but no sweep may carry a check --
    the query says so and the sweep refuses; without the variable the same session answers yes."""
    n, dim, P = 385, 3, 7
    call, _, _ = _needle(n, dim, 0, False, "segments", P)
    for fuse in ("0", None):
        with SegmentRanks(call, n, dim, P, grid=1, env={"TOPOLOW_FUSE_CHECKS": fuse} if fuse else None) as ranks:
            ranks.begin(1, K0, COOLING, 0.0)
            for r, bk in enumerate(ranks.backs):
                assert bk.session.uses_dense_mae
                assert bk.session.can_fuse_segment_checks == bk.can_fuse_segment_checks == (fuse is None)
            bk, pos = ranks.backs[P - 1], ranks.pos[P - 1][0]
            if fuse is None:
                bk.symm_sweep(pos, 0, K0, True)
            else:
                with pytest.raises(_native.NativeError) as ei:
                    bk.symm_sweep(pos, 0, K0, True)
                assert ei.value.code == _native.ERR_UNSUPPORTED
