"""The convergence check pair by pair (run with -m gpu): dense_error_kernel in upper-triangle and PARITY form,
edge_error_kernel in the three precisions, the ERR instances of slab_stage_pipe_kernel, controller_kernel and
reduce_push_kernel against oracle.edge_error on the needle problems of tests/check_needles.py -- about n measured pairs among
n points, a pair planted on every seam of the kernels.  Every count is held as an integer, every sum to a band derived from
the arithmetic (check_needles.sum_band_f32; f64: 1e-12 of the sum); that one lost, doubled or misplaced pair falls outside
these assertions is tests/test_check_needles_host.py."""
import time

import numpy as np
import pytest

from tests import check_needles as cn
from tests.test_gpu_resident_embedding import _Env, _initial_edge_error
from topolow_amd import _native

pytestmark = pytest.mark.gpu

K0, COOLING = 1.5, 0.01


def _position_dim(s):
    return int(s.lib.topolow_session_position_dim(s._h))


def _session(nd, precision="f32", rows=None, relabel=0, targets="raw", share=None, env=None, block=None):
    """A session over `rows` (default: the whole problem) loaded from the list alone; share: mask of the listed pairs its
    check reduces (default: all); block: mask of the listed pairs its block holds (default: all)."""
    with _Env(**(env or {})):
        s = _native.Session(nd.n, nd.dim, *(rows or (0, nd.n)), precision=precision)
        if relabel:
            s.set_relabel(relabel)
        t = nd.edge_dist if targets == "raw" else nd.edge_dist_dev
        if block is None:
            s.load_coo(nd.edge_i, nd.edge_j, t, nd.edge_thresh, nd.degrees)
        else:
            bi, bj = nd.edge_i[block], nd.edge_j[block]
            degrees = 1 + np.bincount(bi, minlength=nd.n) + np.bincount(bj, minlength=nd.n)
            s.load_coo(bi, bj, t[block], nd.edge_thresh[block], degrees)
        m = slice(None) if share is None else share
        s.set_edges(nd.edge_i[m], nd.edge_j[m], t[m], nd.edge_thresh[m])
    return s


def _sparse_block(nd):
    """Every 1 500th listed pair: the block a session of the 4.5-million-edge list relaxes."""
    return np.arange(len(nd.edge_i)) % 1500 == 0


def _position_sets(nd):
    """The start, the start scaled by 2 (most ">" / "<" classifications flip) and a reshuffle of the rows."""
    rng = np.random.default_rng([nd.n, nd.dim, 99])
    return (("start", nd.pos), ("x 2", 2.0 * nd.pos), ("reshuffled", nd.pos[rng.permutation(nd.n)]))


def _hold(s, nd, pos, mask=None, which="dev", what=()):
    """Session.edge_error of `pos` against the oracle on the listed pairs of `mask`: returns (|d sum| / band, count)."""
    m = slice(None) if mask is None else mask
    t = (nd.edge_dist_dev if which == "dev" else nd.edge_dist)[m]
    want = cn.orc.edge_error(pos, nd.edge_i[m], nd.edge_j[m], t, nd.edge_thresh[m])
    if s.precision == "f32":
        band = cn.sum_band_f32(pos, nd.edge_i[m], nd.edge_j[m], t, nd.edge_thresh[m], _position_dim(s))
    else:
        band = 1e-12 * want[0]
    got = _initial_edge_error(s, pos)
    ok, ratio = cn.pass_holds(got, want, band)
    assert got[1] == want[1], ("count",) + tuple(what) + (got, want)
    assert ok, ("sum",) + tuple(what) + (got, want, band, ratio)
    return ratio, want[1]


# ---- 2a. the fp32 dense pass over the whole block -----------------------------------------------------------------------------

@pytest.mark.parametrize("thresholded", [False, True])
@pytest.mark.parametrize("n,dim", cn.DENSE_CASES)
def test_dense_pass_counts_every_pair_of_the_block(n, dim, thresholded):
    """dense_error_kernel<PARITY = false>: 2 113 points are three chunks with a last chunk of 68 columns and 34 tile rows,
    1 023 keep the last tile row short, 2 050 and 2 113 run the packed two-row path and the tile skip; ndim 13 runs
    zero-padded as 16.  Three position sets per session.
    Measured on an MI355X, the largest |d sum| / band per case: 0.19 at (3 points, ndim 2, plain) and 0.07 or less at the
    other sizes of one to ten pairs, 0.008 to 0.025 from 66 points on (0.001 at ndim 1)."""
    nd = cn.needle(n, dim, cn.SEED, thresholded)
    s = _session(nd)
    assert s.uses_dense_mae and s.position_rows == (n + 3) // 4 * 4 and _position_dim(s) == cn.kernel_dim(dim)
    worst = 0.0
    for name, pos in _position_sets(nd):
        ratio, cnt = _hold(s, nd, pos, what=(n, dim, thresholded, name))
        worst = max(worst, ratio)
        assert cnt > 0 or n < 16
    s.close()
    print("dense n=%d dim=%d thr=%d: largest |d sum| / band %.3f" % (n, dim, thresholded, worst))


def test_dense_pass_on_a_relabelled_session():
    """set_relabel: the block, the flags and the positions are in session labels; the same pairs count."""
    nd = cn.needle(2113, 5, cn.SEED, True)
    s = _session(nd, relabel=77)
    assert s.uses_dense_mae and not np.array_equal(s.labels(), np.arange(nd.n))
    for name, pos in _position_sets(nd):
        _hold(s, nd, pos, what=("relabel", name))
    s.close()


# ---- 2b. the PARITY pass: the same problems as row blocks on one device ---------------------------------------------------------

@pytest.mark.parametrize("thresholded", [False, True])
@pytest.mark.parametrize("n,dim", cn.DENSE_CASES)
def test_parity_pass_counts_every_pair_of_its_share(n, dim, thresholded):
    """dense_error_kernel<PARITY = true> on the blocks of shard_rows(n, 2) and (n, 3) and -- a Session accepts any row
    range -- on [0, 1 023), [1 023, 1 090), [1 090, n): odd row counts, starts that are no multiple of 64 or 2.  Every
    block's (sum, count) against the oracle on its share of the list (the parity rule); the counts add up to the whole
    list's.  Measured on an MI355X, the largest |d sum| / band per case: as the whole-block pass at 2 to 5 points (one block),
    0.003 to 0.051 from 66 points on."""
    nd = cn.needle(n, dim, cn.SEED, thresholded)
    splits = [cn.row_blocks(n, 2), cn.row_blocks(n, 3)] + ([cn.hand_made_blocks(n)] if cn.hand_made_blocks(n) else [])
    assert [list(b) for b in splits[:2]] == [_native.shard_rows(n, 2), _native.shard_rows(n, 3)]
    worst = 0.0
    sets = _position_sets(nd)
    for blocks in splits:
        totals = [0] * len(sets)
        for rb, re_ in blocks:
            share = cn.parity_share(nd, rb, re_)
            s = _session(nd, rows=(rb, re_), share=share)
            assert s.uses_dense_mae, (n, dim, rb, re_)
            for q, (name, pos) in enumerate(sets):
                ratio, cnt = _hold(s, nd, pos, mask=share, what=(n, dim, thresholded, name, rb, re_))
                worst = max(worst, ratio)
                totals[q] += cnt
            s.close()
        assert totals == [cn.oracle(pos, nd)[1] for _, pos in sets], (n, dim, thresholded, blocks)
    print("parity n=%d dim=%d thr=%d: largest |d sum| / band %.3f" % (n, dim, thresholded, worst))


# ---- 2c. the edge-list pass -----------------------------------------------------------------------------------------------------

def _sublist(nd, length, seed):
    """`length` of the listed pairs (the ties among them where they fit), every other one given as (j, i)."""
    rng = np.random.default_rng([nd.n, length, seed])
    perm = rng.permutation(len(nd.edge_i))
    if length > len(nd.ties):
        perm = np.concatenate([nd.ties, perm[~np.isin(perm, nd.ties)]])
    pick = np.sort(perm[:length])
    flip = np.arange(length) % 2 == 1
    ei, ej = nd.edge_i[pick], nd.edge_j[pick]
    return nd._replace(edge_i=np.where(flip, ej, ei).astype(np.int32), edge_j=np.where(flip, ei, ej).astype(np.int32),
                       edge_dist=nd.edge_dist[pick], edge_dist_dev=nd.edge_dist_dev[pick],
                       edge_thresh=nd.edge_thresh[pick], ties=np.zeros(0, dtype=np.int64))


@pytest.mark.parametrize("precision", ["f32", "f64", "f64_exact"])
@pytest.mark.parametrize("length", cn.LIST_LENGTHS)
def test_edge_list_pass_counts_every_listed_pair(length, precision):
    """edge_error_kernel on lists of 1, 255, 256, 257, 2 049 and 6 145 pairs (8 200 points list 9 800), in both
    orientations: fp32 forced onto the list (TOPOLOW_EDGE_MAE=1) and f64 on the targets as the device rounds them,
    f64_exact on the caller's.  Measured on an MI355X, the largest |d sum| / band: fp32 2.9e-9 (the pass computes in f64
    from fp32 positions), f64 0.0032, f64_exact 0.0012."""
    base = cn.needle(2113, 5, cn.SEED, True)
    if length > len(base.edge_i):
        base = cn.needle(*cn.BIG_DENSE, cn.SEED, True)
    nd = _sublist(base, length, 1)
    exact = precision == "f64_exact"
    with _Env(TOPOLOW_EDGE_MAE="1"):
        s = _native.Session(nd.n, nd.dim, precision=precision)
        t = nd.edge_dist if exact else nd.edge_dist_dev
        s.load_coo(nd.edge_i, nd.edge_j, t, nd.edge_thresh, nd.degrees)
        s.set_edges(nd.edge_i, nd.edge_j, t, nd.edge_thresh)
    assert not s.uses_dense_mae
    worst = 0.0
    for name, pos in _position_sets(nd):
        ratio, _ = _hold(s, nd, pos, which="raw" if exact else "dev", what=(length, precision, name))
        worst = max(worst, ratio)
    s.close()
    print("list of %d, %s: largest |d sum| / band %.3g" % (length, precision, worst))


def test_fp32_list_that_is_a_strict_subset_of_the_block_takes_the_list_pass():
    """No variable set: the block holds every pair, the list all but 17 of them -- the session must gather the list."""
    nd = cn.needle(2113, 5, cn.SEED, True)
    keep = np.ones(len(nd.edge_i), dtype=bool)
    keep[np.random.default_rng(5).permutation(len(keep))[:17]] = False
    s = _session(nd, share=keep)
    assert not s.uses_dense_mae
    for name, pos in _position_sets(nd):
        _hold(s, nd, pos, mask=keep, what=("subset", name))
    s.close()


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_edge_list_pass_beyond_one_trip_of_the_capped_grid(precision):
    """3 000 points with every pair listed: 4 498 500 edges, more than the 2 048 workgroups x 256 threads x 8 of the capped
    grid reduce in one trip, and 2 048 partials.  The list is generated directly (no n x n array); the block, loaded
    through load_coo, holds 3 000 of the pairs, so the session gathers the list without being told to.
    Measured on an MI355X: |d sum| / band 2.4e-8 (fp32) and 0.027 (f64); the test takes 0.75 s (fp32, which builds the
    list) and 0.11 s (f64)."""
    t0 = time.time()
    nd = cn.full_list(*cn.FULL_LIST, cn.SEED, True)
    assert len(nd.edge_i) > 2048 * 256 * 8
    s = _session(nd, precision=precision, targets="dev", block=_sparse_block(nd))
    assert not s.uses_dense_mae
    for name, pos in _position_sets(nd)[:2]:
        ratio, _ = _hold(s, nd, pos, what=("4.5M", precision, name))
        print("4.5M edges %s %s: |d sum| / band %.3g" % (precision, name, ratio))
    s.close()
    print("4.5M edges %s: %.2f s" % (precision, time.time() - t0))


# ---- 3a. the check fused into the next row-owner stage ----------------------------------------------------------------------------

def _run(s, nd, iters, freq=1, profile=False):
    s.set_positions(nd.pos)
    s.set_profiling(profile)
    before = s.stage_launches
    s.begin(iters, K0, COOLING, 0.0, 1e-12, 10 ** 9, freq, 5, 1)
    s.run()
    s.sync()
    out = dict(pos=s.get_positions(), trace=s.check_trace().copy(), launches=s.stage_launches - before)
    if profile:
        out["symmetric"] = s.profile_symmetric()
        out["fused"] = s.profile_fused()[1]
    return out


def _trace_against_the_oracle(s, nd, full, iters, what):
    """Trace row q of `full` against the oracle on the device's own positions after q iterations (a rerun with
    n_iter = q, whose trace is first held to be a bit-identical prefix but for its own last row, which a separate pass
    reduced).  Returns the largest |d MAE| / band."""
    worst = 0.0
    kd = _position_dim(s)
    for q in range(1, iters + 1):
        rerun = full if q == iters else _run(s, nd, q)
        assert np.array_equal(rerun["trace"][:q - 1], full["trace"][:q - 1]), what + (q,)
        assert [int(t) for t in rerun["trace"][:, 0]] == list(range(1, q + 1))
        if q == iters:
            assert np.array_equal(_run(s, nd, q)["pos"], full["pos"]), what
        pos = rerun["pos"]
        want = cn.oracle(pos, nd)
        band = cn.sum_band_f32(pos, nd.edge_i, nd.edge_j, nd.edge_dist_dev, nd.edge_thresh, kd)
        for label, mae in (("run", full["trace"][q - 1, 1]), ("rerun", rerun["trace"][q - 1, 1])):
            ok, ratio = cn.mae_holds(mae, want, band)
            assert ok, what + (q, label, mae, want, ratio)
            worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("thresholded", [False, True])
@pytest.mark.parametrize("n,dim", cn.FUSED_CASES)
def test_fused_row_owner_check_against_the_oracle(n, dim, thresholded):
    """Four one-stage row-owner iterations (k0 1.5, c_repulsion 0) with a check after each.  2 050 points (even): checks
    1 to 3 ride on stages 2 to 4 -- the ERR instances of slab_stage_pipe_kernel at the wave budgets of ndim 2, 5, 9 and
    12, the count from ballots with thresholds and from the host (fixed_cnt) without -- and check 4 is a separate pass;
    2 113 points (odd): every check is a separate pass.  No symmetric sweep runs.  With TOPOLOW_FUSE_CHECKS=0: the same
    positions, the trace inside the same band.  Measured on an MI355X, the largest |d MAE| / band per case: 0.001 to 0.008
    (ndim 2), the same with and without fusing."""
    nd = cn.needle(n, dim, cn.SEED, thresholded)
    what = (n, dim, thresholded)
    runs = {}
    for fuse in ("1", "0"):
        s = _session(nd, env=dict(TOPOLOW_FUSE_CHECKS=fuse))
        assert s.uses_dense_mae and s.has_thresholds == thresholded
        assert s.can_fuse_checks == (fuse == "1" and n % 2 == 0)
        full = _run(s, nd, 4, profile=True)
        assert full["launches"] == 4 and full["symmetric"][1] + full["symmetric"][3] == 0, full
        assert full["fused"] == (3 if s.can_fuse_checks else 0), full
        worst = _trace_against_the_oracle(s, nd, full, 4, what + (fuse,))
        print("fused n=%d dim=%d thr=%d fuse=%s: largest |d MAE| / band %.3f" % (n, dim, thresholded, fuse, worst))
        runs[fuse] = full
        s.close()
    assert np.array_equal(runs["1"]["pos"], runs["0"]["pos"]), what


# ---- 3b. more than 1 024 partials in front of the controller --------------------------------------------------------------------

def _one_checked_iteration(s, nd, what):
    """One iteration and its check: final_mae and the trace against the oracle and against Session.edge_error, both on
    the returned positions."""
    s.set_positions(nd.pos)
    s.begin(1, K0, COOLING, 0.0, 1e-12, 10 ** 9, 1, 5, 1)
    s.run()
    trace = s.check_trace().copy()
    res = s.finish()
    assert res.iterations == 1 and trace.shape[0] == 1 and trace[0, 1] == res.final_mae, (what, trace, res)
    want = cn.oracle(res.positions, nd)
    band = cn.sum_band_f32(res.positions, nd.edge_i, nd.edge_j, nd.edge_dist_dev, nd.edge_thresh, _position_dim(s))
    ok, ratio = cn.mae_holds(res.final_mae, want, band)
    assert ok, (what, res.final_mae, want, ratio)
    got = _initial_edge_error(s, res.positions)
    assert got[1] == want[1] and cn.pass_holds(got, want, band)[0], (what, got, want)
    assert res.final_mae == pytest.approx(got[0] / got[1], rel=1e-12)    # the same partials in another order: 2 048 x 2^-53
    return ratio


def test_controller_folds_the_2048_partials_of_the_edge_list_pass():
    """The 4.5-million-edge list as a one-iteration run with a check: controller_kernel reads 2 048 partials, two per
    thread.  Measured on an MI355X: |d MAE| / band 7e-10; the test takes 0.25 s."""
    t0 = time.time()
    nd = cn.full_list(*cn.FULL_LIST, cn.SEED, True)
    s = _session(nd, targets="dev", block=_sparse_block(nd))
    assert not s.uses_dense_mae
    ratio = _one_checked_iteration(s, nd, "list")
    s.close()
    print("controller, 2 048 list partials: |d MAE| / band %.3g, %.2f s" % (ratio, time.time() - t0))


def test_controller_folds_the_1161_partials_of_the_dense_pass():
    """8 200 points: 9 chunks x 129 tile rows = 1 161 partials of the separate dense pass (TOPOLOW_FUSE_CHECKS=0), loaded
    from the list alone; the planted pairs of rows >= 7 296 make the partials of index >= 1 024 non-zero.  Measured on
    an MI355X: |d MAE| / band 0.004; the test takes 0.01 s."""
    t0 = time.time()
    nd = cn.needle(*cn.BIG_DENSE, cn.SEED, True)
    c, _, _ = cn.pair_terms(nd.pos, nd.edge_i, nd.edge_j, nd.edge_dist_dev, nd.edge_thresh)
    part = (nd.edge_i // cn.TILE_ROWS) * 9 + nd.edge_j // cn.CHUNK
    assert (c & (part >= 1024) & (nd.edge_i >= 7296)).sum() >= 50 and part.max() == 1160
    s = _session(nd, env=dict(TOPOLOW_FUSE_CHECKS="0"))
    assert s.uses_dense_mae and not s.can_fuse_checks
    ratio = _one_checked_iteration(s, nd, "dense")
    s.close()
    print("controller, 1 161 dense partials: |d MAE| / band %.3g, %.2f s" % (ratio, time.time() - t0))


# ---- 3c. the push of a row-sharded run ------------------------------------------------------------------------------------------

def test_pushed_partials_of_three_row_blocks_against_the_oracle():
    """run_sharded over the three blocks of 2 113 points, thresholded, seven iterations with a check every third: the
    in-process reduce_push_kernel and the rank table in front of a needle with several chunks.  Every trace row against
    the oracle on the positions of that iteration (reruns of 3 and 6 iterations, their traces bit-identical prefixes).
    Measured on an MI355X: the largest |d MAE| / band 0.001."""
    n, dim = cn.PUSH_CASE
    nd = cn.needle(n, dim, cn.SEED, True)
    ss = [_session(nd, rows=(rb, re_), share=cn.parity_share(nd, rb, re_)) for rb, re_ in _native.shard_rows(n, 3)]
    assert len(ss) == 3 and all(s.uses_dense_mae for s in ss)
    kd = _position_dim(ss[0])

    def run(iters):
        r = _native.run_sharded(ss, nd.pos, iters, K0, COOLING, 0.0, 1e-12, 10 ** 9, 3, 5, 1)
        traces = [s.check_trace().copy() for s in ss]
        assert all(np.array_equal(t, traces[0]) for t in traces)
        return r, traces[0]

    full, trace = run(7)
    assert [int(t) for t in trace[:, 0]] == [3, 6, 7] and full.info["blocks"] == 3
    worst = 0.0
    for row, iters in enumerate((3, 6, 7)):
        r, tr = (full, trace) if iters == 7 else run(iters)
        assert np.array_equal(tr[:row], trace[:row]) and int(tr[-1, 0]) == iters
        # (a run restores its best check's positions; the needle's error falls from check to check: the last one's)
        assert r.final_mae == tr[-1, 1] and tr[-1, 1] == tr[:, 1].min(), tr
        want = cn.oracle(r.positions, nd)
        band = cn.sum_band_f32(r.positions, nd.edge_i, nd.edge_j, nd.edge_dist_dev, nd.edge_thresh, kd)
        for mae in (trace[row, 1], tr[-1, 1]):
            ok, ratio = cn.mae_holds(mae, want, band)
            assert ok, (iters, mae, want, ratio)
            worst = max(worst, ratio)
    for s in ss:
        s.close()
    print("push, three blocks: largest |d MAE| / band %.3f" % worst)
