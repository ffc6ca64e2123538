"""The symmetric sweep (csrc/relax_symm.h, csrc/relax_symm64.h) on plans shaped like production's, at 200 and 1 000 points
(run with -m gpu).  The same for the fp32 kernel of ndim 7..10 (csrc/relax_symm_wide.h), with this file's helpers:
tests/test_gpu_symmetric_wide_long_runs.py; that the needle assertions see one pair: tests/test_symm_needle_one_pair.py.

A resident grid is 2 048 waves, so a problem of a few thousand points gives every wave one tile: nothing the kernels carry
from one tile or unit to the next (the prefetched words and records, the two LDS slots, the row sums kept along a unit, the
ERR partial folded per unit, the next unit's descriptor, the priority steps) is ever used.  TOPOLOW_SYMMETRIC_GRID caps the
grid: one workgroup (4 waves) over the 20 tiles of 200 points or the 272 tiles of 1 000 gives runs of several units of up
to 32 tiles, as config 4 gives a resident wave (tests/test_symm_plan.py pins these shapes).  Every capped session asserts
the grid it ran on (Session.symm_grid) and, from the host's plan query, the shape of the plan.

Two kinds of problem: the dense ones of tests/test_gpu_symmetric.py against the f64 CPU model in that file's bands, and a
sparse "needle" problem with c_repulsion = 0, on which an unmeasured or satisfied pair contributes exactly nothing, a point
has a handful of partners at the most, and one lost, doubled or misplaced pair is an error of the order of the move."""
import dataclasses
import functools

import numpy as np
import pytest

from oracle import topolow_oracle as orc
from tests import parity_problems as pp
from tests.test_gpu_sharded_native import _sessions
from tests.test_gpu_symmetric import (_Env, _decode_rounded, _model_iterations, _multi_stage_model, _symmetric_session,
                                      _with_thresholds)
from topolow_amd import _native, core

pytestmark = pytest.mark.gpu

K0, COOLING = 1.5, 0.01
DIM_THR = [(2, 0.0), (2, 0.15), (3, 0.15), (4, 0.0), (5, 0.0), (5, 0.15), (6, 0.0), (6, 0.15)]
LONG_RUNS = [(200, 1), (1000, 1), (1000, 3)]       # (points, workgroups): the smallest with the shape asserted below


def _grid_env(g):
    return dict(TOPOLOW_SYMMETRIC_STAGE_MIN_TILES="0", TOPOLOW_SYMMETRIC_GRID=str(g))


def _shape(n, g, **which):
    units, wave_first = _native.symm_plan(n, 4 * g, **which)
    length = (units[:, 2] - units[:, 1]).astype(int)
    done = np.concatenate([[0], np.cumsum(length)])
    return dict(longest=int(length.max()), run_units=np.diff(wave_first), run_tiles=np.diff(done[wave_first]))


def _assert_long_runs(n, g):
    """The whole-triangle plan of n points on g workgroups is production-shaped: a unit of five tiles or more (the tile
    loop's steady state, not only its first and last trip), a run of two units or more (the hand-over between units),
    every wave at work."""
    sh = _shape(n, g)
    assert sh["longest"] >= 5 and sh["run_units"].max() >= 2 and sh["run_tiles"].min() >= 1, sh


def _expect_grid(g):
    def look(s):
        assert s.symm_grid == g, (s.symm_grid, g)
    return look


def _read_only(*arrays):
    for a in arrays:
        a.setflags(write=False)


# ----------------------------------------------------------------------------------------
# A. dense problems against the model, both precisions
# ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _dense_case(n, dim, thr):
    """The problem of test_symmetric_sweep_f64_equals_the_model_to_rounding and seven one-stage iterations of the model."""
    call, _ = pp.random_problem(n, dim, 0.7 if n > 100 else 0.3, seed=190 + n % 50 + dim, n_iter=7, k0=K0)
    call = _with_thresholds(call, thr)
    call_r = dataclasses.replace(call, dissimilarity_matrix=_decode_rounded(call))
    want = _model_iterations(call_r, 7, K0, COOLING, 0.01)
    _read_only(*want)
    return call, want


def _against_the_model(call, want, n, dim, precision, g, c_rep, label):
    """One and seven one-stage iterations (check_freq 3: the checks of 3 and 6 ride on the sweeps of 4 and 7) in the bands
    of tests/test_gpu_symmetric.py: f64 positions to 1e-12 of the displacement scale per iteration and every check to
    1e-11 of the oracle's edge error of the model's positions; fp32 mean 5e-5 and max 5e-3 of the scale, checks to 2e-5;
    every iteration a symmetric sweep, two of them ERR instances; the unprofiled rerun gives the same bits."""
    f64 = precision == "f64"
    scale = np.abs(want[-1] - call.initial_positions).max()
    out = {}
    for iters in (1, 7):
        got, trace, counts = _symmetric_session(call, n, dim, iters, K0, COOLING, c_rep, 3, profile=True,
                                                precision=precision, env=_grid_env(g), after_run=_expect_grid(g))
        assert counts[1] + counts[3] == iters, counts
        err = np.abs(got - want[iters - 1])
        print("%s %s g=%d iters=%d: max %.3g mean %.3g of the scale" % (label, precision, g, iters, err.max() / scale,
                                                                        err.mean() / scale))
        if f64:
            assert err.max() <= 1e-12 * scale * iters, err.max() / scale
        else:
            assert err.mean() <= 5e-5 * scale and err.max() <= 5e-3 * scale, (err.mean() / scale, err.max() / scale)
        if iters == 7:
            assert counts[3] == 2
            assert [int(t) for t in trace[:, 0]] == [3, 6, 7]
            for row in trace:
                sm, c = orc.edge_error(want[int(row[0]) - 1], call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
                assert row[1] == pytest.approx(sm / c, rel=1e-11 if f64 else 2e-5), (row, sm / c)
        again, trace2, _ = _symmetric_session(call, n, dim, iters, K0, COOLING, c_rep, 3, profile=False,
                                              precision=precision, env=_grid_env(g))
        assert np.array_equal(again, got) and np.array_equal(trace2, trace)
        out[iters] = got
    return out


@pytest.mark.parametrize("n,g,dim,thr,precision", [(n, g, dim, thr, p) for n in (200, 1000) for dim, thr in DIM_THR
                                                   for n_, g in LONG_RUNS if n_ == n for p in ("f32", "f64")])
def test_dense_problems_on_long_runs_against_the_model(n, g, dim, thr, precision):
    """200 points on one workgroup: units of up to five tiles, runs that start in the middle of a tile-row; 1 000 on one:
    68 tiles per run, up to eight units per run, a unit that is a whole 32-tile row; 1 000 on three: run lengths that do
    not divide (22 and 23)."""
    _assert_long_runs(n, g)
    call, want = _dense_case(n, dim, thr)
    _against_the_model(call, want, n, dim, precision, g, 0.01, "dense n=%d dim=%d thr=%g" % (n, dim, thr))


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_a_cap_above_the_resident_grid_changes_nothing(precision):
    """TOPOLOW_SYMMETRIC_GRID only ever lowers the grid: at 10^6 workgroups a session plans, sweeps and returns what it
    does with the variable unset, bit for bit."""
    n, dim = 1000, 5
    call, _ = _dense_case(n, dim, 0.15)
    grids, runs = [], []
    for env in ({}, {"TOPOLOW_SYMMETRIC_GRID": "1000000"}):
        runs.append(_symmetric_session(call, n, dim, 7, K0, COOLING, 0.01, 3, profile=False, precision=precision, env=env,
                                       after_run=lambda s: grids.append(s.symm_grid)))
    assert grids[0] == grids[1] and grids[0] >= 256          # a resident round: a workgroup per CU at the least
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


# ----------------------------------------------------------------------------------------
# B. the needle problem
# ----------------------------------------------------------------------------------------
_CELLS = ((0, 0), (7, 3), (8, 4), (63, 31))        # of a 64 x 32 tile: its corners, and the seam between two lanes' rows / columns


def _plans(n, kind, arg):
    """The unit lists the needle problem takes its planted cells from."""
    if kind == "whole":          # arg: the grids the case runs on
        return [_native.symm_plan(n, 4 * g)[0] for g in arg]
    if kind == "stages":         # arg: S -- the whole triangle and the S stage plans on one workgroup
        return [_native.symm_plan(n, 4)[0]] + [_native.symm_plan(n, 4, stages=arg, stage=st)[0] for st in range(arg)]
    return [_native.symm_plan(n, 4, segment=b, n_segments=arg)[0] for b in range(arg)]       # "segments", arg: blocks


@functools.lru_cache(maxsize=3)
def _needle(n, dim, seed, thresholded, kind, arg):
    """Positions 3 N(0, 1) rounded to fp32; every unordered pair measured with probability 2 / n, plus four cells of the
    first and last tile of every unit of the plans the case runs on (so every unit's first and last trip holds a pair that
    counts); target = distance x 0.5 or x 2, so that t - r never cancels; thresholded: codes exact / ">" / "<" with
    probabilities 1/2, 1/4, 1/4 -- a ">" target below and a "<" target above the distance is satisfied and must count
    neither as a move nor in the MAE.  Returns the call (c_repulsion 0), the call with the targets as the device rounds
    them (for the model) and the mask of the points with a spring partner at the start."""
    rng = np.random.default_rng([n, dim, seed, int(thresholded)])
    pos = (3.0 * rng.standard_normal((n, dim))).astype(np.float32).astype(np.float64)
    M = np.triu(rng.random((n, n)) < 2.0 / n, 1)
    for units in _plans(n, kind, arg):
        for R, j0, j1, _ in units.tolist():
            for J in {j0, j1 - 1}:
                for r, c in _CELLS:
                    i, j = 64 * R + r, 32 * J + c
                    if i < j < n:
                        M[i, j] = True
    cols, rows = np.nonzero(M.T)                     # column-major, as core.prepare_layout_call lists the edges
    ei, ej = rows.astype(np.int32), cols.astype(np.int32)
    r0 = np.sqrt(((pos[ei] - pos[ej]) ** 2).sum(-1))
    factor = rng.choice([0.5, 2.0], size=ei.shape[0])
    target = r0 * factor
    code = (rng.choice([0, 1, -1], size=ei.shape[0], p=[0.5, 0.25, 0.25]) if thresholded
            else np.zeros(ei.shape[0])).astype(np.int32)
    D = np.full((n, n), np.inf)
    T = np.zeros((n, n), dtype=np.int32)
    D[ei, ej] = D[ej, ei] = target
    T[ei, ej] = T[ej, ei] = code
    np.fill_diagonal(D, 0.0)
    degrees = np.isfinite(D).sum(axis=1).astype(np.int32)          # measured cells of the row, the diagonal included
    call = core.LayoutCall(initial_positions=pos, dissimilarity_matrix=D, threshold_matrix=T, degrees=degrees, edge_i=ei,
                           edge_j=ej, edge_dist=target, edge_thresh=code, n_iter=7, k0=K0, cooling_rate=COOLING,
                           c_repulsion=0.0, relative_epsilon=1e-12, convergence_window=10 ** 9, convergence_check_freq=3,
                           verbose=False)
    call_r = dataclasses.replace(call, dissimilarity_matrix=_decode_rounded(call))
    spring = (code == 0) | ((code == 1) & (factor > 1.0)) | ((code == -1) & (factor < 1.0))
    active = np.zeros(n, dtype=bool)
    active[ei[spring]] = True
    active[ej[spring]] = True
    _read_only(pos, D, T, degrees, ei, ej, target, code, active, call_r.dissimilarity_matrix)
    return call, call_r, active


def _idle_and_moved(got, want, start, active, precision):
    """(i) a point without a spring partner is where it started, bit for bit; (ii) every other point against the model:
    fp32 |got_i - want_i| <= 1e-5 |move_i| + 2^-22 |p_i| in the maximum norm -- a term's path is about a dozen fp32
    roundings of 6e-8 (dx, the fma chain, sqrt and rcp to 1 ulp, t - r, two products, ks, the accumulate, the final
    subtraction), 7e-7 of the move, and the stored coordinate rounds once more; a lost, doubled or misplaced pair at a
    point with three partners or fewer is 0.3 of its move or more -- and f64 1e-12 of the displacement scale.  Returns
    the largest error / band."""
    idle = ~active
    assert idle.sum() >= 0.05 * len(active) and active.sum() >= 0.5 * len(active)
    assert np.array_equal(want[idle], start[idle])              # (the model agrees about who has a partner)
    assert np.array_equal(got[idle], start[idle]), np.flatnonzero((got != start).any(axis=1) & idle)[:8]
    err = np.abs(got[active] - want[active]).max(axis=1)
    move = np.abs(want[active] - start[active]).max(axis=1)
    assert move.min() > 0
    if precision == "f64":
        band = np.full_like(err, 1e-12 * move.max())
    else:
        band = 1e-5 * move + 2.0 ** -22 * np.abs(start[active]).max(axis=1)
    ratio = float((err / band).max())
    assert ratio <= 1.0, (ratio, np.flatnonzero(active)[np.argsort(-(err / band))[:8]])
    return ratio


@pytest.mark.parametrize("n,dim,thresholded,precision", [(n, dim, t, p) for n in (200, 1000) for dim in (2, 3, 5, 6)
                                                         for t in (False, True) for p in ("f32", "f64")])
def test_needle_problem_one_pair_is_an_error_of_order_one(n, dim, thresholded, precision):
    """Seeds 0..2, one and three workgroups (200 points on three: twelve waves over twenty tiles, runs of one or two tiles
    that begin anywhere in a tile-row -- not a long-run shape, and not asserted as one): (i) and (ii) of _idle_and_moved
    after one iteration, the bands of part A after seven, every check's MAE against the oracle's edge error (about n
    edges: one lost edge or one wrong count moves it by 1e-3).
    Measured on an MI355X, fp32, the largest error / band of (ii) per case (three seeds, both grids): 0.06 to 0.18 --
    0.179 at (1000, 2, plain), 0.167 at (1000, 3, thresholded), 0.152 at (200, 2, thresholded); the model's own fp32
    arithmetic against its f64 gives 0.05 to 0.19 on the same problems.  f64: 0.001 of its band at the most."""
    _needle_on_the_whole_triangle(n, dim, thresholded, precision)


def _needle_on_the_whole_triangle(n, dim, thresholded, precision):
    """What test_needle_problem_one_pair_is_an_error_of_order_one states, at any ndim; returns the largest error / band."""
    worst = 0.0
    for seed in range(3):
        call, call_r, active = _needle(n, dim, seed, thresholded, "whole", (1, 3))
        want = _model_iterations(call_r, 7, K0, COOLING, 0.0)
        for g in (1, 3):
            if (n, g) in LONG_RUNS:
                _assert_long_runs(n, g)
            else:
                assert _shape(n, g)["run_tiles"].min() >= 1
            got = _against_the_model(call, want, n, dim, precision, g, 0.0, "needle n=%d dim=%d thr=%d seed=%d" %
                                     (n, dim, thresholded, seed))
            worst = max(worst, _idle_and_moved(got[1], want[0], call.initial_positions, active, precision))
    print("needle n=%d dim=%d thr=%d %s: largest error / band %.3f" % (n, dim, thresholded, precision, worst))
    return worst


# ----------------------------------------------------------------------------------------
# C. multi-stage iterations on capped stage plans
# ----------------------------------------------------------------------------------------
def _stage_session(call, n, dim, precision, iters, k0, c_rep, check_freq, seed, stages, g):
    with _Env(TOPOLOW_SYMMETRIC="1", TOPOLOW_SYMMETRIC_MIN_N="0", TOPOLOW_SYMMETRIC_TWO_STAGE="1", **_grid_env(g)):
        s = _native.Session(n, dim, precision=precision)
    s.load_dense(call.dissimilarity_matrix, call.threshold_matrix, call.degrees)
    s.set_edges(call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
    s.set_positions(call.initial_positions)
    s.begin(iters, k0, COOLING, c_rep, 1e-12, 10 ** 9, check_freq, seed, stages)
    s.run()
    s.sync()
    out = s.get_positions(), s.check_trace(), s.stage_launches
    assert s.symm_grid == g
    s.close()
    return out


def _assert_stage_plans(n, g, stages):
    """Every stage plan on g workgroups: runs of several units, every wave at work, and units as long as a stage has
    them -- a stage's interval in a tile-row is one slab wide, 2 TR / S column blocks: 16, 8 and 4 at 1 000 points, so the
    five-tile mark of the whole-triangle plans applies to S = 2 and 4 and an eight-stage unit is at most four tiles."""
    TR = (n + 63) // 64
    _assert_long_runs(n, g)
    for st in range(stages):
        sh = _shape(n, g, stages=stages, stage=st)
        assert sh["longest"] >= min(5, 2 * TR // stages) and sh["run_units"].max() >= 2 and sh["run_tiles"].min() >= 1, sh


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("dim,thr", [(3, 0.0), (5, 0.15), (6, 0.15)])
@pytest.mark.parametrize("stages", [2, 4, 8])
def test_multi_stage_iterations_on_long_runs_against_the_model(stages, dim, thr, precision):
    """1 000 points (the smallest with 16 tile-rows, two per slab of eight) on one workgroup: four S-stage iterations
    against the model of that schedule, in the bands of test_multi_stage_iterations_as_symmetric_sweeps_against_the_model."""
    _stage_iterations_against_the_model(stages, dim, thr, precision)


def _stage_iterations_against_the_model(stages, dim, thr, precision):
    n, g, seed, iters = 1000, 1, 5, 4
    k0 = 2.0 * stages
    _assert_stage_plans(n, g, stages)
    call, _ = pp.random_problem(n, dim, 0.7, seed=300 + n % 50 + dim, n_iter=iters, k0=k0)
    call = _with_thresholds(call, thr)
    call_r = dataclasses.replace(call, dissimilarity_matrix=_decode_rounded(call))
    want = _multi_stage_model(call_r, iters, k0, COOLING, 0.01, seed, stages)
    scale = np.abs(want[-1] - call.initial_positions).max()
    got, trace, launches = _stage_session(call, n, dim, precision, iters, k0, 0.01, 2, seed, stages, g)
    assert launches == iters * stages
    err = np.abs(got - want[-1])
    print("stages=%d dim=%d thr=%g %s: max %.3g mean %.3g of the scale" % (stages, dim, thr, precision, err.max() / scale,
                                                                           err.mean() / scale))
    if precision == "f64":
        assert err.max() <= 1e-12 * scale * iters * stages, err.max() / scale
    else:
        assert err.mean() <= 5e-5 * scale and err.max() <= 5e-3 * scale, (err.mean() / scale, err.max() / scale)
    assert [int(t) for t in trace[:, 0]] == [2, 4]
    for row in trace:
        sm, c = orc.edge_error(want[int(row[0]) - 1], call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
        assert row[1] == pytest.approx(sm / c, rel=1e-11 if precision == "f64" else 2e-5)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("stages", [2, 8])
def test_needle_problem_through_the_stages_of_one_iteration(stages, precision):
    """The thresholded needle problem in five dimensions through ONE S-stage iteration: a point without a spring partner
    has not moved after all S stages (the apply kernel adds only the column partials of this stage's tile-rows; a slot an
    older sweep wrote, added by mistake, moves it), every other point is where the model of the schedule puts it.
    Measured on an MI355X, largest error / band of (ii) over three seeds: fp32 0.098 (S = 2) and 0.187 (S = 8), f64
    0.001."""
    _needle_through_the_stages(stages, 5, precision)


def _needle_through_the_stages(stages, dim, precision):
    """What test_needle_problem_through_the_stages_of_one_iteration states, at any ndim; returns the largest error / band."""
    n, g, seed = 1000, 1, 5
    _assert_stage_plans(n, g, stages)
    worst = 0.0
    for problem_seed in range(3):
        call, call_r, active = _needle(n, dim, problem_seed, True, "stages", stages)
        want = _multi_stage_model(call_r, 1, K0, COOLING, 0.0, seed, stages)[0]
        # a pair satisfied at the start may become a spring once a stage has moved an end of it: the points the model
        # moves are the ones with a partner in some stage (with c_repulsion 0 it leaves the others exactly where they were)
        moved = (want != call.initial_positions).any(axis=1)
        assert not (active & ~moved).any()
        got, _, launches = _stage_session(call, n, dim, precision, 1, K0, 0.0, 3, seed, stages, g)
        assert launches == stages
        worst = max(worst, _idle_and_moved(got, want, call.initial_positions, moved, precision))
    print("needle stages=%d dim=%d %s: largest error / band %.3f" % (stages, dim, precision, worst))
    return worst


# ----------------------------------------------------------------------------------------
# D. sharded segments on one device
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("thread_per_block", ["0", "1"])
@pytest.mark.parametrize("blocks", [2, 3])
@pytest.mark.parametrize("dim,thresholded", [(3, False), (5, True)])
def test_needle_problem_over_sharded_segments(dim, thresholded, blocks, thread_per_block, monkeypatch):
    """1 000 points over two and three row-block sessions on one device (fp32: the sharded sweep has no f64 form), every
    session's segment on one workgroup: 136 or 90 tiles per segment, 34 or 22 - 23 per wave, segments that start in the
    middle of a tile-row.  With c_repulsion 0 neither such a start nor an inbox slot folded twice can hide in a summation
    band: (i) and (ii) after one iteration, part A's fp32 bands and every check's MAE after seven.
    Measured on an MI355X, largest error / band of (ii): 0.112 (ndim 3, plain), 0.050 and 0.070 (ndim 5, thresholded, two
    and three blocks), the same with and without a thread per block."""
    monkeypatch.setenv("TOPOLOW_SHARD_THREAD_PER_BLOCK", thread_per_block)
    _needle_over_segments(dim, thresholded, blocks, thread_per_block)


def _needle_over_segments(dim, thresholded, blocks, thread_per_block):
    """What test_needle_problem_over_sharded_segments states (TOPOLOW_SHARD_THREAD_PER_BLOCK set by the caller), at any
    ndim; returns the largest error / band of (ii)."""
    n, g = 1000, 1
    for b in range(blocks):
        sh = _shape(n, g, segment=b, n_segments=blocks)
        assert sh["longest"] >= 5 and sh["run_units"].max() >= 2 and sh["run_tiles"].min() >= 1, sh
    call, call_r, active = _needle(n, dim, 0, thresholded, "segments", blocks)
    want = _model_iterations(call_r, 7, K0, COOLING, 0.0)
    scale = np.abs(want[-1] - call.initial_positions).max()
    env = {"TOPOLOW_SYMMETRIC": "1", "TOPOLOW_SYMMETRIC_MIN_N": "0", "TOPOLOW_SYMMETRIC_GRID": str(g)}
    for iters in (1, 7):
        ss = _sessions(call, n, dim, blocks, env)
        r = _native.run_sharded(ss, call.initial_positions, iters, K0, COOLING, 0.0, 1e-12, 10 ** 9, 3, 5, 1)
        trace = ss[0].check_trace()
        grids = [s.symm_grid for s in ss]
        for s in ss:
            s.close()
        assert grids == [g] * blocks
        assert r.info["symmetric_segments"] == blocks and r.iterations == iters
        assert r.info["groups"] == (blocks if thread_per_block == "1" else 1)
        got = r.positions
        if iters == 1:
            ratio = _idle_and_moved(got, want[0], call.initial_positions, active, "f32")
            print("needle dim=%d thr=%d blocks=%d threads=%s: largest error / band %.3f" % (dim, thresholded, blocks,
                                                                                         thread_per_block, ratio))
        else:
            err = np.abs(got - want[-1])
            assert err.mean() <= 5e-5 * scale and err.max() <= 5e-3 * scale, (err.mean() / scale, err.max() / scale)
            assert [int(t) for t in trace[:, 0]] == [3, 6, 7]
            for row in trace:
                sm, c = orc.edge_error(want[int(row[0]) - 1], call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
                assert row[1] == pytest.approx(sm / c, rel=2e-5), (row, sm / c)
    return ratio
