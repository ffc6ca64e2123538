"""A convergence check that rode on a one-stage symmetric sweep runs its controller step in one more workgroup of that
iteration's apply launch (csrc/relax_symm.h: SymApplyCheck; csrc/relax_kernels.h: controller_step) instead of a
controller launch of its own on the check stream.  The step is the same code reducing the same partials in the same
order -- 512 threads that each fold two of the 1 024 strided sums as the tree's first level does -- so every comparison
here is the new path against TOPOLOW_CHECK_IN_APPLY=0 in the same build, bit for bit: the returned positions, the check
trace and the result scalars.  Session.checks_in_apply says which path a run's checks took."""
import collections
import os

import numpy as np
import pytest

from oracle import topolow_oracle as orc
from tests import parity_problems as pp
from tests.test_gpu_symmetric import _with_thresholds
from topolow_amd import _native, core, synthetic

pytestmark = pytest.mark.gpu

ENV = dict(TOPOLOW_SYMMETRIC="1", TOPOLOW_SYMMETRIC_MIN_N="0", TOPOLOW_SYMMETRIC_STAGE_MIN_TILES="0")
KNOBS = ("TOPOLOW_CHECK_IN_APPLY", "TOPOLOW_SYMMETRIC_GRID", "TOPOLOW_SERIAL_CHECKS", "TOPOLOW_FUSE_CHECKS")

Run = collections.namedtuple("Run", "positions trace scalars iterations_run stopped in_apply launches grid")


@pytest.fixture(scope="module")
def problem():
    """The 2 048-point problem of __graft_entry__.smoke, late in its schedule (30 slab iterations in)."""
    prob = synthetic.make_problem(2048, latent_dim=5, missing=0.7, seed=3)
    init = synthetic.initial_positions(prob.dissimilarity, 5, 3)
    call = core.prepare_layout_call(prob.dissimilarity, 5, 30, 5.0, 0.01, 0.01, 1e-4, 5, init, False, 3, True)
    res = _native.optimize_layout_exact_arrays(
        call.initial_positions, call.dissimilarity_matrix, call.threshold_matrix, call.degrees,
        call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh, call.n_iter, call.k0,
        call.cooling_rate, call.c_repulsion, call.relative_epsilon, call.convergence_window,
        call.convergence_check_freq, seed=1, schedule="slab")
    return call, res.positions


def _run(call, start, in_apply, begin, precision="f32", grid=None, drive=None):
    """One session run; begin = (n_iter, k0, cooling, c_rep, eps, window, check_freq, seed, stages); drive(session)
    enqueues the run (default: Session.run)."""
    n, dim = start.shape
    env = dict(ENV)
    if not in_apply:
        env["TOPOLOW_CHECK_IN_APPLY"] = "0"
    if grid is not None:
        env["TOPOLOW_SYMMETRIC_GRID"] = str(grid)
    old = {k: os.environ.get(k) for k in list(ENV) + list(KNOBS)}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        s = _native.Session(n, dim, precision=precision)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    s.load_dense(call.dissimilarity_matrix, call.threshold_matrix, call.degrees)
    s.set_edges(call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
    s.set_positions(start)
    s.begin(*begin)
    iterations_run, stopped, _mae = s.run() if drive is None else drive(s)
    trace = s.check_trace()
    res = s.finish()
    out = Run(res.positions, trace, (res.converged, res.iterations, res.final_mae, res.final_k), iterations_run, stopped,
              s.checks_in_apply, s.stage_launches, s.symm_grid)
    s.close()
    return out


def _both(call, start, begin, **kw):
    """The run with the check in the apply and with the separate controller: equal bit for bit; returns the first."""
    new, old = _run(call, start, True, begin, **kw), _run(call, start, False, begin, **kw)
    assert old.in_apply == 0
    assert np.array_equal(new.positions, old.positions)
    assert new.trace.shape == old.trace.shape and np.array_equal(new.trace, old.trace)
    assert new.scalars == old.scalars, (new.scalars, old.scalars)
    assert (new.iterations_run, new.stopped) == (old.iterations_run, old.stopped)
    assert new.stopped or new.launches == old.launches   # (after a stop the host enqueues until it has seen it)
    return new


def _mae_is_the_oracles(call, run, rel):
    sm, cnt = orc.edge_error(run.positions, call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
    assert run.scalars[2] == pytest.approx(sm / cnt, rel=rel), (run.scalars, sm / cnt)


def _six(eps=1e-12, window=10 ** 9, k0=1.5, iters=6):
    return (iters, k0, 0.01, 0.01, eps, window, 1, 5, 1)   # a check after every iteration, one stage per iteration


# ---- 1. partial counts on both sides of the tree's first level --------------------------------------------------
@pytest.mark.parametrize("case", ["resident", "grid8", "n200"])
def test_partial_counts_on_both_sides_of_the_first_tree_level(problem, case):
    """The sweep leaves one MAE partial per unit.  2 048 points on a resident grid: one unit per tile, 1 056 of them, so
    the virtual threads 0..31 sum two partials each and both halves of every thread's pair are in use; on 8 workgroups:
    32 runs cut at the tile-rows' ends, fewer than 512 units, so the second virtual thread of every thread sums nothing;
    200 points: a handful.  Six one-stage iterations with a check after each: five ride in an apply, the last is the
    run's final check (a separate pass)."""
    if case == "n200":
        call, _ = pp.random_problem(200, 5, 0.3, seed=41, n_iter=6, k0=1.5)
        start, grid = call.initial_positions, None
    else:
        (call, start), grid = problem, (8 if case == "grid8" else None)
    r = _both(call, start, _six(), grid=grid)
    assert r.in_apply == 5 and r.launches == 6 and len(r.trace) == 6
    assert grid is None or r.grid == grid
    n_units = len(_native.symm_plan(start.shape[0], 4 * r.grid)[0])
    if case == "resident":
        assert 1024 < n_units <= 2048, n_units
    elif case == "grid8":
        assert 32 <= n_units < 512, n_units
    else:
        assert 1 <= n_units <= 20, n_units
    assert np.isfinite(r.positions).all() and np.abs(r.positions - start).max() > 0
    _mae_is_the_oracles(call, r, 2e-5)


# ---- 2. every controller verdict --------------------------------------------------------------------------------
def test_every_check_improves_and_snapshots(problem):
    call, start = problem
    r = _both(call, start, _six())
    assert np.all(np.diff(r.trace[:, 1]) < 0), r.trace          # every check improved: a snapshot each time
    assert r.scalars[0] is False and r.scalars[1] == 6 and r.scalars[2] == r.trace[-1, 1]
    assert r.in_apply == 5 and not r.stopped and r.iterations_run == 6
    _mae_is_the_oracles(call, r, 2e-5)


def test_plateau_stop_returns_the_snapshot(problem):
    """relative_epsilon = 0.5, window = 2: the first check improves on nothing-yet, the second and third count as a
    plateau and the third stops the run -- in the apply of iteration 4, whose siblings and every later launch are
    no-ops: 40 iterations enqueued, 3 run, and what comes back is the snapshot of the best check."""
    call, start = problem
    r = _both(call, start, _six(eps=0.5, window=2, iters=40))
    converged, best_iter, best_mae, _k = r.scalars
    assert converged is True and r.stopped and r.iterations_run == 3 and len(r.trace) == 3
    assert best_iter <= 3 < 40 and best_mae == r.trace[best_iter - 1, 1] == r.trace[:, 1].min()
    assert r.in_apply >= 3
    _mae_is_the_oracles(call, r, 2e-5)


def test_worsening_stop(problem):
    """One stage per iteration at k = 24, eight times what the schedule allows a single stage: every iteration overshoots
    and the error grows from the first check on (0.35, 0.42, 1.6); window = 2: the third check is the second worsening
    one and stops the run; the snapshot is the first check's."""
    call, start = problem
    r = _both(call, start, _six(window=2, k0=24.0, iters=9))
    converged, best_iter, best_mae, _k = r.scalars
    assert np.all(np.isfinite(r.trace)) and np.all(np.diff(r.trace[:, 1]) > 0), r.trace
    assert converged is True and r.stopped and r.iterations_run == 3 and len(r.trace) == 3
    assert best_iter == 1 and best_mae == r.trace[0, 1]
    _mae_is_the_oracles(call, r, 2e-5)


def test_final_check_is_flushed(problem):
    """Seven iterations, a check every third: 3 and 6 ride on the sweeps of 4 and 7 and run in their applies, the check
    of the run's last iteration has no sweep to ride on and is flushed as a separate pass."""
    call, start = problem
    r = _both(call, start, (7, 1.5, 0.01, 0.01, 1e-12, 10 ** 9, 3, 5, 1))
    assert [int(t) for t in r.trace[:, 0]] == [3, 6, 7] and r.in_apply == 2
    assert r.scalars[1] == 7
    _mae_is_the_oracles(call, r, 2e-5)


# ---- 3. thresholds, widths and precisions that share the apply --------------------------------------------------
@pytest.mark.parametrize("dim,precision", [(2, "f32"), (6, "f32"), (8, "f32"), (5, "f64"), (5, "f64_exact")])
def test_threshold_instances_wide_sweep_and_f64(dim, precision):
    """10 % censored targets (the classifying instances) at ndim 2, 6 and 8 (the wide sweep), and the f64 apply, plain
    and exact (the edge list is the block's cells: load_dense + set_edges), on 1 000 points."""
    n = 1000
    call, _ = pp.random_problem(n, dim, 0.7, seed=300 + dim, n_iter=6, k0=1.5)
    call = _with_thresholds(call, 0.1)
    r = _both(call, call.initial_positions, _six(), precision=precision)
    assert r.in_apply == 5 and r.launches == 6 and len(r.trace) == 6
    assert np.isfinite(r.positions).all() and np.isfinite(r.trace).all()
    _mae_is_the_oracles(call, r, 2e-5 if precision == "f32" else 1e-11)


# ---- 4. mixed schedules -----------------------------------------------------------------------------------------
def test_separate_pass_checks_and_in_apply_checks_alternate_in_one_run(problem):
    """The production schedule from the initial positions: sixteen stages while the layout unfolds, two while k > 3,
    then one.  A check every third iteration: those in front of a multi-stage iteration are separate passes beside it
    (check stream), those in front of a one-stage iteration ride in its apply, and the last is flushed."""
    call, _ = problem
    n_iter, k0, cooling, freq = 60, 5.0, 0.02, 3
    k, stages = k0, []
    for it in range(n_iter):
        stages.append(_native.slab_stages_at(it, k, 5))
        k *= 1.0 - cooling
    assert {16, 2, 1} <= set(stages)
    riding = [i for i in range(freq, n_iter, freq) if stages[i] == 1]     # check after iteration i rides on iteration i + 1
    assert 5 <= len(riding) < n_iter // freq - 5
    r = _both(call, call.initial_positions, (n_iter, k0, cooling, 0.01, 1e-12, 10 ** 9, freq, 5, 0))
    assert len(r.trace) == n_iter // freq and [int(t) for t in r.trace[:, 0]] == list(range(freq, n_iter + 1, freq))
    assert r.in_apply == len(riding)
    _mae_is_the_oracles(call, r, 2e-5)


# ---- 5. a session driven in slices ------------------------------------------------------------------------------
def test_pending_check_crosses_slice_boundaries(problem):
    """enqueue(7) / wait() until the run is enqueued, a check every third iteration: the checks after iterations 21 and
    42 of 44 are pending when their slice ends and ride in the first apply of the next one."""
    call, start = problem

    def sliced(s):
        while s.enqueue(7) > 0:
            s.wait()
        return s.sync()

    begin = (44, 1.5, 0.01, 0.01, 1e-12, 10 ** 9, 3, 5, 1)
    whole = _both(call, start, begin)
    parts = _both(call, start, begin, drive=sliced)
    assert whole.in_apply == parts.in_apply == 14 and len(whole.trace) == 15
    assert np.array_equal(whole.positions, parts.positions) and np.array_equal(whole.trace, parts.trace)
    assert whole.scalars == parts.scalars
