"""The fp32 symmetric sweep's issue priority by work left (csrc/relax_symm.h) changes WHEN a wave's instructions are
issued, never which instructions or in what order a sum is taken: with the priority on (the default) and off
(TOPOLOW_SYM_PRIO=0) a session must return the same bits."""
import os

import numpy as np
import pytest

from topolow_amd import _native, core, synthetic

pytestmark = pytest.mark.gpu


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


def _six_iterations(call, start, stages, prio, grid=None, n=2048, dim=5):
    env = dict(TOPOLOW_SYMMETRIC="1", TOPOLOW_SYMMETRIC_MIN_N="0", TOPOLOW_SYMMETRIC_STAGE_MIN_TILES="0")
    if prio is not None:
        env["TOPOLOW_SYM_PRIO"] = prio
    if grid is not None:
        env["TOPOLOW_SYMMETRIC_GRID"] = str(grid)
    old = {k: os.environ.get(k) for k in list(env) + ["TOPOLOW_SYM_PRIO", "TOPOLOW_SYMMETRIC_GRID"]}
    os.environ.pop("TOPOLOW_SYM_PRIO", None)
    os.environ.pop("TOPOLOW_SYMMETRIC_GRID", None)
    os.environ.update(env)
    try:
        s = _native.Session(n, dim, precision="f32")
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    s.load_dense(call.dissimilarity_matrix, call.threshold_matrix, call.degrees)
    s.set_edges(call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
    s.set_positions(start)
    s.begin(6, 1.5, 0.01, 0.01, 1e-12, 10 ** 9, 1, 5, stages)   # a check after every iteration
    s.run()
    s.sync()
    out = s.get_positions(), s.check_trace(), s.stage_launches
    assert grid is None or s.symm_grid == grid
    s.close()
    return out


def _priority_levels(run_tiles):
    """The priorities a wave with a run of run_tiles tiles sets (csrc/relax_symm.h: 3, 2, 1 while more than 3/4, 1/2,
    1/4 of the run is left, then 0)."""
    lv3, lv2, lv1 = (3 * run_tiles) >> 2, run_tiles >> 1, run_tiles >> 2
    return {3 if left > lv3 else 2 if left > lv2 else 1 if left > lv1 else 0 for left in range(run_tiles, 0, -1)}


@pytest.mark.parametrize("grid", [None, 8], ids=["resident", "grid8"])
@pytest.mark.parametrize("stages", [1, 2])
def test_priority_by_work_left_leaves_every_bit_as_it_was(problem, stages, grid):
    """Six iterations with a check after each, as one-stage iterations (whole-triangle sweeps) and as two-stage ones
    (half sweeps over the stage plans): positions and check trace equal, bit for bit, with and without the priority.
    On a resident grid 2 048 points give a wave one tile or none and the priority is set once; on 8 workgroups (32 waves,
    TOPOLOW_SYMMETRIC_GRID) a run is 33 tiles of the whole triangle and 16 or 17 of a stage, and every wave steps through
    all four levels."""
    call, start = problem
    if grid is not None:
        for which in ([{}] if stages == 1 else [dict(stages=2, stage=st) for st in range(2)]):
            units, wave_first = _native.symm_plan(2048, 4 * grid, **which)
            done = np.concatenate([[0], np.cumsum(units[:, 2] - units[:, 1])])
            run_tiles = np.diff(done[wave_first])
            assert set(run_tiles.tolist()) <= ({33} if stages == 1 else {16, 17})
            assert all(_priority_levels(int(t)) == {0, 1, 2, 3} for t in run_tiles)
    pos_on, trace_on, launches_on = _six_iterations(call, start, stages, None, grid)
    pos_off, trace_off, launches_off = _six_iterations(call, start, stages, "0", grid)
    assert launches_on == launches_off == 6 * stages
    assert len(trace_on) == 6
    assert np.isfinite(pos_on).all() and np.abs(pos_on - start).max() > 0
    assert np.array_equal(pos_on, pos_off)
    assert np.array_equal(trace_on, trace_off)
