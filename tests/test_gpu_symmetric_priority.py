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


def _six_iterations(call, start, stages, prio):
    env = dict(TOPOLOW_SYMMETRIC="1", TOPOLOW_SYMMETRIC_MIN_N="0", TOPOLOW_SYMMETRIC_STAGE_MIN_TILES="0")
    if prio is not None:
        env["TOPOLOW_SYM_PRIO"] = prio
    old = {k: os.environ.get(k) for k in list(env) + ["TOPOLOW_SYM_PRIO"]}
    os.environ.pop("TOPOLOW_SYM_PRIO", None)
    os.environ.update(env)
    try:
        s = _native.Session(2048, 5, precision="f32")
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
    s.close()
    return out


@pytest.mark.parametrize("stages", [1, 2])
def test_priority_by_work_left_leaves_every_bit_as_it_was(problem, stages):
    """Six iterations with a check after each, as one-stage iterations (whole-triangle sweeps) and as two-stage ones
    (half sweeps over the stage plans): positions and check trace equal, bit for bit, with and without the priority."""
    call, start = problem
    pos_on, trace_on, launches_on = _six_iterations(call, start, stages, None)
    pos_off, trace_off, launches_off = _six_iterations(call, start, stages, "0")
    assert launches_on == launches_off == 6 * stages
    assert len(trace_on) == 6
    assert np.isfinite(pos_on).all() and np.abs(pos_on - start).max() > 0
    assert np.array_equal(pos_on, pos_off)
    assert np.array_equal(trace_on, trace_off)
