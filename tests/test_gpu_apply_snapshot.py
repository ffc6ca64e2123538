"""The best-positions snapshot of a check that rides in an apply's launch (csrc/relax_symm.h, csrc/relax_kernels.h): every
column block copies its 32 points of the check's positions into the snapshot buffer the run state does not name, and the
controller's workgroup only records which buffer holds the best positions (RunState::best_buf).  TOPOLOW_CHECK_IN_APPLY=0
keeps every check in controller_kernel, which copies by itself -- the same run, so positions, trace and result scalars
are compared bit for bit (run with -m gpu)."""
import os

import numpy as np
import pytest

from tests.test_gpu_check_in_apply import ENV, KNOBS, _both, _run
from tests.test_gpu_symmetric import _with_thresholds
from topolow_amd import _native, core, synthetic

pytestmark = pytest.mark.gpu

PRECISIONS = ["f32", "f64"]


@pytest.fixture(scope="module")
def call():
    """2 048 points, ndim 5, 70 % missing, from the initial positions: 64 column blocks, each with 160 values to copy."""
    prob = synthetic.make_problem(2048, latent_dim=5, missing=0.7, seed=3)
    init = synthetic.initial_positions(prob.dissimilarity, 5, 3)
    return core.prepare_layout_call(prob.dissimilarity, 5, 30, 5.0, 0.01, 0.01, 1e-4, 5, init, False, 3, True)


def _improved(trace):
    """Per check: whether its error lies below every earlier check's (the controller then takes the snapshot)."""
    mae = trace[:, 1]
    return np.array([q == 0 or mae[q] < mae[:q].min() for q in range(len(mae))])


# one stage per iteration at k0 = 8, three times what a single stage takes from these positions, cooled by a quarter
# per iteration: the CPU model's MAE goes 13.7, 18.7, 15.1, 4.9, 3.6, 3.0 ... -- the checks 2 and 3 do not improve (the
# entry stays), every other one does (the entry flips)
RISE_AND_FALL = (12, 8.0, 0.25, 0.01, 1e-12, 10 ** 9, 1, 5, 1)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_buffer_index_flips_and_stays_and_the_last_check_is_flushed(call, precision):
    r = _both(call, call.initial_positions, RISE_AND_FALL, precision=precision)
    assert len(r.trace) == 12 and r.in_apply == 11 and not r.stopped       # the 12th check has no apply to ride in: flushed
    better = _improved(r.trace)
    assert better[:11].any() and (~better[1:11]).any(), r.trace[:, 1]      # in-apply checks of both kinds
    assert not better[1] and better[3] and better[10]                      # stays behind a flip, flips behind a stay
    assert better[11]                                                      # the flushed check copies by itself, behind in-apply ones
    assert r.scalars[1] == 12 and r.scalars[2] == r.trace[-1, 1]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_stop_inside_an_apply_launch_leaves_the_snapshot_complete(call, precision):
    """relative_epsilon = 0.5, window = 2: the third check improves AND stops the run, in the apply launch of iteration 4.
    Its snapshot is its siblings' copies; the launches the host had already enqueued behind it (it runs up to three checks
    ahead) carry checks of their own and must leave both buffers alone."""
    r = _both(call, call.initial_positions, (40, 1.5, 0.01, 0.01, 0.5, 2, 1, 5, 1), precision=precision)
    converged, best_iter, best_mae, _k = r.scalars
    assert converged is True and r.stopped and r.iterations_run < 40 and len(r.trace) == r.iterations_run
    assert r.in_apply >= r.iterations_run                                  # the stopping check rode in an apply
    assert int(np.argmin(r.trace[:, 1])) == len(r.trace) - 1               # ... and improved: snapshot and stop in one step
    assert best_iter == r.iterations_run and best_mae == r.trace[-1, 1]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_worsening_stop_keeps_the_older_snapshot(call, precision):
    """k0 = 10 without cooling to speak of: the error grows from the first check on and the third check stops the run
    without a snapshot: what comes back is the first check's, two in-apply launches old."""
    r = _both(call, call.initial_positions, (9, 10.0, 0.01, 0.01, 1e-12, 2, 1, 5, 1), precision=precision)
    assert r.stopped and r.scalars[0] is True and r.scalars[1] == 1 and r.scalars[2] == r.trace[0, 1]
    assert np.all(np.diff(r.trace[:, 1]) > 0), r.trace


@pytest.mark.parametrize("precision", PRECISIONS)
def test_multi_stage_iterations_into_one_stage_ones(call, precision):
    """The adaptive schedule from the initial positions with a check after every iteration: the checks in front of
    multi-stage iterations run in controller_kernel (it copies by itself and leaves both entries equal), the later ones
    ride in the applies of one-stage iterations; 10 % censored targets."""
    c = _with_thresholds(call, 0.1)
    n_iter, k0, cooling = 48, 5.0, 0.03
    k, stages = k0, []
    for it in range(n_iter):
        stages.append(_native.slab_stages_at(it, k, 5))
        k *= 1.0 - cooling
    riding = [i for i in range(1, n_iter) if stages[i] == 1]
    assert max(stages) > 1 and stages[-1] == 1 and len(riding) >= 10
    r = _both(c, c.initial_positions, (n_iter, k0, cooling, 0.01, 1e-12, 10 ** 9, 1, 5, 0), precision=precision)
    assert len(r.trace) == n_iter and r.in_apply == len(riding)
    better = _improved(r.trace)
    assert better[:riding[0]].any() and better[riding[0]:].any()           # snapshots by both kinds of controller


@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_same_session_twice_in_a_row(call, precision):
    """A second begin starts from a clean record: the run of RISE_AND_FALL, a stopped run and RISE_AND_FALL again on ONE
    session give what fresh sessions give."""
    fresh = _run(call, call.initial_positions, True, RISE_AND_FALL, precision=precision)
    old = {k: os.environ.get(k) for k in list(ENV) + list(KNOBS)}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(ENV)
    try:
        s = _native.Session(2048, 5, precision=precision)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    try:
        s.load_dense(call.dissimilarity_matrix, call.threshold_matrix, call.degrees)
        s.set_edges(call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
        for begin in (RISE_AND_FALL, (40, 1.5, 0.01, 0.01, 0.5, 2, 1, 5, 1), RISE_AND_FALL, RISE_AND_FALL):
            s.set_positions(call.initial_positions)
            s.begin(*begin)
            s.run()
            trace = s.check_trace()
            res = s.finish()
            if begin is RISE_AND_FALL:
                assert s.checks_in_apply == 11
                assert np.array_equal(res.positions, fresh.positions) and np.array_equal(trace, fresh.trace)
                assert (res.converged, res.iterations, res.final_mae, res.final_k) == fresh.scalars
    finally:
        s.close()
