"""The symmetric sweep at ndim 7..10 (topolow_amd/csrc/relax_symm_wide.h) on plans shaped like production's, at 200 and
1 000 points (run with -m gpu): what tests/test_gpu_symmetric_long_runs.py and tests/test_gpu_symmetric_priority.py state
for the kernels of ndim 2..6, with that file's helpers, bands and needle problem.

The wide kernel shares plans, records and apply kernels with relax_symm.h; the sweep itself is its own code, and so is
everything it carries from one tile or unit of a wave's run to the next: the tile-row's 64 row records rewritten into LDS
at every unit, the row sums reset and stored per unit, the first-half words requested a tile ahead, the next column block's
records handed into the LDS half J & 1 (also from a unit that starts on an odd J0), the next unit's descriptor, the ERR
partial and count folded per unit, the diagonal test for a unit that starts in the middle of a tile-row, the column partials
at R - col_row0 in stage plans, the priority steps across units.  On a resident grid a wave has one tile or none below a
few thousand points and none of that is used; TOPOLOW_SYMMETRIC_GRID gives one or three workgroups runs of several units.
All sessions are fp32 (the wide sweep has no f64 form: tests/test_gpu_symmetric_wide.py pins that)."""
import numpy as np
import pytest

from tests.test_gpu_symmetric_long_runs import (LONG_RUNS, _against_the_model, _assert_long_runs, _dense_case,
                                                _needle_on_the_whole_triangle, _needle_over_segments,
                                                _needle_through_the_stages, _stage_iterations_against_the_model)
from tests.test_gpu_symmetric_priority import _priority_levels, _six_iterations
from topolow_amd import _native, core, synthetic

pytestmark = pytest.mark.gpu

# column-partial stores: one b128 + three b32 at ndim 7, two b128 at 8, two b128 + one b32 at 9, two b128 + two b32 at 10;
# row-pair reads of 5, 5, 6 and 6 LDS pieces; both threshold instances
WIDE_DIM_THR = [(7, 0.15), (8, 0.0), (9, 0.15), (10, 0.0), (10, 0.15)]


# ----------------------------------------------------------------------------------------
# A. dense problems against the model
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,g,dim,thr", [(n, g, dim, thr) for n in (200, 1000) for dim, thr in WIDE_DIM_THR
                                         for n_, g in LONG_RUNS if n_ == n])
def test_wide_dense_problems_on_long_runs_against_the_model(n, g, dim, thr):
    """The plans of test_dense_problems_on_long_runs_against_the_model (they do not depend on ndim): one and seven
    one-stage iterations against the f64 model in the fp32 bands, the checks of 3 and 6 on the sweeps of 4 and 7 to 2e-5,
    the unprofiled rerun bit for bit."""
    _assert_long_runs(n, g)
    call, want = _dense_case(n, dim, thr)
    _against_the_model(call, want, n, dim, "f32", g, 0.01, "wide dense n=%d dim=%d thr=%g" % (n, dim, thr))


# ----------------------------------------------------------------------------------------
# B. the needle problem on the whole triangle
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim,thresholded", [(n, dim, t) for n, dims in ((200, (7, 8, 9, 10)), (1000, (7, 10)))
                                               for dim in dims for t in (False, True)])
def test_wide_needle_problem_one_pair_is_an_error_of_order_one(n, dim, thresholded):
    """test_needle_problem_one_pair_is_an_error_of_order_one at ndim 7..10: seeds 0..2, one and three workgroups, (i) and
    (ii) of _idle_and_moved after one iteration, the dense bands and every check's MAE after seven.  The band is that
    test's: the model's own fp32 arithmetic against its f64 on this generator at ndim 7..10 gives 0.047 to 0.094 of it
    (0.049 to 0.104 at ndim 5 and 6), with 10 - 24 % of the points idle and 67 - 87 % active.
    Measured on an MI355X, the largest error / band of (ii) per case (three seeds, both grids), plain / thresholded:
    200 points 0.079 / 0.077 (ndim 7), 0.054 / 0.062 (8), 0.047 / 0.068 (9), 0.062 / 0.068 (10); 1 000 points
    0.075 / 0.091 (ndim 7), 0.067 / 0.071 (10)."""
    _needle_on_the_whole_triangle(n, dim, thresholded, "f32")


# ----------------------------------------------------------------------------------------
# C. multi-stage iterations on capped stage plans
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("stages,dim,thr", [(2, 7, 0.15), (4, 10, 0.0), (8, 10, 0.15), (8, 8, 0.0)])
def test_wide_multi_stage_iterations_on_long_runs_against_the_model(stages, dim, thr):
    """1 000 points on one workgroup: four S-stage iterations against the model of that schedule in the fp32 bands of
    test_multi_stage_iterations_on_long_runs_against_the_model, the checks of 2 and 4 to 2e-5."""
    _stage_iterations_against_the_model(stages, dim, thr, "f32")


@pytest.mark.parametrize("dim", [7, 10])
@pytest.mark.parametrize("stages", [2, 8])
def test_wide_needle_problem_through_the_stages_of_one_iteration(stages, dim):
    """test_needle_problem_through_the_stages_of_one_iteration at ndim 7 and 10: a point without a spring partner in any
    stage has not moved after all S stages (a column partial of another stage's tile-row -- a wrong col_row0 -- added by
    mistake moves it), every other point is where the model of the schedule puts it.
    Measured on an MI355X, largest error / band of (ii) over three seeds: S = 2: 0.104 (ndim 7) and 0.095 (ndim 10);
    S = 8: 0.162 and 0.175."""
    _needle_through_the_stages(stages, dim, "f32")


# ----------------------------------------------------------------------------------------
# D. sharded segments on one device
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("thread_per_block", ["0", "1"])
@pytest.mark.parametrize("blocks", [2, 3])
@pytest.mark.parametrize("dim,thresholded", [(7, False), (10, True)])
def test_wide_needle_problem_over_sharded_segments(dim, thresholded, blocks, thread_per_block, monkeypatch):
    """test_needle_problem_over_sharded_segments at ndim 7 and 10: 1 000 points over two and three row-block sessions on
    one device, every segment on one workgroup; (i) and (ii) after one iteration, part A's bands and every check's MAE
    after seven.
    Measured on an MI355X, largest error / band of (ii): 0.078 and 0.073 (ndim 7, plain, two and three blocks), 0.051 and
    0.057 (ndim 10, thresholded), the same with and without a thread per block."""
    monkeypatch.setenv("TOPOLOW_SHARD_THREAD_PER_BLOCK", thread_per_block)
    _needle_over_segments(dim, thresholded, blocks, thread_per_block)


# ----------------------------------------------------------------------------------------
# E. the issue priority changes no bit
# ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def problem_ndim_8():
    """The 2 048-point problem of tests/test_gpu_symmetric_priority.py at latent_dim and ndim 8, from its start."""
    prob = synthetic.make_problem(2048, latent_dim=8, missing=0.7, seed=3)
    init = synthetic.initial_positions(prob.dissimilarity, 8, 3)
    call = core.prepare_layout_call(prob.dissimilarity, 8, 30, 5.0, 0.01, 0.01, 1e-4, 5, init, False, 3, True)
    return call, call.initial_positions


@pytest.mark.parametrize("grid", [None, 8], ids=["resident", "grid8"])
@pytest.mark.parametrize("stages", [1, 2])
def test_wide_priority_by_work_left_leaves_every_bit_as_it_was(problem_ndim_8, stages, grid):
    """test_priority_by_work_left_leaves_every_bit_as_it_was at ndim 8: six iterations with a check after each, one- and
    two-stage, positions and check trace equal bit for bit with the priority on (TOPOLOW_SYM_PRIO unset) and off ("0").
    On 8 workgroups a run is 33 tiles of the whole triangle and 16 or 17 of a stage: every wave steps through all four
    levels, across its units."""
    n, dim = 2048, 8
    call, start = problem_ndim_8
    if grid is not None:
        for which in ([{}] if stages == 1 else [dict(stages=2, stage=st) for st in range(2)]):
            units, wave_first = _native.symm_plan(n, 4 * grid, **which)
            done = np.concatenate([[0], np.cumsum(units[:, 2] - units[:, 1])])
            run_tiles = np.diff(done[wave_first])
            assert set(run_tiles.tolist()) <= ({33} if stages == 1 else {16, 17})
            assert all(_priority_levels(int(t)) == {0, 1, 2, 3} for t in run_tiles)
            assert stages == 2 or np.diff(wave_first).max() >= 2      # whole triangle: ... and across unit boundaries
    pos_on, trace_on, launches_on = _six_iterations(call, start, stages, None, grid, n=n, dim=dim)
    pos_off, trace_off, launches_off = _six_iterations(call, start, stages, "0", grid, n=n, dim=dim)
    assert launches_on == launches_off == 6 * stages
    assert len(trace_on) == 6
    assert np.isfinite(pos_on).all() and np.abs(pos_on - start).max() > 0
    assert np.array_equal(pos_on, pos_off)
    assert np.array_equal(trace_on, trace_off)
