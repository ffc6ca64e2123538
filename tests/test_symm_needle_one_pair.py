"""The needle assertions of tests/test_gpu_symmetric_long_runs.py and tests/test_gpu_symmetric_wide_long_runs.py can
see ONE pair (host only: the library's plan query and the CPU model, no GPU): positions that differ from the model's by a
single lost spring pair, or by one end's share of a pair counted twice, fall out of _idle_and_moved's fp32 band."""
import numpy as np
import pytest

from tests.models import slab_model
from tests.test_gpu_symmetric import _model_iterations
from tests.test_gpu_symmetric_long_runs import _CELLS, COOLING, K0, _idle_and_moved, _needle, _plans

N, DIM = 200, 10


@pytest.fixture(scope="module")
def case():
    """The needle problem (200 points, ndim 10, thresholded, seed 0), the model's first iteration, and for every spring
    pair with an end of three spring partners or fewer (141 of the 154, planted cells among them): (i, j, that end, the
    model's iteration without the pair).  The planted cells share the rows 0, 7, 8 and 63 of a tile-row, so a planted
    pair's row end collects partners, up to seven here: no planted pair has three or fewer at BOTH ends, and the end with
    the fewer is the one held to the statement."""
    call, call_r, active = _needle(N, DIM, 0, True, "whole", (1, 3))
    start = call.initial_positions
    want = _model_iterations(call_r, 1, K0, COOLING, 0.0)[0]
    ei, ej, code = call.edge_i, call.edge_j, call.edge_thresh
    r0 = np.sqrt(((start[ei] - start[ej]) ** 2).sum(-1))
    spring = (code == 0) | ((code == 1) & (call.edge_dist > r0)) | ((code == -1) & (call.edge_dist < r0))
    partners = np.bincount(ei[spring], minlength=N) + np.bincount(ej[spring], minlength=N)
    assert np.array_equal(partners > 0, active)
    planted = {(64 * R + r, 32 * J + c) for units in _plans(N, "whole", (1, 3)) for R, j0, j1, _ in units.tolist()
               for J in {j0, j1 - 1} for r, c in _CELLS}
    pairs = []
    for i, j in zip(ei[spring].tolist(), ej[spring].tolist()):
        end = i if partners[i] <= partners[j] else j
        if partners[end] > 3:
            continue
        # the model without that pair: its cell unmeasured, the degrees (and with them every other pair's share) as they were
        D = call_r.dissimilarity_matrix.copy()
        D[i, j] = D[j, i] = np.inf
        lost = slab_model.stage(start, D, call_r.threshold_matrix, call_r.degrees, [[0, N]], K0, 0.0, "f64")
        assert np.flatnonzero((lost != want).any(axis=1)).tolist() == [i, j]
        pairs.append((i, j, end, lost))
    assert len(pairs) >= 50 and sum((i, j) in planted for i, j, _, _ in pairs) >= 5
    assert {int(partners[end]) for _, _, end, _ in pairs} == {1, 2, 3}
    return start, active, want, pairs


def test_the_model_itself_is_inside_the_band(case):
    start, active, want, _ = case
    assert _idle_and_moved(want, want, start, active, "f32") == 0.0


def test_one_lost_pair_is_outside_the_band(case):
    start, active, want, pairs = case
    for i, j, _, lost in pairs:
        with pytest.raises(AssertionError):
            _idle_and_moved(lost, want, start, active, "f32")


def test_one_pair_doubled_at_one_end_is_outside_the_band(case):
    start, active, want, pairs = case
    for i, j, end, lost in pairs:
        doubled = want.copy()
        doubled[end] += want[end] - lost[end]        # that end's half of the pair's move once more; the other end as it was
        assert np.flatnonzero((doubled != want).any(axis=1)).tolist() == [end]
        with pytest.raises(AssertionError):
            _idle_and_moved(doubled, want, start, active, "f32")
