"""The strip loops of symm_apply_kernel (topolow_amd/csrc/relax_symm.h): column sums of the tile-rows above a point's
own and row sums of its tile-row's units, each summed by 16 parts that take every 16th strip (run with -m gpu).  Written
when the strips were tried in batches of four loads (the shapes are the smallest at which such a batch is full, ragged or
repeated); the plain loops stayed, and the cases hold for them as they would for any other way of walking the strips.

4 200 points are 66 tile-rows, so a point of the last tile-row has 65 tile-rows above it: part 0 walks five column strips,
the other parts four.  On 256 workgroups tile-row 0 is cut into more than thirty units: a part walks two row strips.  The
needle cases put ONE measured pair where exactly one strip of one part carries its sum; the dense cases run every strip
of every point against the CPU model of tests/test_gpu_symmetric.py, in that file's bands."""
import dataclasses
import functools

import numpy as np
import pytest

from tests import parity_problems as pp
from tests.test_gpu_symmetric import (_Env, _decode_rounded, _model_iterations, _multi_stage_model, _symmetric_session,
                                      _with_thresholds)
from topolow_amd import _native, core

pytestmark = pytest.mark.gpu

N, GRID = 4200, 256
K0, COOLING = 1.5, 0.01
LAST = 65                                             # the last tile-row: points 4160 .. 4199


def _row0_units():
    units = _native.symm_plan(N, 4 * GRID)[0]
    return units[units[:, 0] == 0]


def _expect_grid(s):
    assert s.symm_grid == GRID, s.symm_grid


def test_the_shape_has_five_column_strips_and_two_row_strips():
    """(host only in effect: the library's plan query)  66 tile-rows; tile-row 0 in more than 17 units, fewer than 64."""
    units = _native.symm_plan(N, 4 * GRID)[0]
    assert int(units[:, 0].max()) == LAST
    assert 18 <= _row0_units().shape[0] <= 63


def _one_pair_call(lo, hi, dim):
    """Positions 3 N(0, 1) rounded to fp32, one measured pair (lo, hi) with target half its distance, no repulsion: the
    two points move towards each other, nothing else moves."""
    rng = np.random.default_rng([lo, hi, dim])
    pos = (3.0 * rng.standard_normal((N, dim))).astype(np.float32).astype(np.float64)
    pos[hi] = pos[lo] + 40.0                              # far apart
    ei, ej = np.array([lo], dtype=np.int32), np.array([hi], dtype=np.int32)
    target = 0.5 * np.sqrt(((pos[ei] - pos[ej]) ** 2).sum(-1))
    D = np.full((N, N), np.inf)
    T = np.zeros((N, N), dtype=np.int32)
    D[ei, ej] = D[ej, ei] = target
    np.fill_diagonal(D, 0.0)
    degrees = np.isfinite(D).sum(axis=1).astype(np.int32)
    call = core.LayoutCall(initial_positions=pos, dissimilarity_matrix=D, threshold_matrix=T, degrees=degrees, edge_i=ei,
                           edge_j=ej, edge_dist=target, edge_thresh=np.zeros(1, dtype=np.int32), n_iter=1, k0=K0,
                           cooling_rate=COOLING, c_repulsion=0.0, relative_epsilon=1e-12, convergence_window=10 ** 9,
                           convergence_check_freq=3, verbose=False)
    return call, dataclasses.replace(call, dissimilarity_matrix=_decode_rounded(call))


def _needle(lo, hi, precision):
    dim = 2
    call, call_r = _one_pair_call(lo, hi, dim)
    start = call.initial_positions
    want = _model_iterations(call_r, 1, K0, COOLING, 0.0)[0]
    moved = np.flatnonzero((want != start).any(axis=1)).tolist()
    assert moved == [lo, hi]
    got, _, counts = _symmetric_session(call, N, dim, 1, K0, COOLING, 0.0, 3, profile=True, precision=precision,
                                        env=dict(TOPOLOW_SYMMETRIC_GRID=str(GRID)), after_run=_expect_grid)
    assert counts[1] + counts[3] == 1
    idle = np.ones(N, dtype=bool)
    idle[[lo, hi]] = False
    assert np.array_equal(got[idle], start[idle]), np.flatnonzero((got != start).any(axis=1) & idle)[:8]
    scale = np.abs(want - start).max()
    assert scale > 1.0                                     # the pair's move: a lost or doubled strip is an error of this size
    err = np.abs(got - want).max()
    print("pair (%d, %d) %s: error %.3g of the move" % (lo, hi, precision, err / scale))
    assert err <= (1e-12 if precision == "f64" else 5e-5) * scale, err / scale


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("tile_row", [0, 15, 16, 63, 64, 65])
def test_one_pair_whose_column_sum_lies_in_one_tile_row(tile_row, precision):
    """The pair (64 R + 9, a point of the last tile-row): the second point's move is the column sum of tile-row R --
    strip 0 of part 0 and of part 15, strip 1 of part 0, the fourth and last strip of part 15, the fifth strip that only
    part 0 has (R = 64) -- and for R = 65 the pair lies in the diagonal square, whose column sums nobody reads:
    both moves arrive as row sums."""
    lo = 64 * tile_row + 9
    hi = 64 * LAST + (7 * tile_row) % 40                   # both column blocks of the last tile-row take their turn (R = 16: the second)
    assert lo < hi < N and hi // 64 == LAST
    _needle(lo, hi, precision)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("unit", [0, 15, 16, 17, -1])
def test_one_pair_whose_row_sum_lies_in_one_unit_of_tile_row_0(unit, precision):
    """The pair (a point of tile-row 0, a point of the unit's first column block): the first point's move is the row sum of
    that unit -- strip 0 of part 0 and of part 15, strip 1 of parts 0 and 1, and the last unit's."""
    _, j0, j1, _ = _row0_units()[unit].tolist()
    lo, hi = 3, 32 * j0 + 5                                # (unit 0: inside the diagonal square)
    assert lo < hi < N and j0 < j1
    _needle(lo, hi, precision)


@functools.lru_cache(maxsize=1)
def _dense_problem(n, dim):
    call, _ = pp.random_problem(n, dim, 0.7, seed=400 + n % 50 + dim, n_iter=4, k0=K0)
    return call


@functools.lru_cache(maxsize=1)
def _dense_case(n, dim, thr, stages):
    call = _with_thresholds(_dense_problem(n, dim), thr)
    call_r = dataclasses.replace(call, dissimilarity_matrix=_decode_rounded(call))
    if stages == 1:
        want = _model_iterations(call_r, 2, K0, COOLING, 0.01)[-1]
    else:
        want = _multi_stage_model(call_r, 2, 2.0 * stages, COOLING, 0.01, 5, stages)[-1]
    want.setflags(write=False)
    return call, want


DENSE = [(N, dim, thr, stages) for dim in (2, 5) for thr in (0.0, 0.15) for stages in (1, 2, 4)]
DENSE += [(N + 1, dim, 0.15, stages) for dim in (2, 5) for stages in (1, 4)]


@pytest.mark.parametrize("n,dim,thr,stages,precision", [c + (p,) for c in DENSE for p in ("f32", "f64")])
def test_dense_problem_against_the_model(n, dim, thr, stages, precision):
    """Two iterations of one, two or four stages (the stage applies sum the window [rp0, rp1) of the tile-rows above: up
    to 33 of them at two stages, three strips of a part) against the CPU model of exactly that schedule: f64 to 1e-12 of
    the displacement scale per stage, fp32 mean 5e-5 and max 5e-3 of it.  One stage: the check of iteration 1 rides in the
    apply launch of iteration 2.  4 201 points: the last block's `i < n` cuts after its ninth point."""
    call, want = _dense_case(n, dim, thr, stages)
    scale = np.abs(want - call.initial_positions).max()
    if stages == 1:
        got, trace, counts = _symmetric_session(call, n, dim, 2, K0, COOLING, 0.01, 1, profile=True, precision=precision)
        assert counts[1] == 1 and counts[3] == 1
        assert [int(t) for t in trace[:, 0]] == [1, 2]
    else:
        with _Env(TOPOLOW_SYMMETRIC="1", TOPOLOW_SYMMETRIC_MIN_N="0", TOPOLOW_SYMMETRIC_TWO_STAGE="1",
                  TOPOLOW_SYMMETRIC_STAGE_MIN_TILES="0"):
            s = _native.Session(n, dim, precision=precision)
        try:
            s.load_dense(call.dissimilarity_matrix, call.threshold_matrix, call.degrees)
            s.set_edges(call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
            s.set_positions(call.initial_positions)
            s.begin(2, 2.0 * stages, COOLING, 0.01, 1e-12, 10 ** 9, 2, 5, stages)
            s.run()
            s.sync()
            got, launches = s.get_positions(), s.stage_launches
        finally:
            s.close()
        assert launches == 2 * stages
    err = np.abs(got - want)
    print("n=%d dim=%d thr=%g stages=%d %s: max %.3g mean %.3g of the scale" % (n, dim, thr, stages, precision,
                                                                             err.max() / scale, err.mean() / scale))
    if precision == "f64":
        assert err.max() <= 1e-12 * scale * 2 * stages, err.max() / scale
    else:
        assert err.mean() <= 5e-5 * scale and err.max() <= 5e-3 * scale, (err.mean() / scale, err.max() / scale)
