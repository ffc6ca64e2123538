"""The symmetric sweep at ndim 7..10 (topolow_amd/csrc/relax_symm_wide.h) in its sharded forms and under the CV
session's hold-out (run with -m gpu): the in-process engine over row-block sessions, the eligibility of caller-driven
segments, and folds held out of a resident session."""
import numpy as np
import pytest

from tests import parity_problems as pp
from tests.test_gpu_cv_session import FULL_SYMMETRIC, N, block, fold_edges, full_edges, make_session, problem
from tests.test_gpu_sharded_native import _sessions
from tests.test_gpu_symmetric import _Env
from topolow_amd import _native, synthetic

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dim,thr", [(7, 0.0), (10, 0.15)])
def test_sharded_wide_sweep_equals_the_single_block(dim, thr):
    """2 and 3 row blocks on one device against ONE block (the plain sweep), in the pattern and bands of
    test_sharded_symmetric_sweep_equals_the_single_block: 2e-5 of the coordinate scale per iteration on positions, 2e-6 on
    every check, and the sharded sweep really ran.  2 973 points: the segments cut tile-rows in the middle."""
    n = 2973
    call, _ = pp.random_problem(n, dim, 0.7, seed=40 + dim, thresholds=0.0, n_iter=10, k0=1.5)
    if thr > 0:
        rng = np.random.default_rng(3)
        code = rng.choice([0, 1, -1], size=call.edge_thresh.shape[0], p=[1 - thr, thr / 2, thr / 2])
        call.edge_thresh[:] = code.astype(call.edge_thresh.dtype)
    env = {"TOPOLOW_SYMMETRIC": "1", "TOPOLOW_SYMMETRIC_MIN_N": "0"}
    scale = float(np.abs(call.initial_positions).max())
    iters = 9                                   # checks at 3 and 6 ride on the sweeps of 4 and 7, the last one is separate
    runs = {}
    for blocks in (1, 2, 3):
        ss = _sessions(call, n, dim, blocks, env)
        r = _native.run_sharded(ss, call.initial_positions, iters, 1.5, 0.01, 0.01, 1e-12, 10 ** 9, 3, 5, 1)
        runs[blocks] = (r, ss[0].check_trace())
        for s in ss:
            s.close()
    one, t_one = runs[1]
    assert t_one.shape[0] == 3
    for blocks in (2, 3):
        got, tr = runs[blocks]
        diff = np.abs(got.positions - one.positions).max()
        print(f"ndim={dim} blocks={blocks}: max position difference {diff / scale:.3e} of the scale, checks {tr[:, 1]} / {t_one[:, 1]}")
        assert got.info["symmetric_segments"] == blocks                  # the sharded sweep really ran
        assert diff <= 2e-5 * scale * iters, blocks
        assert tr.shape == t_one.shape and np.array_equal(tr[:, 0], t_one[:, 0])
        assert np.allclose(tr[:, 1], t_one[:, 1], rtol=2e-6, atol=0), (blocks, tr[:, 1], t_one[:, 1])
        assert got.iterations == one.iterations and got.final_mae == pytest.approx(one.final_mae, rel=2e-6)
    assert one.info["symmetric_segments"] == 0


def test_segment_eligibility_at_ndim_10():
    """Caller-driven segments: an fp32 ndim-10 session above the size gate is eligible, an f64 one is not, nor is the
    fp32 one below the gate."""
    n, dim = 1000, 10
    call, _ = pp.random_problem(n, dim, 0.7, seed=9, n_iter=3, k0=1.5)

    def eligible(precision, min_n):
        with _Env(TOPOLOW_SYMMETRIC="1", TOPOLOW_SYMMETRIC_MIN_N=str(min_n)):
            s = _native.Session(n, dim, precision=precision)
        s.load_coo(call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh, call.degrees)
        out = s.symm_segment_eligible(2)
        s.close()
        return out
    assert eligible("f32", 1000) is True
    assert eligible("f64", 1000) is False
    assert eligible("f32", 1001) is False


def _run(s, init, n_iter=40, seed=77):
    """A whole run (multi-stage iterations as pair splits, one-stage iterations as the sweep, checks every iteration)
    and how many of its iterations ran as one sweep + apply."""
    s.set_positions(init)
    s.set_profiling(True)
    s.begin(n_iter, 5.0, 0.02, 0.01, 1e-4, 5, 1, seed)
    s.run()
    trace = s.check_trace().copy()
    counts = s.profile_symmetric()
    res = s.finish()
    s.set_profiling(False)
    return res, trace, counts[1] + counts[3]


def _same_run(a, b):
    (ra, ta, sa), (rb, tb, sb) = a, b
    assert np.array_equal(ra.positions, rb.positions)
    assert np.array_equal(ta, tb) and ta.shape[0] >= 5
    assert (ra.converged, ra.iterations, ra.final_mae, ra.final_k) == (rb.converged, rb.iterations, rb.final_mae, rb.final_k)
    assert sa == sb


@pytest.mark.parametrize("which", ["plain", "thresholds"])
def test_fold_held_out_of_an_ndim_10_session(monkeypatch, which):
    """The hold-out patches the sweep's tile-major copy in place (203 points: four tile-rows, held-out pairs in the last,
    partial one): the run with the fold held out equals a fresh session loaded with the fold's edge list bit for bit;
    after the restore a full-matrix run equals the run made before the hold-out bit for bit."""
    ndim = 10
    p = problem()
    h = p["holds"][which]
    init = synthetic.initial_positions(np.full((N, N), 6.0), ndim, 3)
    s = make_session(monkeypatch, "f32", "slab", ndim, FULL_SYMMETRIC, full_edges(p), p["deg"])
    fresh = make_session(monkeypatch, "f32", "slab", ndim, FULL_SYMMETRIC, fold_edges(p, h), h["deg"])
    try:
        before = _run(s, init)                       # (the sweep's copy exists when the fold arrives: patched, not rebuilt)
        assert before[2] > 0                         # iterations of this run took the sweep
        s.hold_out(h["pi"], h["pj"], h["deg"])
        assert np.array_equal(block(s), block(fresh))
        held = _run(s, init)
        assert held[2] > 0
        _same_run(held, _run(fresh, init))
        got = s.score_pairs(h["pi"], h["pj"], h["truth"])
        pos = held[0].positions
        want = np.abs(h["truth"] - np.linalg.norm(pos[h["pi"]] - pos[h["pj"]], axis=1)).sum()
        assert got[1] == h["pi"].size and got[0] == pytest.approx(want, rel=1e-12)
        s.restore_held_out(p["deg"])
        _same_run(_run(s, init), before)
    finally:
        s.close()
        fresh.close()
