"""The symmetric sweep at ndim 7..10 (topolow_amd/csrc/relax_symm_wide.h: fp32, the lane's rows in LDS) -- run with
-m gpu.  The same statements as tests/test_gpu_symmetric.py makes for ndim 2..6, at the sizes where this kernel can go
wrong: phantom rows and columns (n = 33, 66), fewer tiles than waves, ragged n % 32, the diagonal squares met from both
sides; every instance (threshold-free / thresholds x plain / ERR) at the smallest and the largest ndim.  Here a wave has
one tile or none (but for the 7 205-point cases): what the kernel carries from one tile or unit of a run to the next is
held to the model on capped grids, with the needle problem, in tests/test_gpu_symmetric_wide_long_runs.py."""
import dataclasses
import functools

import numpy as np
import pytest

from oracle import topolow_oracle as orc
from tests import parity_problems as pp
from tests.conftest import layout_call_args
from tests.test_gpu_parity import _decode_rounded
from tests.test_gpu_symmetric import (_Env, _model_iterations, _multi_stage_model, _symmetric_session, _with_thresholds,
                                      session_run)
from topolow_amd import _native

pytestmark = pytest.mark.gpu

K0, COOLING, C_REP = 1.5, 0.01, 0.01
INSTANCES = [(7, 0.0), (7, 0.15), (8, 0.0), (9, 0.15), (10, 0.0), (10, 0.15)]


@functools.lru_cache(maxsize=None)
def _problem(n, dim, thr):
    """The problem and the CPU model's positions after 1..7 one-stage iterations (computed once per case)."""
    call, _ = pp.random_problem(n, dim, 0.7 if n > 100 else 0.3, seed=90 + n % 50 + dim, n_iter=7, k0=K0)
    call = _with_thresholds(call, thr)
    call_r = dataclasses.replace(call, dissimilarity_matrix=_decode_rounded(call))
    want = _model_iterations(call_r, 7, K0, COOLING, C_REP)
    for w in want:
        w.setflags(write=False)
    return call, want


def _against_the_model_and_the_oracle(n, dim, thr):
    call, want = _problem(n, dim, thr)
    scale = np.abs(want[-1] - call.initial_positions).max()
    for iters in (1, 7):
        got, trace, counts = _symmetric_session(call, n, dim, iters, K0, COOLING, C_REP, 3, profile=True)
        print(f"n={n} ndim={dim} thr={thr} iters={iters}: symmetric iterations {counts[1]} + {counts[3]}")
        assert counts[1] + counts[3] == iters, counts            # every iteration ran as a symmetric sweep + apply
        err = np.abs(got - want[iters - 1])
        print(f"  position error mean {err.mean() / scale:.3e} max {err.max() / scale:.3e} of the displacement scale")
        assert err.mean() <= 5e-5 * scale and err.max() <= 5e-3 * scale, (err.mean() / scale, err.max() / scale)
        if iters == 7:
            assert counts[3] == 2                                # the checks at 3 and 6 rode on the sweeps of 4 and 7
            assert [int(t) for t in trace[:, 0]] == [3, 6, 7]
            for row in trace:
                s, c = orc.edge_error(want[int(row[0]) - 1], call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
                print(f"  check {int(row[0])}: {row[1]!r} against {s / c!r} (rel {abs(row[1] - s / c) / (s / c):.2e})")
                assert row[1] == pytest.approx(s / c, rel=2e-5), (row, s / c)
        # the unprofiled run (checks beside the next iteration on the second stream) gives the same bits
        again, trace2, _ = _symmetric_session(call, n, dim, iters, K0, COOLING, C_REP, 3, profile=False)
        assert np.array_equal(again, got) and np.array_equal(trace2, trace)


@pytest.mark.parametrize("n", [33, 66, 1000])
@pytest.mark.parametrize("dim,thr", INSTANCES)
def test_wide_sweep_against_the_model_and_the_oracle(n, dim, thr):
    """One and seven one-stage iterations: positions against slab_model.stage in f64 on the rounded targets (the fp32
    band of the project: mean 5e-5, max 5e-3 of the displacement scale); the fused checks of iterations 3 and 6 (ERR
    instance) against orc.edge_error of the positions those sweeps read (rel 2e-5); every iteration as sweep + apply;
    profiled and unprofiled runs bit-identical."""
    _against_the_model_and_the_oracle(n, dim, thr)


def test_wide_sweep_above_the_size_gate_against_the_model_and_the_oracle():
    """n = 7205 (n % 32 = 5, 113 tile-rows: every wave of the resident grid has a run), ndim 10, thresholds."""
    _against_the_model_and_the_oracle(7205, 10, 0.15)


@pytest.mark.parametrize("dim,thresholds", [(7, 0.1), (8, 0.0), (10, 0.1)])
def test_wide_sweep_equals_the_row_owner_sweep(dim, thresholds):
    """Bands of test_symmetric_sweep_equals_the_row_owner_sweep: 2e-5 of the coordinate scale per iteration on positions,
    2e-6 on the fused MAE."""
    n = 7205
    call, _ = pp.random_problem(n, dim, 0.7, seed=50 + dim, thresholds=0.0, n_iter=10, k0=1.5)
    if thresholds > 0:
        rng = np.random.default_rng(3)
        code = rng.choice([0, 1, -1], size=call.edge_thresh.shape[0], p=[1 - thresholds, thresholds / 2, thresholds / 2])
        call.edge_thresh[:] = code.astype(call.edge_thresh.dtype)
    scale = float(np.abs(call.initial_positions).max())
    for iters in (1, 7):
        a, ta = session_run(call, n, dim, False, iters, 1.5)
        b, tb = session_run(call, n, dim, True, iters, 1.5)
        assert not np.array_equal(a.positions, b.positions)          # two kernels, two orders of summation
        assert np.abs(a.positions - b.positions).max() <= 2e-5 * scale * iters
        assert ta.shape == tb.shape and np.array_equal(ta[:, 0], tb[:, 0])
        assert np.allclose(ta[:, 1], tb[:, 1], rtol=2e-6, atol=0)
        assert b.final_mae == pytest.approx(a.final_mae, rel=2e-6) and a.iterations == b.iterations


def test_wide_sweep_with_random_labels_against_the_model():
    n, dim = 1000, 9
    call, want = _problem(n, dim, 0.15)
    got, _, counts = _symmetric_session(call, n, dim, 3, K0, COOLING, C_REP, 3, profile=True, relabel=77)
    assert counts[1] + counts[3] == 3
    scale = np.abs(want[2] - call.initial_positions).max()
    err = np.abs(got - want[2])
    assert err.mean() <= 5e-5 * scale and err.max() <= 5e-3 * scale, (err.mean() / scale, err.max() / scale)


@pytest.mark.parametrize("n,dim,thr,stages", [(1000, 7, 0.15, 2), (2973, 10, 0.0, 2), (1000, 8, 0.0, 4)])
def test_wide_multi_stage_iterations_against_the_model(n, dim, thr, stages):
    """Four S-stage iterations as S sweeps over the pairs of one stage each, against the CPU model of that schedule in
    the fp32 bands of the one-stage test; the separate checks against the oracle's edge error (2e-5); with
    TOPOLOW_SYMMETRIC_TWO_STAGE=0 the row-owner stages, another schedule, come back."""
    k0, cooling, c_rep, seed, iters = 2.0 * stages, 0.01, 0.01, 5, 4
    call, _ = pp.random_problem(n, dim, 0.7, seed=300 + n % 50 + dim, n_iter=iters, k0=k0)
    call = _with_thresholds(call, thr)
    call_r = dataclasses.replace(call, dissimilarity_matrix=_decode_rounded(call))
    want = _multi_stage_model(call_r, iters, k0, cooling, c_rep, seed, stages)
    scale = np.abs(want[-1] - call.initial_positions).max()

    def run(symmetric_stages):
        with _Env(TOPOLOW_SYMMETRIC="1", TOPOLOW_SYMMETRIC_MIN_N="0", TOPOLOW_SYMMETRIC_TWO_STAGE=symmetric_stages,
                  TOPOLOW_SYMMETRIC_STAGE_MIN_TILES="0"):
            s = _native.Session(n, dim, precision="f32")
        s.load_dense(call.dissimilarity_matrix, call.threshold_matrix, call.degrees)
        s.set_edges(call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
        s.set_positions(call.initial_positions)
        s.begin(iters, k0, cooling, c_rep, 1e-12, 10 ** 9, 2, seed, stages)
        s.run()
        s.sync()
        out = s.get_positions(), s.check_trace(), s.stage_launches
        s.close()
        return out
    got, trace, launches = run("1")
    assert launches == iters * stages
    err = np.abs(got - want[-1])
    print(f"n={n} ndim={dim} S={stages}: mean {err.mean() / scale:.3e} max {err.max() / scale:.3e}")
    assert err.mean() <= 5e-5 * scale and err.max() <= 5e-3 * scale, (err.mean() / scale, err.max() / scale)
    assert [int(t) for t in trace[:, 0]] == [2, 4]
    for row in trace:
        sm, c = orc.edge_error(want[int(row[0]) - 1], call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
        assert row[1] == pytest.approx(sm / c, rel=2e-5)
    other, _, _ = run("0")
    assert np.abs(other - got).max() > 1e-6 * scale        # the row-owner stages are another schedule


def test_production_entry_at_ndim_10_with_and_without_the_wide_sweep():
    """optimize_layout_exact_arrays at ndim 10, the size gate lowered: same stop within two checks, same final MAE to
    1e-3, and the reported MAE is the oracle's edge error of the returned positions (2e-5, fp32)."""
    call, _ = pp.random_problem(1500, 10, 0.7, seed=17, thresholds=0.1, n_iter=400, k0=10.0, cool=0.02, c_rep=0.01,
                                check_freq=3, window=5, eps=1e-4)
    with _Env(TOPOLOW_SYMMETRIC="0", TOPOLOW_SYMMETRIC_MIN_N="0"):
        a = [_native.optimize_layout_exact_arrays(*layout_call_args(call), seed=1 + q) for q in range(2)]
    with _Env(TOPOLOW_SYMMETRIC="1", TOPOLOW_SYMMETRIC_MIN_N="0"):
        b = [_native.optimize_layout_exact_arrays(*layout_call_args(call), seed=1 + q) for q in range(2)]
    for x, y in zip(a, b):
        print(f"row-owner: {x.iterations} iterations, MAE {x.final_mae!r}; sweep: {y.iterations}, {y.final_mae!r}")
        assert x.converged and y.converged
        assert not np.array_equal(x.positions, y.positions)             # the sweep really ran
        assert abs(x.iterations - y.iterations) <= 6                     # two checks (rounding can move a plateau)
        assert y.final_mae == pytest.approx(x.final_mae, rel=1e-3)
        sm, cnt = orc.edge_error(y.positions, call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
        assert y.final_mae == pytest.approx(sm / cnt, rel=2e-5)


def test_f64_sessions_of_ndim_8_stay_on_the_row_owner_kernel():
    """The f64 sweep exists for ndim 2..6: at ndim 8 TOPOLOW_SYMMETRIC=1 changes nothing, bit for bit."""
    n, dim = 1000, 8
    call, _ = _problem(n, dim, 0.0)
    got, trace, counts = _symmetric_session(call, n, dim, 7, K0, COOLING, C_REP, 3, profile=True, precision="f64")
    assert counts[1] == 0 and counts[3] == 0
    with _Env(TOPOLOW_SYMMETRIC="0"):
        s = _native.Session(n, dim, precision="f64")
    s.load_dense(call.dissimilarity_matrix, call.threshold_matrix, call.degrees)
    s.set_edges(call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
    s.set_positions(call.initial_positions)
    s.begin(7, K0, COOLING, C_REP, 1e-12, 10 ** 9, 3, 5, 1)
    s.run()
    s.sync()
    row_owner, trace_ro = s.get_positions(), s.check_trace()
    s.close()
    assert np.array_equal(got, row_owner) and np.array_equal(trace, trace_ro)
