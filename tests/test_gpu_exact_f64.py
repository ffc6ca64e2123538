"""precision = "f64_exact" (run with -m gpu): every f64 kernel beyond one workgroup reads target = word + delta, the
caller's f64 target to 2e-14 relative, where precision = "f64" takes its forces from the 4-byte words (fp32 rounded to
4 ulp, 3e-7 relative).  Every comparison below is against the CPU model or the oracle fed the caller's OWN, UNROUNDED
matrix, in the bands the f64 tests hold against the rounded one.

Each model-based test first shows, on the CPU, that its problem discriminates: the model on rounded targets
(_decode_rounded, what precision "f64" computes) lies at least 100 bands from the model on the exact ones.  Measured
for the sweep cases: >= 2e-8 of the displacement scale against bands of <= 7e-12; for the fixed-stage row-owner cases
(band 1e-9 x max(scale, 1), 1e-6 in one dimension) see _ROW_OWNER_SHAPES."""
import dataclasses
import functools

import numpy as np
import pytest

from oracle import topolow_oracle as orc
from tests import parity_problems as pp
from tests.conftest import layout_call_args
from tests.test_gpu_parity import _decode_rounded, _model_run
from tests.test_gpu_symmetric import _Env, _model_iterations, _multi_stage_model, _symmetric_session, _with_thresholds
from tests.test_r_shim import _run as _r_run, harness  # noqa: F401  (the fake-R harness fixture)
from topolow_amd import _native

pytestmark = pytest.mark.gpu

K0, COOLING, C_REP = 1.5, 0.01, 0.01
SWEEP_SHAPES = [(2, 0.0), (3, 0.15), (5, 0.0), (5, 0.15), (6, 0.15)]


def _rounded(call):
    return dataclasses.replace(call, dissimilarity_matrix=_decode_rounded(call))


def _discriminates(exact, rounded, band):
    """The model on rounded targets is at least 100 bands away from the model on the exact ones."""
    gap = np.abs(exact - rounded).max()
    print("discrimination: gap %.3g, band %.3g, bands %.0f" % (gap, band, gap / band))
    assert gap >= 100 * band, (gap, band)


@functools.lru_cache(maxsize=None)
def _sweep_problem(n, dim, thr):
    """The problems of test_symmetric_sweep_f64_equals_the_model_to_rounding; the model's seven one-stage iterations on
    the caller's targets and on the rounded ones (computed once, shared, never written to)."""
    call, _ = pp.random_problem(n, dim, 0.7 if n > 100 else 0.3, seed=190 + n % 50 + dim, n_iter=7, k0=K0)
    call = _with_thresholds(call, thr)
    exact = _model_iterations(call, 7, K0, COOLING, C_REP)
    rounded = _model_iterations(_rounded(call), 7, K0, COOLING, C_REP)
    scale = np.abs(exact[-1] - call.initial_positions).max()
    return call, exact, rounded, scale


def _check_trace(trace, want, call, rel=1e-11):
    for row in trace:
        sm, c = orc.edge_error(want[int(row[0]) - 1], call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
        assert row[1] == pytest.approx(sm / c, rel=rel), (row, sm / c)


# ---- 1. the symmetric sweep, one stage per iteration ---------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 66, 1000])
@pytest.mark.parametrize("dim,thr", SWEEP_SHAPES)
def test_exact_sweep_equals_the_model_on_unrounded_targets(n, dim, thr):
    """n = 33 and 66: phantom rows and columns, fewer tiles than waves; 1000: n % 32 = 8; the diagonal squares are met
    from both sides at every size.  Positions within 1e-12 x scale per iteration of the model on the caller's targets,
    every iteration a sweep + apply, the checks at 3, 6 (fused: ERR instances) and 7 against the oracle's edge error of
    the model's positions, profiled and unprofiled runs bit-identical -- and a plain "f64" session on the same problem
    is NOT inside 100 bands of that model."""
    call, exact, rounded, scale = _sweep_problem(n, dim, thr)
    for iters in (1, 7):
        band = 1e-12 * scale * iters
        _discriminates(exact[iters - 1], rounded[iters - 1], band)
        got, trace, counts = _symmetric_session(call, n, dim, iters, K0, COOLING, C_REP, 3, profile=True,
                                                precision="f64_exact")
        assert counts[1] + counts[3] == iters, counts
        err = np.abs(got - exact[iters - 1]).max()
        print("n %d dim %d thr %g iters %d: |got - model(exact)| = %.3g of the scale" % (n, dim, thr, iters, err / scale))
        assert err <= band, err / scale
        if iters == 7:
            assert counts[3] == 2
            assert [int(t) for t in trace[:, 0]] == [3, 6, 7]
            _check_trace(trace, exact, call)
        again, trace2, _ = _symmetric_session(call, n, dim, iters, K0, COOLING, C_REP, 3, profile=False,
                                              precision="f64_exact")
        assert np.array_equal(again, got) and np.array_equal(trace2, trace)
    plain, _, _ = _symmetric_session(call, n, dim, 7, K0, COOLING, C_REP, 3, profile=False, precision="f64")
    assert np.abs(plain - exact[-1]).max() > 100 * 1e-12 * scale * 7          # what the feature changes


# ---- 2. half the edge list: the deltas come from the matrix --------------------------------------------------------
def test_exact_sweep_with_half_the_edge_list():
    """The case of test_symmetric_sweep_f64_check_falls_back_when_the_edge_list_is_not_the_block: the fused check needs
    the list to be the block's measured cells, so there is no ERR launch and the MAE is that of the half list; the
    positions are exact all the same, because the delta tiles are made from the matrix."""
    n, dim = 1000, 5
    call, _ = pp.random_problem(n, dim, 0.7, seed=77, n_iter=7, k0=K0)
    call = _with_thresholds(call, 0.1)
    exact = _model_iterations(call, 7, K0, COOLING, C_REP)
    rounded = _model_iterations(_rounded(call), 7, K0, COOLING, C_REP)
    scale = np.abs(exact[-1] - call.initial_positions).max()
    _discriminates(exact[-1], rounded[-1], 1e-12 * scale * 7)
    half = np.arange(call.edge_i.shape[0]) % 2 == 0
    part = dataclasses.replace(call, edge_i=call.edge_i[half], edge_j=call.edge_j[half], edge_dist=call.edge_dist[half],
                               edge_thresh=call.edge_thresh[half])
    got, trace, counts = _symmetric_session(part, n, dim, 7, K0, COOLING, C_REP, 3, profile=True, precision="f64_exact")
    assert counts[1] == 7 and counts[3] == 0
    assert np.abs(got - exact[-1]).max() <= 1e-12 * scale * 7
    assert [int(t) for t in trace[:, 0]] == [3, 6, 7]
    _check_trace(trace, exact, part)


# ---- 3. random labels ----------------------------------------------------------------------------------------------
def test_exact_sweep_with_random_labels():
    """The delta block is relabelled like the words (topolow_session_set_relabel)."""
    n, dim = 1000, 5
    call, _ = pp.random_problem(n, dim, 0.7, seed=77, n_iter=7, k0=K0)
    call = _with_thresholds(call, 0.1)
    exact = _model_iterations(call, 7, K0, COOLING, C_REP)
    rounded = _model_iterations(_rounded(call), 7, K0, COOLING, C_REP)
    scale = np.abs(exact[-1] - call.initial_positions).max()
    for iters in (1, 7):
        _discriminates(exact[iters - 1], rounded[iters - 1], 1e-12 * scale * iters)
        got, trace, counts = _symmetric_session(call, n, dim, iters, K0, COOLING, C_REP, 3, profile=True, relabel=91,
                                                precision="f64_exact")
        assert counts[1] + counts[3] == iters
        assert np.abs(got - exact[iters - 1]).max() <= 1e-12 * scale * iters
        if iters == 7:
            assert counts[3] == 2
            _check_trace(trace, exact, call)


# ---- 4. multi-stage iterations as symmetric sweeps -----------------------------------------------------------------
@pytest.mark.parametrize("n,dim,thr,stages", [(300, 2, 0.0, 2), (1000, 5, 0.15, 2), (1000, 5, 0.15, 4)])
def test_exact_multi_stage_sweeps_equal_the_model_on_unrounded_targets(n, dim, thr, stages):
    """The environment of test_multi_stage_iterations_as_symmetric_sweeps_against_the_model: the pair-split stages
    launch the same exact kernel with another plan."""
    k0, seed, iters = 2.0 * stages, 5, 4
    call, _ = pp.random_problem(n, dim, 0.7 if n > 500 else 0.3, seed=300 + n % 50 + dim, n_iter=iters, k0=k0)
    call = _with_thresholds(call, thr)
    exact = _multi_stage_model(call, iters, k0, COOLING, C_REP, seed, stages)
    rounded = _multi_stage_model(_rounded(call), iters, k0, COOLING, C_REP, seed, stages)
    scale = np.abs(exact[-1] - call.initial_positions).max()
    band = 1e-12 * scale * iters * stages
    _discriminates(exact[-1], rounded[-1], band)
    with _Env(TOPOLOW_SYMMETRIC="1", TOPOLOW_SYMMETRIC_MIN_N="0", TOPOLOW_SYMMETRIC_TWO_STAGE="1",
              TOPOLOW_SYMMETRIC_STAGE_MIN_TILES="0"):
        s = _native.Session(n, dim, precision="f64_exact")
    s.load_dense(call.dissimilarity_matrix, call.threshold_matrix, call.degrees)
    s.set_edges(call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
    s.set_positions(call.initial_positions)
    s.begin(iters, k0, COOLING, C_REP, 1e-12, 10 ** 9, 2, seed, stages)
    s.run()
    s.sync()
    got, trace, launches = s.get_positions(), s.check_trace(), s.stage_launches
    s.close()
    assert launches == iters * stages
    assert np.abs(got - exact[-1]).max() <= band, np.abs(got - exact[-1]).max() / scale
    assert [int(t) for t in trace[:, 0]] == [2, 4]
    _check_trace(trace, exact, call)


# ---- 5. the row-owner stage kernel (TOPOLOW_SYMMETRIC=0) ------------------------------------------------------------
# (n, ndim, missing, thresholds, stages): the shapes of test_slab_f64_matches_model that take seconds, plus 11 and 16
# coordinates (the 12- and 16-coordinate instances).  Bands of that test: 1e-9 x max(scale, 1), 1e-6 in one dimension --
# only 100 times below what the rounding moves, so the gap between the two models was measured on the CPU first, in
# bands: 180, 414, 517, 99 187 (one dimension) for the first, second, third and fifth shape.  Three shapes first thought
# of did not reach 100 and were replaced by the same coordinate counts at 90 % missing, which do:
#   (777, 10, 0.6, 0.0, 4):  95 bands  ->  (777, 10, 0.9, 0.0, 4): 216
#   (300, 11, 0.6, 0.1, 4):  89 bands  ->  (777, 11, 0.9, 0.1, 4): 364
#   (300, 16, 0.6, 0.0, 4):  55 bands  ->  (777, 16, 0.9, 0.0, 4): 161
_ROW_OWNER_SHAPES = [(256, 5, 0.7, 0.0, 4), (301, 3, 0.5, 0.2, 4), (1030, 5, 0.7, 0.1, 8), (777, 10, 0.9, 0.0, 4),
                     (513, 1, 0.3, 0.0, 4), (777, 11, 0.9, 0.1, 4), (777, 16, 0.9, 0.0, 4)]


@pytest.mark.parametrize("n,dim,missing,thr,stages", _ROW_OWNER_SHAPES)
def test_exact_row_owner_stages_match_the_model_on_unrounded_targets(n, dim, missing, thr, stages):
    call, _ = pp.random_problem(n, dim, missing, seed=n + 1, thresholds=thr, n_iter=6, check_freq=3)
    seed = 42
    want, _k = _model_run(call, seed, stages, 6, "f64")
    want_r, _k = _model_run(_rounded(call), seed, stages, 6, "f64")
    scale = np.abs(want - call.initial_positions).max()
    band = (1e-6 if dim == 1 else 1e-9) * max(scale, 1.0)
    _discriminates(want, want_r, band)
    with _Env(TOPOLOW_SYMMETRIC="0"):
        s = _native.Session(n, dim, precision="f64_exact")
    s.load_dense(call.dissimilarity_matrix, call.threshold_matrix, call.degrees)
    s.set_edges(call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
    s.set_positions(call.initial_positions)
    s.begin(6, call.k0, call.cooling_rate, call.c_repulsion, 1e-12, 1000, 3, seed, stages)
    s.run()
    got = s.get_positions()
    res = s.finish()
    s.close()
    print("n %d dim %d: |got - model(exact)| = %.3g, band %.3g" % (n, dim, np.abs(got - want).max(), band))
    assert np.abs(got - want).max() <= band
    sm, cnt = orc.edge_error(res.positions, call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
    assert res.final_mae == pytest.approx(sm / cnt, rel=1e-12)


@pytest.mark.parametrize("n", [66, 1000])
def test_exact_row_owner_one_stage_iterations(n):
    """One-stage iterations on the row-owner kernel, in the sweep's band."""
    dim, thr = 5, 0.15
    call, exact, rounded, scale = _sweep_problem(n, dim, thr)
    band = 1e-12 * scale * 7
    _discriminates(exact[-1], rounded[-1], band)
    with _Env(TOPOLOW_SYMMETRIC="0"):
        s = _native.Session(n, dim, precision="f64_exact")
    s.load_dense(call.dissimilarity_matrix, call.threshold_matrix, call.degrees)
    s.set_edges(call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
    s.set_positions(call.initial_positions)
    s.begin(7, K0, COOLING, C_REP, 1e-12, 10 ** 9, 3, 5, 1)
    s.run()
    s.sync()
    got = s.get_positions()
    s.close()
    assert np.abs(got - exact[-1]).max() <= band, np.abs(got - exact[-1]).max() / scale


# ---- 6. tile Gauss-Seidel ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim,missing,thr", [(65, 3, 0.5, 0.2), (130, 5, 0.6, 0.1), (777, 5, 0.7, 0.15)])
def test_exact_tile_gs_matches_the_oracle_on_unrounded_targets(n, dim, missing, thr):
    """test_tile_gs_f64_matches_oracle_same_order without the rounding: the oracle replays tilegs_pair_order on the
    caller's own matrix and edge list."""
    call, _ = pp.random_problem(n, dim, missing, seed=300 + n, thresholds=thr, n_iter=7, check_freq=2)
    seed = 77
    s = _native.Session(n, dim, precision="f64_exact")
    s.set_schedule("gs")
    s.load_dense(call.dissimilarity_matrix, call.threshold_matrix, call.degrees)
    s.set_edges(call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
    s.set_positions(call.initial_positions)
    s.begin(7, call.k0, call.cooling_rate, call.c_repulsion, 1e-4, 5, 2, seed, 0)
    s.run()
    got = s.finish()
    s.close()

    def order_fn(it, arr):
        arr[:] = _native.tilegs_pair_order(n, seed, it)
    ref = orc.optimize_layout_exact(*layout_call_args(call), order_mode=orc.ORDER_SUPPLIED, order_fn=order_fn)
    assert np.abs(got.positions - ref.positions).max() <= 1e-11
    assert got.iterations == ref.iterations and got.converged == ref.converged
    assert got.final_mae == pytest.approx(ref.final_mae, rel=1e-11)


# ---- 7. the production entry ---------------------------------------------------------------------------------------
def test_exact_production_entry():
    call, _ = pp.random_problem(1500, 5, 0.7, seed=17, thresholds=0.1, n_iter=400, k0=10.0, cool=0.02, c_rep=0.01)
    with _Env(TOPOLOW_SYMMETRIC_MIN_N="0"):
        a = _native.optimize_layout_exact_arrays(*layout_call_args(call), seed=3, schedule="slab", precision="f64_exact")
        b = _native.optimize_layout_exact_arrays(*layout_call_args(call), seed=3, schedule="slab", precision="f64")
    assert a.converged and a.info["precision"] == "f64_exact" and a.info["schedule"] == "slab"
    sm, cnt = orc.edge_error(a.positions, call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
    assert a.final_mae == pytest.approx(sm / cnt, rel=1e-12)
    assert b.info["precision"] == "f64" and not np.array_equal(a.positions, b.positions)
    # one workgroup: the GS kernel reads f64 targets at either value
    small, _ = pp.random_problem(101, 5, 0.7, seed=101, n_iter=25)
    x = _native.optimize_layout_exact_arrays(*layout_call_args(small), seed=9, schedule="gs", precision="f64_exact")
    y = _native.optimize_layout_exact_arrays(*layout_call_args(small), seed=9, schedule="gs", precision="f64")
    assert x.info["precision"] == "f64_exact" and y.info["precision"] == "f64" and x.info["schedule"] == "gs"
    assert np.array_equal(x.positions, y.positions) and x.final_mae == y.final_mae and x.iterations == y.iterations


# ---- 8. what it refuses; what it leaves alone ----------------------------------------------------------------------
def test_exact_refusals():
    def refused(fn, what):
        with pytest.raises(_native.NativeError, match=what) as ei:
            fn()
        assert ei.value.code == _native.ERR_UNSUPPORTED

    refused(lambda: _native.Session(100, 3, 0, 50, precision="f64_exact"), "whole-problem sessions only")
    refused(lambda: _native.Session(100, 20, precision="f64_exact"), "ndim must be between 1 and 16")
    call, _ = pp.random_problem(100, 3, 0.5, seed=4, n_iter=5)
    s = _native.Session(100, 3, precision="f64_exact")
    refused(lambda: s.commit_encoded(call.degrees), "carries no deltas")
    s.load_dense(call.dissimilarity_matrix, call.threshold_matrix, call.degrees)
    s.set_edges(call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
    refused(lambda: s.hold_out(call.edge_i[:5], call.edge_j[:5], call.degrees), "delta block")
    s.close()
    refused(lambda: _native.optimize_layout_exact_arrays(*layout_call_args(call), seed=1, schedule="slab",
                                                         precision="f64_exact", devices=[0, 0]), "one GPU only")


def test_plain_f64_sessions_still_equal_the_rounded_model():
    """The guard that the default did not move: precision "f64" on the shapes of the first test is the model on the
    ROUNDED targets to 1e-12 x scale per iteration, as before."""
    for n in (33, 66, 1000):
        for dim, thr in SWEEP_SHAPES:
            call, _, rounded, _ = _sweep_problem(n, dim, thr)
            scale = np.abs(rounded[-1] - call.initial_positions).max()
            got, _, counts = _symmetric_session(call, n, dim, 7, K0, COOLING, C_REP, 3, profile=True, precision="f64")
            assert counts[1] + counts[3] == 7
            assert np.abs(got - rounded[-1]).max() <= 1e-12 * scale * 7, (n, dim, thr)


# ---- 9. the R shim -------------------------------------------------------------------------------------------------
def test_r_shim_passes_the_exact_precision_through(harness, tmp_path):  # noqa: F811
    """options(topolow.precision = "f64_exact") through the fake-R harness of tests/test_r_shim.py: the positions of the
    library's own call at that precision (whose report names it), not those of "f64"."""
    call, _ = pp.random_problem(40, 3, 0.4, seed=12, n_iter=30)
    opts = [("topolow.seed", "int", 42), ("topolow.schedule", "str", "slab")]
    out = _r_run(harness, tmp_path, call, opts + [("topolow.precision", "str", "f64_exact")])
    want = _native.optimize_layout_exact_arrays(*layout_call_args(call), seed=42, schedule="slab", precision="f64_exact")
    assert want.info["precision"] == "f64_exact"
    got = np.array(out["positions"]).reshape(want.positions.shape, order="F")
    assert np.array_equal(got, want.positions)
    assert out["iterations"] == want.iterations and out["final_mae"] == want.final_mae
    plain = _r_run(harness, tmp_path, call, opts + [("topolow.precision", "str", "f64")])
    assert not np.array_equal(np.array(plain["positions"]).reshape(want.positions.shape, order="F"), want.positions)
