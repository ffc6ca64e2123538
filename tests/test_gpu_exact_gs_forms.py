"""Exact Gauss-Seidel, every kernel form (run with -m gpu on an MI355X): each form of the one-workgroup kernel
(relax_gs.h) and of the tile schedule (relax_tilegs.h) against the CPU oracle replaying topolow_gs_pair_order /
topolow_tilegs_pair_order pair for pair.

Forms of gs_embed_kernel and the case that reaches each (the library has no "which form ran" flag; the reasons are
asserted from the sizes with gs_forms.lds_bytes / table_eligible, which restate the documented rules):
  * LDS table: a batch whose members all have < 65 535 edges and a table within 78 KB -- n = 2, 3, 65 (90 % missing), 130;
  * dense, one pair per thread with the next round's target prefetched: pairs per round <= threads (1 024 at most) --
    n = 700 fully measured (244 650 edges: no table), 1 200, 2 048 (1 024 pairs on 1 024 threads: the last size);
  * dense strided: n >= 2 049 -> 1 025 pairs per round > 1 024 threads -- n = 2 049 (odd: a bye), 2 050, 2 500, the limit;
  * more than 64 KB of dynamic LDS (the hipFuncSetAttribute branch): 56 bytes per point in f64 at ndim 5 -> n >= 1 165;
  * the 160 KB limit: the largest n that topolow_batch_problem_fits accepts, found by bisection, odd and even;
  * mixed grids: one launch sized by its largest member holding table-eligible, prefetching and strided members;
  * the fp32 pair update (v_rcp_f32 / v_sqrt_f32 / fma) in all three forms;
and of the tile schedule: every coordinate count its kernels are instantiated for (1..10, 12, 16 and the zero-padded
11, 13, 14, 15), both precisions, ragged last tiles, and problems below one tile (one block: no pair round, the intra
kernel does all the work).

Sizes found by bisection on MI355X builds (tests/test_gs_batch_limit.py lists all): f64 ndim 5 -> 2 920, ndim 11 / 12 ->
1 460, ndim 16 -> 1 135; fp32 ndim 5 -> 4 543.

Tolerances: f64 as tests/test_gpu_parity.py and tests/test_gpu_fuzz.py hold the small cases (positions 1e-12 (1 +
max|ref|), controller fields equal, MAE rel 1e-11; tile schedule 1e-11 absolute); fp32 calibrated in the test on the
oracle's own fp32 replay (fp32_ratio)."""
import dataclasses
import functools

import numpy as np
import pytest

from oracle import topolow_oracle as orc
from tests import gs_forms as g
from tests.conftest import layout_call_args
from topolow_amd import _native, cv, synthetic

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------------------
# shared cases: a problem per (n, ndim, missing, thresholds, iterations), its oracle replays and its run alone, each
# computed once
# ----------------------------------------------------------------------------------------
def params_of(n):
    """Every size its own spring, cooling and repulsion constants."""
    return dict(k0=2.0 + n % 5, cool=0.03 + 0.01 * (n % 4), c_rep=0.01 * (1 + n % 3))


def seed_of(n, dim):
    return 5000 + 7 * n + dim


@functools.lru_cache(maxsize=6)
def call_of(n, dim=5, missing=0.7, thr=0.15, n_iter=5):
    """check_freq 2: with 5 iterations checks after 2 and 4 and the final one after 5 (the `last iteration` branch)."""
    return g.problem(n, dim, missing, seed=n + dim, thresholds=thr, n_iter=n_iter, check_freq=2, **params_of(n))


_ORACLE, _ALONE = {}, {}


def oracle_of(key, arith="f64"):
    if (key, arith) not in _ORACLE:
        _ORACLE[key, arith] = g.oracle_gs(call_of(*key), seed_of(key[0], key[1]), arith)
    return _ORACLE[key, arith]


def alone_of(key, precision="f64"):
    """The case as a batch of one."""
    if (key, precision) not in _ALONE:
        res, _ = _native.optimize_layout_exact_batch([call_of(*key)], seeds=[seed_of(key[0], key[1])], precision=precision)
        _ALONE[key, precision] = res[0]
    return _ALONE[key, precision]


def same_as_oracle(got, ref, tag):
    assert not isinstance(got, Exception), (tag, got)
    dev = np.abs(got.positions - ref.positions).max()
    print(f"{tag}: max |dev| {dev:.3e} (scale {np.abs(ref.positions).max():.3g}), MAE {got.final_mae!r} vs {ref.final_mae!r}, "
          f"best {got.iterations} run {got.info['iterations_run']} checks {got.info['n_checks']}")
    assert dev <= 1e-12 * (1 + np.abs(ref.positions).max()), (tag, dev)
    assert (got.converged, got.iterations, got.info["iterations_run"]) == (ref.converged, ref.iterations, ref.iters_run), tag
    assert got.final_k == ref.final_k, tag
    assert got.final_mae == pytest.approx(ref.final_mae, rel=1e-11), tag


def same_run(a, b, tag):
    """Bit-equal positions and controller fields; the MAE to rel 1e-11 (the table and the dense form add the check's
    terms in different edge orders)."""
    assert not isinstance(a, Exception) and not isinstance(b, Exception), (tag, a, b)
    assert np.array_equal(a.positions, b.positions), (tag, np.abs(a.positions - b.positions).max())
    assert (a.converged, a.iterations, a.final_k, a.info["iterations_run"], a.info["n_checks"]) == \
           (b.converged, b.iterations, b.final_k, b.info["iterations_run"], b.info["n_checks"]), tag
    assert a.final_mae == pytest.approx(b.final_mae, rel=1e-11), tag


def fp32_ratio(got_positions, got_mae, ref64, ref32, start, tag):
    """The fp32 band, calibrated on the reference side: d_ref = what rounding every operation to fp32 does to this
    problem over these iterations (largest difference between the oracle's fp32 and f64 replays of the same order, in
    units of the largest displacement from the start).  The kernels add v_rcp_f32 / v_sqrt_f32 (about 1 ulp each) and
    fused multiply-adds on top of fp32 rounding, so they must land at the same order: within 4 d_ref of the f64 replay.
    The MAE against the fp32 replay's: within 4 x the relative difference of the two replays' MAEs, floor 1e-6."""
    disp = np.abs(ref64.positions - start).max()
    d_ref = np.abs(ref32.positions - ref64.positions).max() / disp
    d_gpu = np.abs(got_positions - ref64.positions).max() / disp
    m_ref = abs(ref32.final_mae - ref64.final_mae) / ref64.final_mae
    m_gpu = abs(got_mae - ref32.final_mae) / ref32.final_mae
    print(f"{tag}: d_ref {d_ref:.3e} d_gpu {d_gpu:.3e} ratio {d_gpu / d_ref:.2f}; MAE rel: replays {m_ref:.3e} "
          f"kernel {m_gpu:.3e}")
    assert d_ref > 0 and d_gpu <= 4 * d_ref, (tag, d_gpu, d_ref)
    assert m_gpu <= max(4 * m_ref, 1e-6), (tag, m_gpu, m_ref)


def resolve(size, dim):
    """"limit" -> the largest n the library accepts at this ndim (n_max of the coordinate count it runs as)."""
    if not size.startswith("limit"):
        return int(size)
    return g.batch_limit(g.kernel_dim(dim), "f64") + (int(size[5:]) if len(size) > 5 else 0)


# ----------------------------------------------------------------------------------------
# 1. one-workgroup kernel, f64
# ----------------------------------------------------------------------------------------
def test_limits_found_by_bisection():
    """n_max(ndim, precision) from _native.batch_problem_fits: monotone in n (gs_forms.batch_limit scans every n) and
    where the arithmetic on the LDS carve-up puts it, to 1 %: about 2 920 (f64, ndim 5), 4 540 (fp32, ndim 5), 1 135
    (f64, ndim 16)."""
    found = {(d, p): g.batch_limit(d, p) for d in (5, 12, 16) for p in ("f64", "f32")}
    print("limits found:", found)
    assert abs(found[5, "f64"] - 2920) <= 29 and abs(found[5, "f32"] - 4540) <= 45 and abs(found[16, "f64"] - 1135) <= 11
    assert g.batch_limit(11, "f64") == found[12, "f64"]
    # the forms the cases below are said to reach
    assert g.lds_bytes(1200, 5, 8) > 64 * 1024 and g.lds_bytes(2048, 5, 8) > 64 * 1024
    assert g.lds_bytes(found[5, "f64"], 5, 8) > g.LDS_LIMIT - 64


@pytest.mark.parametrize("size,dim", [("2049", 5), ("2050", 5), ("2500", 5), ("limit", 5), ("limit-1", 5), ("limit", 16),
                                      ("limit", 11), ("1200", 5), ("2048", 5)])
def test_one_workgroup_f64_matches_oracle(size, dim):
    """Through optimize_layout_exact_batch, 70 % missing (> 65 535 edges: dense form), 15 % thresholds, 5 iterations.
      n = 2 049 -> 1 025 pairs per round > 1 024 threads: strided form, odd field (a bye in every round);
      n = 2 050: the first even field of the strided form; n = 2 500: strided, 137 KB of LDS;
      n = limit, limit - 1 at ndim 5 (2 920, 2 919): strided form at the 160 KB limit, even and odd;
      n = limit at ndim 16 (1 135) and at ndim 11 (1 460: runs zero-padded as 12; the returned positions have 11
      columns): prefetching form at the 160 KB limit;
      n = 1 200, 2 048: prefetching form above 64 KB of LDS (66 and 112 KB)."""
    n = resolve(size, dim)
    key = (n, dim, 0.7, 0.15, 5)
    assert not g.table_eligible(call_of(*key)) and _native.batch_problem_fits(n, dim, "f64", 0)
    got = alone_of(key)
    assert got.positions.shape == (n, dim)
    same_as_oracle(got, oracle_of(key), f"n {n} ndim {dim}")


def test_2048_points_one_shot_equals_batch():
    """The largest size the one-shot entry sends to the one-workgroup kernel: schedule="gs" and the batch entry give the
    same bits."""
    key = (2048, 5, 0.7, 0.15, 5)
    one = _native.optimize_layout_exact_arrays(*layout_call_args(call_of(*key)), seed=seed_of(2048, 5), schedule="gs",
                                               precision="f64")
    assert one.info["schedule"] == "gs" and one.info["precision"] == "f64"
    bat = alone_of(key)
    assert np.array_equal(one.positions, bat.positions)
    assert (one.converged, one.iterations, one.final_mae, one.final_k, one.info["iterations_run"], one.info["n_checks"]) == \
           (bat.converged, bat.iterations, bat.final_mae, bat.final_k, bat.info["iterations_run"], bat.info["n_checks"])


@pytest.mark.parametrize("dim,precision", [(5, "f64"), (16, "f64"), (11, "f64"), (5, "f32")])
def test_one_point_past_the_limit_is_refused(dim, precision):
    """n_max + 1: batch_problem_fits says no and the batch entry answers TOPOLOW_ERR_UNSUPPORTED, pointing to the slab
    schedule (nothing is launched)."""
    n = g.batch_limit(g.kernel_dim(dim), precision) + 1
    assert not _native.batch_problem_fits(n, dim, precision, 0) and _native.batch_problem_fits(n - 1, dim, precision, 0)
    rng = np.random.default_rng(n)
    chain = np.arange(n - 1, dtype=np.int32)
    call = cv.SparseCall(initial_positions=rng.normal(size=(n, dim)), degrees=np.full(n, 3, np.int32), edge_i=chain,
                         edge_j=chain + 1, edge_dist=rng.uniform(1, 2, n - 1), edge_thresh=np.zeros(n - 1, np.int32),
                         n_iter=2, k0=3.0, cooling_rate=0.05, c_repulsion=0.01, relative_epsilon=1e-4,
                         convergence_window=5, convergence_check_freq=2)
    with pytest.raises(_native.NativeError, match="slab schedule") as e:
        _native.optimize_layout_exact_batch([call], seeds=[1], precision=precision)
    assert e.value.code == _native.ERR_UNSUPPORTED


def test_run_to_the_controllers_stop_above_64kb_of_lds():
    """1 200 points (66 KB of LDS, prefetching form) with a strong repulsion and fast cooling: the error falls, then
    rises as the springs cool, the controller stops the run on the worsening rule and the best snapshot -- several
    iterations back -- is restored.  (Parameters chosen on the oracle: best iteration 14 of 22 run.)"""
    call = g.problem(1200, 5, 0.7, seed=1200, thresholds=0.15, n_iter=200, check_freq=2, k0=10.0, cool=0.25, c_rep=1.0,
                     eps=1e-4, window=4)
    ref = g.oracle_gs(call, 77)
    assert ref.converged and ref.iterations + 4 <= ref.iters_run < 200, (ref.iterations, ref.iters_run)
    got, _ = _native.optimize_layout_exact_batch([call], seeds=[77])
    same_as_oracle(got[0], ref, "n 1200 to the stop")


def test_edge_list_standing_for_the_matrix_strided_form():
    """30 % of the 2 500-point case's edges (thresholds among them) with dissimilarity_matrix = None: the list is the
    matrix, which the dense form rebuilds on the host (n > 2 048: no table).  Equals the oracle on the matrix rebuilt
    from the same list."""
    base = call_of(2500, 5, 0.7, 0.15, 5)
    lean, full = g.subset_of_edges(base, 0.3, seed=9)
    assert (lean.edge_thresh != 0).sum() > 1000 and lean.dissimilarity_matrix is None
    got, _ = _native.optimize_layout_exact_batch([lean], seeds=[41])
    same_as_oracle(got[0], g.oracle_gs(full, 41), "n 2500 listed")


# ----------------------------------------------------------------------------------------
# 2. unlike members in one grid
# ----------------------------------------------------------------------------------------
MIXED = [(2, 5, 0.0, 0.15, 5), (3, 5, 0.0, 0.15, 5), (65, 5, 0.9, 0.15, 5), (700, 5, 0.0, 0.15, 5),
         (2500, 5, 0.7, 0.15, 5)]
NAN_MEMBER = (20, 5, 0.3, 0.15, 12)
TWO_GRIDS = [(3, 2, 0.0, 0.15, 5), (200, 2, 0.9, 0.15, 5), (65, 5, 0.9, 0.15, 5), (700, 5, 0.0, 0.15, 5)]


def run_batch(keys, extra=(), holdouts=None):
    calls = [call_of(*k) for k in keys] + [c for c, _ in extra]
    seeds = [seed_of(k[0], k[1]) for k in keys] + [s for _, s in extra]
    res, _ = _native.optimize_layout_exact_batch(calls, seeds=seeds, holdouts=holdouts)
    return res


def nan_call():
    """20 points, a NaN in the start, checks every 3 iterations: three NaN checks before the guard looks at iteration 10,
    fewer than the window of 5 (five NaN checks in a row read as a plateau before the guard is reached -- in the reference
    too: the oracle then returns converged at iteration 10 instead of raising)."""
    call = g.problem(*NAN_MEMBER[:3], seed=20, thresholds=NAN_MEMBER[3], n_iter=NAN_MEMBER[4], check_freq=3)
    bad = call.initial_positions.copy()
    bad[4, 0] = np.nan
    return dataclasses.replace(call, initial_positions=bad)


def mixed_holdouts():
    """Held-out pairs of the 2 500-point member (300 random pairs, then i == j, a pair twice, a pair reversed) and of
    the 2-point member; none for the others."""
    rng = np.random.default_rng(5)
    hi, hj = rng.integers(0, 2500, 300), rng.integers(0, 2500, 300)
    hi = np.concatenate([hi, [7, hi[0], hj[1]]]).astype(np.int32)
    hj = np.concatenate([hj, [7, hj[0], hi[1]]]).astype(np.int32)
    big = (hi, hj, rng.uniform(0.5, 9.0, hi.size))
    small = (np.array([0, 1, 0, 0, 1], np.int32), np.array([1, 0, 0, 1, 1], np.int32), np.array([1.5, 0.25, 0.0, 3.0, 2.0]))
    return [small, None, None, None, big, None]


@functools.lru_cache(maxsize=1)
def mixed_grid():
    """ONE launch at ndim 5: threads (1 024) and LDS (137 KB) sized by the 2 500-point member.  n = 2, 3 and 65 alone
    would take the LDS table; next to n = 700 (244 650 edges: no table) and n = 2 500 every member runs the dense form:
    the small ones its prefetching body, the 2 500-point one the strided body, in the same grid.  A sixth member starts
    with a NaN coordinate."""
    assert [g.table_eligible(call_of(*k)) for k in MIXED] == [True, True, True, False, False]
    return run_batch(MIXED, extra=[(nan_call(), 99)], holdouts=mixed_holdouts())


def test_mixed_grid_members_match_their_oracle_replays():
    for key, got in zip(MIXED, mixed_grid()):
        same_as_oracle(got, oracle_of(key), f"mixed grid, n {key[0]}")


def test_mixed_grid_members_equal_their_runs_alone():
    """A member's result does not depend on its companions, whichever form it takes alone (n = 2, 3, 65: the table)."""
    for key, got in zip(MIXED, mixed_grid()):
        same_run(got, alone_of(key), f"mixed grid vs alone, n {key[0]}")


def test_mixed_grid_holdouts_stay_with_their_member():
    res = mixed_grid()
    for got, hold in zip(res[:5], mixed_holdouts()):
        if hold is None:
            assert got.info["holdout_count"] == 0 and got.info["holdout_sum_abs"] == 0.0
            continue
        hi, hj, truth = hold
        p = got.positions
        want = np.abs(truth - np.sqrt(((p[hi] - p[hj]) ** 2).sum(-1))).sum()
        assert got.info["holdout_count"] == hi.size
        assert got.info["holdout_sum_abs"] == pytest.approx(want, rel=1e-12)


def test_mixed_grid_nonfinite_member_leaves_the_others_alone():
    """The member that starts with a NaN reports TOPOLOW_ERR_NONFINITE at iteration 10 (the library's guard, reference
    :359-361); the same grid without it gives the other members the same bits."""
    res = mixed_grid()
    bad = res[5]
    assert isinstance(bad, _native.NativeError) and bad.code == _native.ERR_NONFINITE
    assert "Numerical instability at iteration 10." in str(bad)
    with pytest.raises(orc.OracleError, match=r"Numerical instability at iteration 10\."):
        g.oracle_gs(nan_call(), 99)
    for key, a, b in zip(MIXED, res, run_batch(MIXED)):
        same_run(a, b, f"with / without the NaN member, n {key[0]}")
        assert a.final_mae == b.final_mae


def test_table_members_with_the_dense_switch(monkeypatch):
    """A grid of table-eligible members only (n = 2, 3, 65) runs the LDS-table form; TOPOLOW_GS_DENSE=1 sends the same
    grid to the dense form: same position arithmetic, bit-equal positions."""
    keys = MIXED[:3]
    table = run_batch(keys)
    monkeypatch.setenv("TOPOLOW_GS_DENSE", "1")
    dense = run_batch(keys)
    for key, a, b in zip(keys, table, dense):
        same_run(a, b, f"table vs dense, n {key[0]}")
        same_run(a, alone_of(key), f"table grid vs alone, n {key[0]}")


def test_two_grids_side_by_side():
    """ndim 2 and ndim 5 in one call: two grids on their own streams -- the ndim-2 members (3 and 200 points, 90 %
    missing) all take the table, the ndim-5 grid holds one member that cannot (n = 700 fully measured) and so runs dense."""
    assert [g.table_eligible(call_of(*k)) for k in TWO_GRIDS] == [True, True, True, False]
    for key, got in zip(TWO_GRIDS, run_batch(TWO_GRIDS)):
        same_as_oracle(got, oracle_of(key), f"two grids, n {key[0]} ndim {key[1]}")
        same_run(got, alone_of(key), f"two grids vs alone, n {key[0]} ndim {key[1]}")


# ----------------------------------------------------------------------------------------
# 3. fp32 in the batch kernel
# ----------------------------------------------------------------------------------------
FP32 = [(130, 5, 0.6, 0.15, 6), (700, 5, 0.0, 0.15, 6), (2500, 5, 0.7, 0.15, 6)]


@pytest.mark.parametrize("key", FP32, ids=["table-130", "prefetch-700", "strided-2500"])
def test_batch_fp32_at_the_oracles_fp32_level(key):
    """The fp32 pair update in the LDS-table form (n = 130, 3 354 edges), the prefetching form (n = 700 fully measured)
    and the strided form (n = 2 500), 6 iterations, 15 % thresholds, against the oracle's f64 replay of the same order
    in the band fp32_ratio calibrates on the oracle's fp32 replay.
    Measured on MI355X, d_gpu / d_ref (d_ref): n = 130 1.06 (1.3e-5), n = 700 1.12 (1.9e-4), n = 2 500 1.06 (1.3e-3);
    MAE against the fp32 replay 1.0e-7, 9.4e-7, 3.0e-8 relative (bands 1e-6, 3.8e-5, 3.5e-5)."""
    assert g.table_eligible(call_of(*key), "f32") == (key[0] == 130)
    got = alone_of(key, "f32")
    assert not isinstance(got, Exception), got
    ref64, ref32 = oracle_of(key), oracle_of(key, "f32")
    assert got.info["iterations_run"] == ref64.iters_run == 6
    fp32_ratio(got.positions, got.final_mae, ref64, ref32, call_of(*key).initial_positions, f"batch fp32 n {key[0]}")


def test_batch_fp32_table_and_dense_forms_agree(monkeypatch):
    """The same fp32 call in the table form and, with TOPOLOW_GS_DENSE=1, in the dense form: bit-equal positions after
    the same iterations.  The MAEs agree to 1e-6 relative only: the table form's check reads the targets it keeps in
    LDS, rounded to fp32, the dense form's reads the f64 edge list."""
    key = FP32[0]
    table = alone_of(key, "f32")
    monkeypatch.setenv("TOPOLOW_GS_DENSE", "1")
    dense, _ = _native.optimize_layout_exact_batch([call_of(*key)], seeds=[seed_of(key[0], key[1])], precision="f32")
    dense = dense[0]
    assert np.array_equal(table.positions, dense.positions)
    assert (table.iterations, table.info["iterations_run"], table.info["n_checks"]) == \
           (dense.iterations, dense.info["iterations_run"], dense.info["n_checks"])
    print("fp32 table / dense MAE:", table.final_mae, dense.final_mae)
    assert table.final_mae == pytest.approx(dense.final_mae, rel=1e-6)


# ----------------------------------------------------------------------------------------
# 4. tile schedule, every instantiation
# ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def tile_call(n, dim):
    return g.problem(n, dim, 0.6, seed=300 + n + dim, thresholds=0.1, n_iter=7, check_freq=2)


def tile_run(call, seed, precision):
    """A session with the tile schedule, as test_gpu_parity.test_tile_gs_f64_matches_oracle_same_order drives it: the
    matrix loaded dense, the edge list with the targets the session keeps (4-ulp-rounded fp32)."""
    n, dim = call.initial_positions.shape
    r = g.rounded(call)
    s = _native.Session(n, dim, precision=precision)
    try:
        s.set_schedule("gs")
        s.load_dense(call.dissimilarity_matrix, call.threshold_matrix, call.degrees)
        s.set_edges(r.edge_i, r.edge_j, r.edge_dist, r.edge_thresh)
        s.set_positions(call.initial_positions)
        s.begin(call.n_iter, call.k0, call.cooling_rate, call.c_repulsion, call.relative_epsilon, call.convergence_window,
                call.convergence_check_freq, seed, 0)
        s.run()
        return s.finish()
    finally:
        s.close()


TILE_F64 = [(130, d) for d in (1, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16)] + [(2, 5), (3, 5), (33, 5), (63, 5), (129, 2)]


@pytest.mark.parametrize("n,dim", TILE_F64)
def test_tile_gs_f64_every_width_and_sub_tile_sizes(n, dim):
    """tilegs_pair_kernel / tilegs_intra_kernel<DIM, double> for the coordinate counts test_tile_gs_f64_matches_oracle_
    same_order leaves out (it has 2, 3 and 5): n = 130 is two full tiles and a third of 2 points; ndim 11 runs
    zero-padded as 12, 13..15 as 16.  n = 2, 3, 33, 63 at ndim 5: one block, so no pair round at all and the intra
    kernel does everything; n = 129 at ndim 2: a third tile holding a single point."""
    call = tile_call(n, dim)
    seed = 77
    got = tile_run(call, seed, "f64")
    ref = g.oracle_tilegs(g.rounded(call), seed)
    dev = np.abs(got.positions - ref.positions).max()
    print(f"tile f64 n {n} ndim {dim}: max |dev| {dev:.3e}, MAE {got.final_mae!r} vs {ref.final_mae!r}")
    tol = 1e-11
    if dim == 1:
        # one dimension: near-coincident points make the repulsion stiff (tests/test_gpu_parity.py's slab band); the
        # wider allowance only where the oracle itself is chaotic over these iterations (a 1e-13 nudge of the start
        # moves its own answer, as tests/test_gpu_fuzz.py::test_slab_fuzz_against_model decides it)
        nudged = dataclasses.replace(g.rounded(call), initial_positions=call.initial_positions * (1 + 1e-13))
        moved = np.abs(g.oracle_tilegs(nudged, seed).positions - ref.positions).max()
        scale = max(1.0, np.abs(ref.positions).max())
        print(f"  ndim 1 nudge test: oracle moves by {moved:.3e}")
        if moved > 1e-10 * scale:
            tol = 1e-6 * scale
    assert got.positions.shape == (n, dim)
    assert dev <= tol
    assert got.iterations == ref.iterations and got.converged == ref.converged
    assert got.final_mae == pytest.approx(ref.final_mae, rel=1e-11)


TILE_F32 = [(n, d) for n in (130, 777) for d in (2, 5, 10, 16)] + [(33, 5)]


@pytest.mark.parametrize("n,dim", TILE_F32)
def test_tile_gs_f32_every_width(n, dim):
    """The float instantiations of the tile kernels (the fp32 pair update on encoded targets): two ragged sizes at four
    coordinate counts and one sub-tile problem, in the band fp32_ratio calibrates on the oracle's fp32 replay.
    Measured on MI355X, d_gpu / d_ref at ndim 2, 5, 10, 16: n = 130 1.37, 0.93, 0.88, 0.99 (d_ref 1.0e-5 .. 3.5e-5);
    n = 777 0.95, 0.98, 0.93, 0.97 (d_ref 9.5e-5 .. 6.3e-4); n = 33 at ndim 5 0.55 (d_ref 3.9e-6).  MAE against the
    fp32 replay 1e-7 .. 2.9e-6 relative, at most 0.64 of its band (n = 130, ndim 10: 2.1e-6 of 3.4e-6)."""
    call = tile_call(n, dim)
    seed = 78
    got = tile_run(call, seed, "f32")
    r = g.rounded(call)
    ref64, ref32 = g.oracle_tilegs(r, seed), g.oracle_tilegs(r, seed, "f32")
    assert got.positions.shape == (n, dim)
    fp32_ratio(got.positions, got.final_mae, ref64, ref32, call.initial_positions, f"tile fp32 n {n} ndim {dim}")


def test_tile_gs_f32_through_the_one_shot_entry():
    """2 100 points: past the one-shot entry's one-workgroup sizes, so schedule="gs" with precision="f32" takes the tile
    schedule's float kernels (33 blocks, the last of 52 points).  The reported MAE is the oracle's edge error of the
    returned positions on the targets the session keeps, in the band the fp32 slab path is held to (its check is the
    session's fp32 error pass, not an f64 one: measured on MI355X 4.0e-9 relative, above f64 rounding)."""
    call = g.problem(2100, 5, 0.7, seed=2100, thresholds=0.1, n_iter=60)
    got = _native.optimize_layout_exact_arrays(*layout_call_args(call), seed=1, schedule="gs", precision="f32")
    assert got.info["schedule"] == "gs" and got.info["precision"] == "f32" and got.positions.shape == (2100, 5)
    sm, cnt = orc.edge_error(got.positions, call.edge_i, call.edge_j, g.round_targets(call.edge_dist), call.edge_thresh)
    print("one-shot tile fp32: MAE", got.final_mae, "oracle", sm / cnt, "rel", abs(got.final_mae - sm / cnt) / (sm / cnt))
    assert got.final_mae == pytest.approx(sm / cnt, rel=2e-5)


# ----------------------------------------------------------------------------------------
# 5. the CV sweep above 2 048 points
# ----------------------------------------------------------------------------------------
def test_cv_sweep_above_2048_points_runs_the_strided_form():
    """A 2 100-point panel, 90 % missing: cv.likelihood_sweep's default routing keeps it on the one-workgroup kernel
    (batch_problem_fits) -- its strided form, the folds' edge lists standing for the matrix -- and must return what
    "sparse-calls" returns (one call object per fold through the batch entry): every field to the last bit, the random
    stream left in the same place."""
    n = 2100
    D = synthetic.make_problem(n, latent_dim=3, missing=0.9, seed=21).dissimilarity
    n_edges = int(np.triu(~np.isnan(D), 1).sum())
    assert _native.batch_problem_fits(n, 3, "f64", n_edges)
    sets = [dict(N=3, k0=4.0, cooling_rate=0.03, c_repulsion=0.01)]
    r1, r2 = np.random.default_rng(9), np.random.default_rng(9)
    a, _, na = cv.likelihood_sweep(D, sets, 20, 1e-4, folds=2, rng=r1)
    b, _, nb = cv.likelihood_sweep(D, sets, 20, 1e-4, folds=2, rng=r2, path="sparse-calls")
    assert na == nb == 2 and r1.uniform() == r2.uniform()
    print("sweep above 2 048:", a[0])
    assert np.isfinite(a[0]["Holdout_MAE"]) and len(a[0]["fold_mae"]) == 2
    assert a == b
