"""Cross-validation folds on a device-resident session (run with -m gpu): topolow_session_hold_out /
_restore_held_out / _score_pairs (topolow_amd/csrc/relax_cv.h), the sweep built on them (topolow_cv_sweep_session) and
its routing in cv.likelihood_sweep.

The shapes are small where the kernels can go wrong: 203 points -- not a multiple of 4 or 64, four 64-row tiles of the
symmetric sweep's tile-major copy with held-out pairs in its last, partial one -- and the derived flags (a fold that
holds out every threshold pair flips the session's threshold bit)."""
import functools
import os

import numpy as np
import pytest

from tests import parity_problems as pp
from topolow_amd import _native, core, cv, synthetic
from topolow_amd.sharded import _as_tensor

pytestmark = pytest.mark.gpu

N = 203
RELABEL = 0x5eed1
FULL_SYMMETRIC = dict(TOPOLOW_SYMMETRIC="1", TOPOLOW_SYMMETRIC_MIN_N="0", TOPOLOW_SYMMETRIC_STAGE_MIN_TILES="0")
# (precision, schedule, ndim, environment at session creation)
CASES = [(p, s, d, FULL_SYMMETRIC) for d in (2, 5) for p, s in (("f32", "slab"), ("f64", "slab"), ("f64", "gs"))]
CASES.append(("f32", "slab", 5, dict(TOPOLOW_SYMMETRIC="0")))
CASE_IDS = [f"{p}-{s}-ndim{d}{'-rowowner' if e is not FULL_SYMMETRIC else ''}" for p, s, d, e in CASES]
HIV = dict(N=2, k0=3.550036, cooling_rate=0.04130713, c_repulsion=0.0007038619)   # tests/test_gpu_assays.py


def problem(n=N, D=None, n_hold=280, always=(), which=("plain", "thresholds")):
    """A matrix as a session's input: the full edge list (upper triangle in np.nonzero order, 10 % of the measured pairs
    '>' codes), degrees, and hold-out sets with what they leave -- n_hold random edges, the edges at the list indices
    `always`, ends in the last, partial tile of rows, and the oddities a caller may send.  Without arguments the cached
    203 synthetic points, 60 % missing."""
    if D is None:
        assert (n, n_hold, tuple(always), tuple(which)) == (N, 280, (), ("plain", "thresholds"))
        return _default_problem()
    assert D.shape == (n, n)
    rng = np.random.default_rng(1)
    ei, ej = np.nonzero(np.triu(~np.isnan(D), 1))
    ed = D[ei, ej]
    et = (rng.uniform(size=ei.size) < 0.10).astype(np.int32)
    deg = (~np.isnan(D)).sum(axis=1).astype(np.int32)
    um_i, um_j = np.nonzero(np.triu(np.isnan(D), 1))
    tail = np.flatnonzero(ej >= (n - 1) // 64 * 64)        # an end in the last, partial tile of rows
    always = np.asarray(always, dtype=np.int64)

    def hold_set(extra):
        take = np.unique(np.concatenate([rng.choice(ei.size, n_hold, replace=False), tail[:12], always, extra]))
        hi, hj = ei[take].tolist(), ej[take].tolist()
        hi += [hj[0], hi[1], 7, int(um_i[0])]              # a pair again the other way round, a pair twice, i == j,
        hj += [ei[take][0], hj[1], 7, int(um_j[0])]        # an unmeasured pair
        keep = np.ones(ei.size, dtype=bool)
        keep[take] = False
        fdeg = deg.copy()
        np.subtract.at(fdeg, ei[take], 1)
        np.subtract.at(fdeg, ej[take], 1)
        return dict(pi=np.array(hi, np.int32), pj=np.array(hj, np.int32), keep=keep, deg=fdeg.astype(np.int32),
                    truth=np.concatenate([ed[take], [ed[take][0], ed[take][1], 1.25, 2.5]]))
    holds = {}
    if "plain" in which:
        holds["plain"] = hold_set(np.zeros(0, dtype=np.int64))
        assert not holds["plain"]["keep"].all() and (et[holds["plain"]["keep"]] != 0).any()
    if "thresholds" in which:
        holds["thresholds"] = hold_set(np.flatnonzero(et != 0))
        assert not (et[holds["thresholds"]["keep"]] != 0).any()
    return dict(n=n, ei=ei.astype(np.int32), ej=ej.astype(np.int32), ed=ed, et=et, deg=deg, holds=holds)


@functools.lru_cache(maxsize=1)
def _default_problem():
    return problem(N, synthetic.make_problem(N, latent_dim=5, missing=0.6, seed=5).dissimilarity)


def make_session(monkeypatch, precision, schedule, ndim, env, edges=None, deg=None, n=N, **kw):
    for k in ("TOPOLOW_SYMMETRIC", "TOPOLOW_SYMMETRIC_MIN_N", "TOPOLOW_SYMMETRIC_STAGE_MIN_TILES", "TOPOLOW_EDGE_MAE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = _native.Session(n, ndim, precision=precision, **kw)
    if schedule == "gs":
        s.set_schedule("gs")
    if edges is not None:
        s.set_relabel(RELABEL)
        s.load_coo(*edges, deg)
        s.set_edges(*edges)
    return s


def fold_edges(p, h):
    k = h["keep"]
    return p["ei"][k], p["ej"][k], p["ed"][k], p["et"][k]


def full_edges(p):
    return p["ei"], p["ej"], p["ed"], p["et"]


def block(s):
    import torch
    t = _as_tensor(torch, s.encoded_ptr, (s.n, s.encoded_ld), torch.int32, torch.device("cuda", torch.cuda.current_device()))
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def run(s, init, ndim, n_iter=40, seed=77):
    s.set_positions(init)
    s.begin(n_iter, 5.0, 0.02, 0.01, 1e-4, 5, 1, seed)
    s.run()
    trace = s.check_trace().copy()
    res = s.finish()
    return res, trace


def same_run(a, b):
    (ra, ta), (rb, tb) = a, b
    assert np.array_equal(ra.positions, rb.positions)
    assert np.array_equal(ta, tb) and ta.shape[0] >= 5
    assert (ra.converged, ra.iterations, ra.final_mae, ra.final_k) == (rb.converged, rb.iterations, rb.final_mae, rb.final_k)


def check_held_out_session(monkeypatch, p, h, precision, schedule, ndim, env, thresholds_left, run_first, inspect=None):
    """Block, flags and runs of a session of problem p with the set h held out equal, bit for bit, those of a fresh
    session loaded with the fold's list; after the restore the session equals one that never held anything out;
    score_pairs is the NumPy score of the positions finish() returns.  thresholds_left: whether the fold keeps a
    threshold pair; run_first: the session runs before the fold arrives; inspect(session): the caller's own assertions
    on each of the three sessions, once loaded, and on the held-out one again after its run."""
    n = p["n"]
    init = synthetic.initial_positions(np.full((n, n), 6.0), ndim, 3)
    s = make_session(monkeypatch, precision, schedule, ndim, env, full_edges(p), p["deg"], n=n)
    never = make_session(monkeypatch, precision, schedule, ndim, env, full_edges(p), p["deg"], n=n)
    fresh = make_session(monkeypatch, precision, schedule, ndim, env, fold_edges(p, h), h["deg"], n=n)
    try:
        for x in (s, never, fresh):
            if inspect is not None:
                inspect(x, False)
        original = block(s)
        assert s.has_thresholds
        if run_first:             # the sweep's copy exists already when the fold arrives: it is patched, not rebuilt
            same_run(run(s, init, ndim), run(never, init, ndim))
        s.hold_out(h["pi"], h["pj"], h["deg"])
        assert np.array_equal(block(s), block(fresh))
        assert s.has_thresholds == fresh.has_thresholds == thresholds_left
        held = run(s, init, ndim)
        same_run(held, run(fresh, init, ndim))
        if inspect is not None:
            inspect(s, True)
        # the score, on the device: i == j and the unmeasured pair count like every other entry
        pos = held[0].positions
        want = np.abs(h["truth"] - np.linalg.norm(pos[h["pi"]] - pos[h["pj"]], axis=1)).sum()
        got = s.score_pairs(h["pi"], h["pj"], h["truth"])
        assert got[1] == h["pi"].size and got[0] == pytest.approx(want, rel=1e-12)
        assert s.score_pairs(h["pi"], h["pj"], h["truth"]) == got
        assert s.score_pairs([], [], []) == (0.0, 0)
        s.restore_held_out(p["deg"])
        assert np.array_equal(block(s), original) and s.has_thresholds
        same_run(run(s, init, ndim), run(never, init, ndim))
        # ... and once more: the second fold meets a session whose copies were patched and put back
        s.hold_out(h["pi"], h["pj"], h["deg"])
        assert np.array_equal(block(s), block(fresh))
        same_run(run(s, init, ndim), held)
        s.restore_held_out(p["deg"])
        assert np.array_equal(block(s), original)
    finally:
        for x in (s, never, fresh):
            x.close()


@pytest.mark.parametrize("which", ["plain", "thresholds"])
@pytest.mark.parametrize("precision,schedule,ndim,env", CASES, ids=CASE_IDS)
def test_held_out_session_is_the_fresh_session_of_the_fold(monkeypatch, precision, schedule, ndim, env, which):
    """check_held_out_session on the 203-point problem: a fold that keeps threshold pairs, met by a session that has run
    already, and one that holds out every threshold pair and flips the session's threshold bit."""
    p = problem()
    check_held_out_session(monkeypatch, p, p["holds"][which], precision, schedule, ndim, env,
                           thresholds_left=which == "plain", run_first=which == "plain")


def test_a_block_loaded_over_a_held_out_fold_is_a_fresh_session(monkeypatch):
    """A fold is held out and run, then the full matrix is loaded again without a restore: a new block.  The hold is
    gone with the old one, the sweep's patched copy is invalid, and the next run is a fresh session's of the full
    matrix, bit for bit.  777 points: 13 tile-rows of the tile-major copy; one-stage iterations, checks on sweeps."""
    n, ndim = 777, 3
    call, _ = pp.random_problem(n, ndim, 0.7, seed=43, thresholds=0.0, n_iter=10, k0=1.5)
    edges = (call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
    take = np.random.default_rng(9).choice(call.edge_i.size, 200, replace=False)
    fdeg = np.asarray(call.degrees).copy()
    np.subtract.at(fdeg, call.edge_i[take], 1)
    np.subtract.at(fdeg, call.edge_j[take], 1)

    def nine(s):
        s.set_positions(call.initial_positions)
        s.begin(9, 1.5, 0.01, 0.01, 1e-12, 10 ** 9, 3, 77, 1)
        s.run()
        trace = s.check_trace().copy()
        return s.finish(), trace

    def same(a, b):
        (ra, ta), (rb, tb) = a, b
        return (np.array_equal(ra.positions, rb.positions) and np.array_equal(ta, tb) and ta.shape[0] == 3 and
                (ra.iterations, ra.final_mae, ra.final_k) == (rb.iterations, rb.final_mae, rb.final_k))

    s = make_session(monkeypatch, "f32", "slab", ndim, FULL_SYMMETRIC, edges, call.degrees, n=n)
    fresh = make_session(monkeypatch, "f32", "slab", ndim, FULL_SYMMETRIC, edges, call.degrees, n=n)
    try:
        want = nine(fresh)
        s.hold_out(call.edge_i[take], call.edge_j[take], fdeg)
        assert s.symm_grid > 0                                   # the copy the fold was patched into
        assert not same(nine(s), want)
        s.load_coo(*edges, call.degrees)
        assert same(nine(s), want)
        with pytest.raises(_native.NativeError, match="nothing is held out"):
            s.restore_held_out(call.degrees)
    finally:
        s.close()
        fresh.close()


def test_refusals_leave_the_session_usable(monkeypatch):
    p = problem()
    h = p["holds"]["plain"]
    init = synthetic.initial_positions(np.full((N, N), 6.0), 5, 3)
    s = make_session(monkeypatch, "f32", "slab", 5, FULL_SYMMETRIC, full_edges(p), p["deg"])
    ref = make_session(monkeypatch, "f32", "slab", 5, FULL_SYMMETRIC, full_edges(p), p["deg"])
    part = make_session(monkeypatch, "f32", "slab", 5, FULL_SYMMETRIC, row_begin=0, row_end=96)
    try:
        def refused(code, fn, *a):
            with pytest.raises(_native.NativeError) as e:
                fn(*a)
            assert e.value.code == code, e.value
        refused(_native.ERR_BAD_ARGUMENT, s.restore_held_out, p["deg"])              # nothing held out
        refused(_native.ERR_BAD_ARGUMENT, s.hold_out, [0], [N], h["deg"])             # a pair out of range
        s.set_positions(init)
        s.begin(40, 5.0, 0.02, 0.01, 1e-4, 5, 1, 77)
        s.enqueue(3)
        refused(_native.ERR_BAD_ARGUMENT, s.hold_out, h["pi"], h["pj"], h["deg"])    # during a run
        s.finish()
        s.hold_out(h["pi"], h["pj"], h["deg"])
        refused(_native.ERR_BAD_ARGUMENT, s.hold_out, h["pi"], h["pj"], h["deg"])    # twice
        s.restore_held_out(p["deg"])
        part.set_relabel(RELABEL)
        part.load_coo(*full_edges(p), p["deg"])
        part.set_edges(p["ei"][:0], p["ej"][:0], p["ed"][:0], p["et"][:0])
        refused(_native.ERR_UNSUPPORTED, part.hold_out, h["pi"], h["pj"], h["deg"])  # a row block
        same_run(run(s, init, 5), run(ref, init, 5))
    finally:
        for x in (s, ref, part):
            x.close()


def _mix64(z):
    m = (1 << 64) - 1
    z = (z + 0x9e3779b97f4a7c15) & m
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & m
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & m
    return z ^ (z >> 31)


def _sweep_by_hand(m, sets_of_fold, picks, draws, seeds, n_iter):
    """What topolow_cv_sweep_session documents, with the session primitives: one session per ndim, relabelled from the
    group's first seed, loaded once; per fold hold out / start / run / finish without download / score / restore."""
    fb = cv.FoldBuilder(m)
    n = fb.n
    up = fb.rows < fb.cols
    full = (fb.rows[up], fb.cols[up], fb.vals[up], fb.codes[up])
    deg = np.bincount(fb.rows, minlength=n).astype(np.int32)
    out = [None] * len(picks)
    for ndim in dict.fromkeys(ps["N"] for ps in sets_of_fold):
        members = [f for f, ps in enumerate(sets_of_fold) if ps["N"] == ndim]
        s = _native.Session(n, ndim, precision="f32")
        s.set_relabel(_mix64(seeds[members[0]] ^ 0x1abe15eed) | 1)
        s.load_coo(*full, deg)
        s.set_edges(*full)
        for f in members:
            ps = sets_of_fold[f]
            order, fdeg, vmax, n_edges, (pi, pj), (si, sj, st) = _native.cv_fold_pairs(fb.cells(), picks[f], False,
                                                                                      m.names is not None)
            if n_edges == 0:
                out[f] = _native.ERR_BAD_ARGUMENT
                continue
            steps = (0.0 + (2.0 * (vmax / n) - 0.0) * draws[f]).T
            walk = np.vstack([np.zeros((1, ndim)), np.cumsum(steps, axis=0)])
            init = np.empty_like(walk)
            init[np.arange(n) if order is None else order] = walk
            s.hold_out(pi, pj, fdeg)
            s.set_positions(init)
            s.begin(n_iter, ps["k0"], ps["cooling_rate"], ps["c_repulsion"], 1e-4, 5, 3, seeds[f])
            while s.enqueue(50) > 0:
                pass
            res = s.finish(download=False)
            total, count = s.score_pairs(si, sj, st)
            s.restore_held_out(deg)
            out[f] = (total, count, res.iterations, int(res.converged))
        s.close()
    return out


def test_sweep_equals_its_parts_on_the_hiv_panel():
    m = core.coded_matrix(pp.hiv_matrix())
    fb = cv.FoldBuilder(m)
    n = fb.n
    rng = np.random.default_rng(21)
    sets = [HIV, dict(N=3, k0=5.0, cooling_rate=0.02, c_repulsion=0.005)]
    sets_of_fold, picks, draws = [], [], []
    for ps in sets:
        for h in fb.folds(5, rng):
            sets_of_fold.append(ps); picks.append(h); draws.append(rng.random((ps["N"], n - 1)))
    seeds = [int(rng.integers(0, 2 ** 63 - 1)) for _ in picks]

    def sweep(pk):
        return _native.cv_sweep_session(fb.cells(), True, False, [ps["N"] for ps in sets_of_fold],
                                        [ps["k0"] for ps in sets_of_fold], [ps["cooling_rate"] for ps in sets_of_fold],
                                        [ps["c_repulsion"] for ps in sets_of_fold], pk, draws, seeds, 120, 1e-4, 5, 3)
    hsum, hcnt, its, conv, ec, secs = sweep(picks)
    hand = _sweep_by_hand(m, sets_of_fold, picks, draws, seeds, 120)
    assert secs > 0 and not ec.any()
    for f, want in enumerate(hand):
        assert (hsum[f], hcnt[f], its[f], conv[f]) == want, f
    assert hcnt.min() > 0 and np.all(np.isfinite(hsum))
    # one fold without a valid measurement (every cell picked): it reports its code, the others are unchanged
    bad = list(picks)
    bad[3] = fb.rows + fb.cols * n
    hsum2, hcnt2, its2, conv2, ec2, _ = sweep(bad)
    assert ec2[3] == _native.ERR_BAD_ARGUMENT and hcnt2[3] == 0 and not np.delete(ec2, 3).any()
    for a, b in ((hsum, hsum2), (hcnt, hcnt2), (its, its2), (conv, conv2)):
        assert np.array_equal(np.delete(a, 3), np.delete(b, 3))
    # ... and one that diverges
    wild = [dict(ps) for ps in sets_of_fold]
    k0 = [ps["k0"] for ps in sets_of_fold]
    k0[6] = 1e30
    out = _native.cv_sweep_session(fb.cells(), True, False, [ps["N"] for ps in wild], k0,
                                   [ps["cooling_rate"] for ps in wild], [ps["c_repulsion"] for ps in wild], picks, draws,
                                   seeds, 120, 1e-4, 5, 3)
    assert out[4][6] == _native.ERR_NONFINITE and not np.delete(out[4], 6).any()
    for a, b in ((hsum, out[0]), (hcnt, out[1]), (its, out[2]), (conv, out[3])):
        assert np.array_equal(np.delete(a, 6), np.delete(b, 6))


def test_session_path_takes_the_same_folds_from_the_same_stream():
    hv = pp.hiv_matrix()
    r1, r2 = np.random.default_rng(9), np.random.default_rng(9)
    sets = [HIV, dict(N=3, k0=5.0, cooling_rate=0.02, c_repulsion=0.005)]
    a, _, na = cv.likelihood_sweep(hv, sets, 60, 1e-4, folds=5, rng=r1, path="session")
    b, _, nb = cv.likelihood_sweep(hv, sets, 60, 1e-4, folds=5, rng=r2, path="sparse")
    assert na == nb == 10 and r1.uniform() == r2.uniform()
    for x, y in zip(a, b):
        assert x["fold_n_samples"] == y["fold_n_samples"] and len(x["fold_n_samples"]) == 5
        assert np.isfinite(x["Holdout_MAE"])


def test_tile_gauss_seidel_sweep_meets_the_batch_paths_rule_on_hiv():
    """The reference's arithmetic pair by pair (tile Gauss-Seidel, f64) on sessions, held to the rule of
    tests/test_gpu_assays.py::test_config5_batched_cv_matches_published_holdout_mae: 20 folds at the published
    parameters against the reference's 20 per-fold errors (3 standard errors of the difference of the means) and its
    pooled figure 1.315 (7 %).  Measured on MI355X: pooled 1.300, fold mean 1.300 (reference 1.329), all folds
    converged."""
    res, secs, n_emb = cv.likelihood_sweep(pp.hiv_matrix(), [HIV], 500, 1e-4, folds=20, rng=np.random.default_rng(11),
                                           path="session", schedule="gs")
    r = res[0]
    f, ref = np.array(r["fold_mae"]), pp.ref_fold_stats("HIV")
    print("tile GS on sessions: pooled", r["Holdout_MAE"], "fold mean", f.mean(), "reference", ref.mean(),
          "pct_converged", r["pct_converged"])
    assert n_emb == 20 and f.size == 20 and r["pct_converged"] >= 50
    se = np.hypot(f.std(ddof=1) / np.sqrt(20), ref.std(ddof=1) / np.sqrt(20))
    assert abs(f.mean() - ref.mean()) <= 3 * se, (f.mean(), ref.mean(), se)
    assert abs(r["Holdout_MAE"] / 1.315 - 1) <= 0.07, r["Holdout_MAE"]


def test_slab_sweep_is_at_the_level_of_the_batch_path_on_hiv():
    """The slab schedule on sessions against the exact batch path on the same folds, pooled Holdout_MAE over 5
    generator seeds, in the 5 % band the project states for the slab schedule on a small sparse panel
    (tests/test_gpu_assays.py::test_config2_slab_schedule_on_h3n2_when_forced).  Measured on MI355X, session / batch per
    seed: 1.0046, 1.0142, 0.9961, 0.9997, 0.9933 (mean +0.16 %)."""
    hv = pp.hiv_matrix()
    ratios = []
    for seed in range(5):
        a, _, _ = cv.likelihood_sweep(hv, [HIV], 500, 1e-4, folds=20, rng=np.random.default_rng(seed), path="session",
                                      schedule="slab")
        b, _, _ = cv.likelihood_sweep(hv, [HIV], 500, 1e-4, folds=20, rng=np.random.default_rng(seed), path="sparse")
        assert len(a[0]["fold_mae"]) == 20
        ratios.append(a[0]["Holdout_MAE"] / b[0]["Holdout_MAE"])
    print("slab on sessions / batch, pooled Holdout_MAE per seed:", ratios)
    assert abs(np.mean(ratios) - 1) <= 0.05, ratios


def test_a_matrix_beyond_one_workgroup_is_routed_to_the_session_sweep():
    n = 3000
    D = synthetic.make_problem(n, latent_dim=5, missing=0.7, seed=4).dissimilarity
    assert not _native.batch_problem_fits(n, 5, "f64", 0)
    m = core.coded_matrix(D)
    picks = cv.FoldBuilder(m).folds(2, np.random.default_rng(6))      # the folds the sweep will draw first
    res, secs, n_emb = cv.likelihood_sweep(m, [dict(N=5, k0=5.0, cooling_rate=0.01, c_repulsion=0.01)], 30, 1e-4,
                                           folds=2, rng=np.random.default_rng(6))
    assert n_emb == 2 and np.isfinite(res[0]["Holdout_MAE"])
    want = []
    for h in picks:
        r, c = h % n, h // n
        cells = np.unique(np.concatenate([r + c * n, c + r * n]))
        v, k = m.values[cells % n, cells // n], m.codes[cells % n, cells // n]
        want.append(int(np.sum(~np.isnan(v) & (k == 0))))
    assert res[0]["fold_n_samples"] == want
