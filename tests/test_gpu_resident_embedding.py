"""The resident embedding -- a session, the whole relaxation and the post-metrics read from a prepared handle -- against
the present route over the arrays the handle's fetch() returns: the same bits everywhere."""
import os

import numpy as np
import pytest

from tests import resident_helpers as rh
from topolow_amd import _native, core

pytestmark = pytest.mark.gpu

same = rh.same_bits


class _Env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _laid_out(D, codes, layout):
    if layout == "F":
        return np.asfortranarray(D), None if codes is None else np.asfortranarray(codes)
    return D, codes


def _initial_edge_error(s, init):
    """topolow_session_edge_error of `init`, laid out as the session lays positions out (session labels, padded)."""
    import torch
    rows, dim = s.position_rows, int(s.lib.topolow_session_position_dim(s._h))
    f64 = s.precision != "f32"
    buf = np.zeros((rows, dim), dtype=np.float64 if f64 else np.float32)
    buf[:s.n, :s.ndim] = init[s.labels()]
    buf[s.n:, 0] = 1e150 if f64 else 1e18
    t = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    out = s.edge_error(t.data_ptr())
    del t
    return out


def _observe(s, init, seed, runs):
    """What the tests compare of a loaded session: the flags, the edge error of the start, and per run -- (n_iter, k0,
    check_freq, slab_stages) -- the positions and the check trace."""
    seen = [s.uses_dense_mae, s.has_thresholds, _initial_edge_error(s, init)]
    for n_iter, k0, freq, stages in runs:
        s.set_positions(init)
        s.begin(n_iter, k0, 0.01, 0.01, 1e-12, 10 ** 9, freq, seed, stages)
        s.run()
        s.sync()
        seen.append((s.get_positions(), s.check_trace().copy()))
    return seen


def _assert_same_observations(a, b, what):
    assert a[0] == b[0], ("uses_dense_mae",) + what
    assert a[1] == b[1], ("has_thresholds",) + what
    assert a[2] == b[2], ("edge_error of the start",) + what
    for q, (x, y) in enumerate(zip(a[3:], b[3:])):
        assert same(x[0], y[0]), ("positions, run %d" % q,) + what
        assert same(x[1], y[1]) and len(x[1]) > 0, ("check_trace, run %d" % q,) + what


RUNS = ((7, 5.0, 3, 1), (7, 5.0, 3, 2))     # 7 iterations, a check every 3rd: one stage, then slab_stages = 2


# ---- 1. a session from a handle equals a session from its fetch ------------------------------------------------------

@pytest.mark.parametrize("thresholds", [0.0, 0.15])
@pytest.mark.parametrize("missing", [0.3, 0.7])
@pytest.mark.parametrize("n", [33, 66, 257, 1100])
def test_session_from_a_handle_equals_session_from_its_fetch(n, missing, thresholds):
    """Below, just above and not a multiple of the 64 x 64 prep tiles, and above the device-prep gate; C and Fortran
    input, reordered and preserved, the three precisions, relabel seed 0 and 77, one-stage and two-stage iterations on
    the slab schedule (a Session's own): everything a run reads or reports, bit for bit."""
    D, codes = rh.problem(n, missing, thresholds)
    init = rh.start_positions(n, 3, n)
    for layout in ("C", "F"):
        Dl, cl = _laid_out(D, codes, layout)
        for preserve in (False, True):
            with _native.PreparedHandle(Dl, cl, preserve_order=preserve) as h:
                assert not h.declined and bool(h.info["reordered"]) == (not preserve)
                f = h.fetch(want_reordered=False)
                for precision in ("f32", "f64", "f64_exact"):
                    for relabel in (0, 77):
                        what = (n, missing, thresholds, layout, preserve, precision, relabel)
                        s = _native.Session(n, 3, precision=precision)
                        s.set_relabel(relabel)
                        s.load_prepared(h)
                        got = _observe(s, init, 5, RUNS)
                        s.close()
                        c = _native.Session(n, 3, precision=precision)
                        c.set_relabel(relabel)
                        c.load_dense(f.dense, f.tdense, f.degrees)
                        c.set_edges(f.edge_i, f.edge_j, f.edge_dist, f.edge_thresh)
                        want = _observe(c, init, 5, RUNS)
                        c.close()
                        _assert_same_observations(got, want, what)
                        if precision == "f32":
                            assert got[0], what     # the list is the block: the check reads the block
                            c = _native.Session(n, 3, precision=precision)
                            c.set_relabel(relabel)
                            c.load_coo(f.edge_i, f.edge_j, f.edge_dist, f.edge_thresh, f.degrees)
                            c.set_edges(f.edge_i, f.edge_j, f.edge_dist, f.edge_thresh)
                            _assert_same_observations(got, _observe(c, init, 5, RUNS), what + ("coo",))
                            c.close()
                        else:
                            assert not got[0], what


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_forced_edge_list_pass_gathers_the_device_built_list(precision):
    """TOPOLOW_EDGE_MAE=1: the session gathers the list whatever the precision -- the list the new kernel wrote."""
    n = 257
    D, codes = rh.problem(n, 0.7, 0.15)
    init = rh.start_positions(n, 3, n)
    with _Env(TOPOLOW_EDGE_MAE="1"), _native.PreparedHandle(D, codes) as h:
        s = _native.Session(n, 3, precision=precision)
        s.set_relabel(77)
        s.load_prepared(h)                      # before any fetch(): this call compacts the handle's list
        f = h.fetch(want_reordered=False)
        c = _native.Session(n, 3, precision=precision)
        c.set_relabel(77)
        c.load_dense(f.dense, f.tdense, f.degrees)
        c.set_edges(f.edge_i, f.edge_j, f.edge_dist, f.edge_thresh)
        got, want = _observe(s, init, 5, RUNS), _observe(c, init, 5, RUNS)
        s.close()
        c.close()
    assert not got[0]
    _assert_same_observations(got, want, (precision,))


# ---- 2. the same on the symmetric sweep ---------------------------------------------------------------------------------

@pytest.mark.parametrize("ndim,precision", [(5, "f32"), (5, "f64"), (5, "f64_exact"), (8, "f32")])
def test_symmetric_sweep_on_a_session_from_a_handle(ndim, precision):
    """n = 1100 with the size gate at zero: every iteration a sweep (the tile-major copy, and for f64 the delta tiles,
    are made from what load_prepared left -- the block and the device-built edge list), fused checks included."""
    n = 1100
    D, codes = rh.problem(n, 0.7, 0.15)
    init = rh.start_positions(n, ndim, n + ndim)
    runs = ((6, 1.5, 1, 1),)      # k <= 3: one-stage iterations; a check after every iteration rides on the next sweep
    seen = []
    with _native.PreparedHandle(D, codes) as h:
        f = h.fetch(want_reordered=False)
        for from_handle in (True, False):
            with _Env(TOPOLOW_SYMMETRIC="1", TOPOLOW_SYMMETRIC_MIN_N="0"):
                s = _native.Session(n, ndim, precision=precision)
            s.set_relabel(77)
            if from_handle:
                s.load_prepared(h)
            else:
                s.load_dense(f.dense, f.tdense, f.degrees)
                s.set_edges(f.edge_i, f.edge_j, f.edge_dist, f.edge_thresh)
            s.set_profiling(True)
            seen.append(_observe(s, init, 5, runs))
            plain_ms, plain_n, fused_ms, fused_n = s.profile_symmetric()
            assert plain_n + fused_n == 6 and fused_n >= 1, (from_handle, plain_n, fused_n)
            s.close()
    _assert_same_observations(seen[0], seen[1], (ndim, precision))


# ---- 3. optimize against optimize_layout_exact_arrays on the fetched arrays -----------------------------------------------

RUN_KW = dict(n_iter=60, k0=5.0, cooling_rate=0.01, c_repulsion=0.01, relative_epsilon=1e-4, convergence_window=5,
              convergence_check_freq=3)


def _arrays_run(f, init, verbose=False, **opt_kw):
    return _native.optimize_layout_exact_arrays(
        init, f.dense, f.tdense, f.degrees, f.edge_i, f.edge_j, f.edge_dist, f.edge_thresh, RUN_KW["n_iter"],
        RUN_KW["k0"], RUN_KW["cooling_rate"], RUN_KW["c_repulsion"], RUN_KW["relative_epsilon"],
        RUN_KW["convergence_window"], RUN_KW["convergence_check_freq"], verbose, **opt_kw)


@pytest.mark.parametrize("n,opt_kw,schedule,precision", [
    (300, dict(), "gs", "f64"),                      # AUTO: one-workgroup Gauss-Seidel
    (1100, dict(), "slab", "f32"),                   # AUTO: slab
    (2100, dict(schedule="gs"), "gs", "f64"),        # beyond the LDS: tile Gauss-Seidel
])
def test_optimize_equals_the_call_on_the_fetched_arrays(n, opt_kw, schedule, precision):
    D, codes = rh.problem(n, 0.7, 0.15)
    init = rh.start_positions(n, 5, n)
    with _native.PreparedHandle(D, codes) as h:
        before = h.fetch()
        lines_h, lines_a = [], []
        got = h.optimize(init, 5, verbose=True, seed=9, print=lines_h.append, **RUN_KW, **opt_kw)
        want = _arrays_run(before, init, verbose=True, seed=9, print=lines_a.append, **opt_kw)
        assert same(got.positions, want.positions)
        assert (got.converged, got.iterations) == (want.converged, want.iterations)
        assert same(np.float64(got.final_mae), np.float64(want.final_mae))
        assert same(np.float64(got.final_k), np.float64(want.final_k))
        assert got.info["schedule"] == want.info["schedule"] == schedule
        assert got.info["precision"] == want.info["precision"] == precision
        assert got.info["iterations_run"] == want.info["iterations_run"]
        assert lines_h == lines_a and len(lines_h) >= 4

        # An interrupt on the second poll.  A session is polled once per 50 enqueued iterations, so 60 iterations that
        # cannot stop early give exactly two polls.  The one-workgroup kernel is one launch, polled per 50 iterations
        # of progress or 50 ms: only a run that cannot end before its second poll makes the case deterministic.
        polls = []

        def second_poll():
            polls.append(1)
            return len(polls) >= 2

        long_run = dict(RUN_KW, relative_epsilon=1e-12, convergence_window=10 ** 9)
        if schedule == "gs" and not opt_kw:
            long_run["n_iter"] = 20000
        with pytest.raises(_native.NativeError) as e:
            h.optimize(init, 5, seed=9, interrupt=second_poll, **long_run, **opt_kw)
        assert e.value.code == _native.ERR_INTERRUPTED and len(polls) == 2

        after = h.fetch()       # the handle is not consumed
        for field in ("order", "degrees", "edge_i", "edge_j", "edge_dist", "edge_thresh", "dense", "tdense",
                      "values_reordered", "codes_reordered"):
            assert same(getattr(before, field), getattr(after, field)), field
        assert np.array_equal(h.order, before.order)


# ---- 4. post_metrics on the handle ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("preserve", [False, True])
@pytest.mark.parametrize("layout", ["C", "F"])
@pytest.mark.parametrize("n", [66, 1100])
def test_post_metrics_on_the_handle(n, layout, preserve, monkeypatch):
    D, codes = rh.problem(n, 0.7, 0.15)
    D = D.copy()
    D[3, 7] = np.inf        # a non-finite value never counts
    D[n - 1, n - 1] = 0.5   # the diagonal counts like any other cell
    Dl, cl = _laid_out(D, codes, layout)
    pos = np.random.default_rng(n).normal(size=(n, 5)) * 3.0
    h = _native.PreparedHandle(Dl, cl, preserve_order=preserve)
    if h.declined:      # the infinite cell: the device leaves the ordering to the host
        h.close()
        h = _native.PreparedHandle(Dl, cl, order=core.spectral_order(Dl))
    with h:
        order = h.order
        assert (order is None) == preserve
        cm = core.CodedMatrix(Dl, cl, None, True)
        rm = cm.reordered(order) if order is not None else cm
        numeric = np.ascontiguousarray(rm.as_numeric())     # what device_post hands to post_metrics today
        est0, sum0, count0 = _native.post_metrics(pos, numeric)
        est, sum_abs, count = h.post_metrics(pos)
        assert same(est, est0) and same(est, _native.est_distances(pos))
        assert count == count0 and count > 0
        if layout == "C":     # a line of the handle is a row of the matrix, as a line of the C-ordered matrix is
            assert same(np.float64(sum_abs), np.float64(sum0))
        else:                 # a line is a column: the same terms, grouped by columns instead of rows
            assert abs(sum_abs / count - sum0 / count0) <= 1e-12 * (sum0 / count0)
            by_columns = _native.post_metrics(pos, np.asfortranarray(numeric), want_est=False)
            assert same(np.float64(sum_abs), np.float64(by_columns[1])) and by_columns[2] == count
        monkeypatch.setenv("TOPOLOW_POST_TILE_COLS", "17")
        est17, sum17, count17 = h.post_metrics(pos)
        monkeypatch.delenv("TOPOLOW_POST_TILE_COLS")
        assert same(est17, est) and same(np.float64(sum17), np.float64(sum_abs)) and count17 == count
        none, sum_n, count_n = h.post_metrics(pos, want_est=False)
        assert none is None and same(np.float64(sum_n), np.float64(sum_abs)) and count_n == count


# ---- 5. euclidean_embedding() resident against the present route ----------------------------------------------------------

def _embed(D, resident, seed=21, **kw):
    args = dict(ndim=5, mapping_max_iter=20, k0=5.0, cooling_rate=0.01, c_repulsion=0.01)
    args.update(kw)
    with _Env(TOPOLOW_RESIDENT="1" if resident else "0", TOPOLOW_DEVICE_PREP="1"):
        _native.set_seed(seed)
        return core.euclidean_embedding(D, **args)


def _assert_same_topolow(a, b, mae_bits):
    assert same(a.positions, b.positions)
    assert same(a.est_distances, b.est_distances)
    if mae_bits:
        assert same(np.float64(a.mae), np.float64(b.mae))
    else:
        assert abs(a.mae - b.mae) <= 1e-12 * b.mae
    assert a.iter == b.iter and a.parameters == b.parameters and a.convergence == b.convergence
    assert a.names == b.names
    for key in ("schedule", "precision", "iterations_run", "n_checks", "seed", "stage_launches"):
        assert a.native_info[key] == b.native_info[key], key


def test_euclidean_embedding_resident_equals_the_present_route(capfd, monkeypatch):
    n = 1100
    D, codes = rh.problem(n, 0.7, 0.15)
    names = ["s%04d" % q for q in range(n)]
    made = []
    real = _native.PreparedHandle

    class Counting(real):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self.info["order_route"])

    monkeypatch.setattr(_native, "PreparedHandle", Counting)

    def both(D_, mae_bits=True, **kw):
        capfd.readouterr()      # the file descriptor: the library's own verbose lines are part of the comparison
        del made[:]
        a = _embed(D_, True, verbose=True, **kw)
        lines_a = capfd.readouterr().out
        assert made, "the resident route did not run"
        routes = list(made)
        b = _embed(D_, False, verbose=True, **kw)
        lines_b = capfd.readouterr().out
        strip = [ln for ln in lines_a.splitlines() if not ln.startswith("Optimization finished in")]
        assert strip == [ln for ln in lines_b.splitlines() if not ln.startswith("Optimization finished in")]
        assert len(strip) >= 6 and any(ln.startswith("Iter ") for ln in strip)
        _assert_same_topolow(a, b, mae_bits)
        return a, routes

    both(D)                                                                  # a plain C array
    both(np.asfortranarray(D), mae_bits=False)                               # Fortran input: mae to 1e-12
    a, _ = both(core.CodedMatrix(D, codes, names, True))                     # row names, thresholds
    assert a.names != names and sorted(a.names) == names
    shuffled = np.random.default_rng(2).permutation(n)
    init = core.RMatrix(rh.start_positions(n, 5, 4)[shuffled], [names[q] for q in shuffled])
    both(core.CodedMatrix(D, codes, names, True), initial_positions=init)    # named start positions in shuffled order
    a, routes = both(core.RMatrix(D, names), preserve_order=True)
    assert a.names == names and routes == [_native.ORDER_PRESERVED]
    # an input the device declines to order: inexact keys with one negative cell; the host orders, a second handle runs
    Dn = D.copy()
    Dn[2, 5] = -0.3
    a, routes = both(Dn)
    assert routes == [_native.ORDER_DECLINED, _native.ORDER_DECLINED]


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_session_usable():
    n = 66
    D, codes = rh.problem(n, 0.3, 0.15)
    Dn = D.copy()
    Dn[2, 5] = -0.3
    init = rh.start_positions(n, 3, n)
    with _native.PreparedHandle(D, codes) as h, _native.PreparedHandle(Dn, codes) as declined, \
            _native.PreparedHandle(rh.problem(33, 0.3, 0.0)[0]) as small:
        assert declined.declined and declined.info["order_route"] == _native.ORDER_DECLINED
        s = _native.Session(n, 3)
        for bad, word in ((declined, "declined"), (small, "33 points")):
            with pytest.raises(_native.NativeError) as e:
                s.load_prepared(bad)
            assert e.value.code == _native.ERR_BAD_ARGUMENT and word in str(e.value)
        block = _native.Session(n, 3, row_begin=0, row_end=32)
        with pytest.raises(_native.NativeError) as e:
            block.load_prepared(h)
        assert e.value.code == _native.ERR_BAD_ARGUMENT and "whole-problem" in str(e.value)
        block.close()
        with pytest.raises(_native.NativeError) as e:
            h.optimize(init, 3, devices=[0, 0], **RUN_KW)
        assert e.value.code == _native.ERR_UNSUPPORTED and "sharded" in str(e.value)
        for call in (lambda: declined.optimize(init, 3, **RUN_KW), lambda: declined.post_metrics(init)):
            with pytest.raises(_native.NativeError) as e:
                call()
            assert e.value.code == _native.ERR_BAD_ARGUMENT and "declined" in str(e.value)
        # the session that refused twice loads and runs as a fresh one does
        s.load_prepared(h)
        got = _observe(s, init, 5, RUNS)
        s.close()
        c = _native.Session(n, 3)
        c.load_prepared(h)
        _assert_same_observations(got, _observe(c, init, 5, RUNS), ("after refusals",))
        c.close()


# ---- 7. the .Call round trip --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return rh.build_harness(tmp_path_factory.mktemp("resident_harness"))


@pytest.mark.parametrize("n", [66, 300])
def test_dot_call_round_trip(harness, tmp_path, n):
    D, codes = rh.problem(n, 0.7, 0.15)
    init = rh.start_positions(n, 3, n)
    kw = dict(n_iter=20, k0=5.0, cooling_rate=0.01, c_repulsion=0.01, relative_epsilon=1e-4, convergence_window=5,
              convergence_check_freq=3)
    res = rh.run_harness(harness, tmp_path, D, codes.astype(np.int32), None, init, 3, seed=7, verbose=True)
    assert res["error"] is None and res["protect_depth"] == 0
    assert res["names"] == ["positions", "est_distances", "sum_abs", "count", "order", "converged", "iterations",
                            "final_mae", "final_k", "order_route", "numeric_max"]
    # R's matrices are column-major: the handle reads the same matrix with transposed = 0
    with _native.PreparedHandle(np.asfortranarray(D), np.asfortranarray(codes)) as h:
        lines = []
        want = h.optimize(init, 3, seed=7, verbose=True, print=lines.append, **kw)
        est, sum_abs, count = h.post_metrics(want.positions)
        assert res["order_route"] == h.info["order_route"] and res["numeric_max"] == h.info["numeric_max"]
        assert res["order"] == (h.order + 1).tolist()
    assert same(np.array(res["positions"]).reshape(3, n).T, want.positions)
    assert same(np.array(res["est_distances"]).reshape(n, n).T, est)
    assert res["sum_abs"] == sum_abs and res["count"] == count
    assert (bool(res["converged"]), res["iterations"]) == (want.converged, want.iterations)
    assert res["final_mae"] == want.final_mae and res["final_k"] == want.final_k
    assert res["printed"] == "".join(lines)
    # a declined first call returns the route and the scale alone; the caller orders and calls again
    Dn = D.copy()
    Dn[2, 5] = -0.3
    res = rh.run_harness(harness, tmp_path, Dn, None, None, init, 3, want_est=False)
    assert res["error"] is None and res["order_route"] == 3 and res["positions"] is None and res["order"] is None
    assert res["protect_depth"] == 0 and res["numeric_max"] == np.nanmax(Dn)
    order = core.spectral_order(Dn)
    res = rh.run_harness(harness, tmp_path, Dn, None, order + 1, init, 3, want_est=False)
    assert res["error"] is None and res["order"] == (order + 1).tolist() and res["est_distances"] is None
    with _native.PreparedHandle(np.asfortranarray(Dn), None, order=order) as h:
        want = h.optimize(init, 3, seed=7, **kw)
        assert same(np.array(res["positions"]).reshape(3, n).T, want.positions)
        assert res["sum_abs"] == h.post_metrics(want.positions, want_est=False)[1]
    # an interrupt on the second poll is re-raised after the handle is gone
    if n == 300:
        res = rh.run_harness(harness, tmp_path, D, None, None, init, 3, n_iter=200, interrupt_after=2)
        assert res["error"] == "interrupted by the caller" and res["interrupted"] == 1 and res["protect_depth"] == 0
