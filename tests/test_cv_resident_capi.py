"""Cross-validation folds from a prepared handle, without a device: the two C entries (declared with the documented
argument lists, exported, argument errors before any device call), the routing of cv.likelihood_sweep(path="resident")
with the native layer replaced, and the ordering rule on the input the GPU decline test relies on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from topolow_amd import _native, cv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOLD_ARGS = ("p picks n_picks preserve_order named order degrees numeric_max n_edges pair_i pair_j n_pairs score_i "
             "score_j score_truth n_scored order_route errbuf errlen").split()
SWEEP_ARGS = ("p named preserve_order n_folds ndim k0 cooling_rate c_repulsion picks picks_offset unit_draws draws_offset "
              "seeds n_iter relative_epsilon convergence_window convergence_check_freq precision schedule holdout_sum_abs "
              "holdout_count iterations converged error_code order_route device_seconds errbuf errlen").split()


def _declared_arguments(name):
    header = open(os.path.join(ROOT, "include", "topolow_relax.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, header, flags=re.S)
    assert m, name
    return [re.split(r"[\s\*]+", a.strip())[-1] for a in m.group(1).split(",")]


def test_symbols_are_declared_and_exported_with_the_documented_arguments():
    lib = _native.load()
    for name, args in (("topolow_layout_prep_fold", FOLD_ARGS), ("topolow_layout_prep_cv_sweep", SWEEP_ARGS)):
        assert _declared_arguments(name) == args
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(args)
    assert len(FOLD_ARGS) == 19 and len(SWEEP_ARGS) == 28
    for name in ("fold", "cv_sweep"):
        assert hasattr(_native.PreparedHandle, name)
    assert (_native.ORDER_PRESERVED, _native.ORDER_DEVICE_EXACT, _native.ORDER_DEVICE_GAP, _native.ORDER_DECLINED) == (0, 1, 2, 3)


def test_argument_errors_come_before_any_device_call():
    """TOPOLOW_ERR_BAD_ARGUMENT with or without a GPU: every NULL and a negative count are found before the handle (here
    a pointer to zeroed memory that nothing may read) is looked at; an empty sweep is TOPOLOW_OK."""
    lib = _native.load()
    err = C.create_string_buffer(256)
    scratch = np.zeros(4096, dtype=np.float64)
    some = scratch.ctypes.data_as(C.c_void_p)
    dp = scratch.ctypes.data_as(C.POINTER(C.c_double))
    ip = scratch.ctypes.data_as(C.POINTER(C.c_int32))
    i64 = scratch.ctypes.data_as(C.POINTER(C.c_int64))
    u64 = scratch.ctypes.data_as(C.POINTER(C.c_uint64))
    bad = _native.ERR_BAD_ARGUMENT

    def fold(**kw):
        a = dict(p=some, picks=i64, n_picks=1, order=ip, degrees=ip, numeric_max=dp, n_edges=i64, pair_i=ip, pair_j=ip,
                 n_pairs=i64, score_i=ip, score_j=ip, score_truth=dp, n_scored=i64, order_route=ip)
        a.update(kw)
        return lib.topolow_layout_prep_fold(a["p"], a["picks"], a["n_picks"], 0, 1, a["order"], a["degrees"],
                                            a["numeric_max"], a["n_edges"], a["pair_i"], a["pair_j"], a["n_pairs"],
                                            a["score_i"], a["score_j"], a["score_truth"], a["n_scored"], a["order_route"],
                                            err, len(err))

    for key in ("p", "picks", "order", "degrees", "numeric_max", "n_edges", "pair_i", "pair_j", "n_pairs", "score_i",
                "score_j", "score_truth", "n_scored", "order_route"):
        err.value = b""
        assert fold(**{key: None}) == bad, key
        assert err.value, key
    assert fold(n_picks=-1) == bad

    def sweep(n_folds=1, **kw):
        a = dict(p=some, ndim=ip, k0=dp, cooling_rate=dp, c_repulsion=dp, picks=i64, picks_offset=i64, unit_draws=dp,
                 draws_offset=i64, seeds=u64, holdout_sum_abs=dp, holdout_count=i64, iterations=ip, converged=ip,
                 error_code=ip, order_route=ip, schedule=0)
        a.update(kw)
        return lib.topolow_layout_prep_cv_sweep(a["p"], 1, 0, n_folds, a["ndim"], a["k0"], a["cooling_rate"],
                                                a["c_repulsion"], a["picks"], a["picks_offset"], a["unit_draws"],
                                                a["draws_offset"], a["seeds"], 10, 1e-4, 5, 3, _native.PRECISION_AUTO,
                                                a["schedule"], a["holdout_sum_abs"], a["holdout_count"], a["iterations"],
                                                a["converged"], a["error_code"], a["order_route"], None, err, len(err))

    for key in ("p", "ndim", "k0", "cooling_rate", "c_repulsion", "picks_offset", "unit_draws", "draws_offset", "seeds",
                "holdout_sum_abs", "holdout_count", "iterations", "converged", "error_code", "order_route"):
        err.value = b""
        assert sweep(**{key: None}) == bad, key
        assert err.value, key
    assert sweep(n_folds=-1) == bad
    assert sweep(schedule=17) == bad
    assert sweep(n_folds=0) == _native.OK
    assert sweep(n_folds=0, ndim=None, seeds=None, error_code=None, order_route=None) == _native.OK
    assert lib.topolow_layout_prep_fold_seconds(None, dp) == bad


def test_two_equal_keys_on_inexact_sums_are_declined():
    """Two interchangeable points have the same sums, hence the same non-zero key: on sums that are not exact the rule
    cannot tell which of them NumPy puts first (tests/test_gpu_cv_resident.py builds such a matrix)."""
    rs = np.array([0.3, 0.7, 0.7, 1.9])
    cnt = np.array([3, 3, 3, 3])
    route, order = _native.order_from_sums(rs, cnt, rs, cnt, 0)
    assert route == _native.ORDER_DECLINED and order is None
    route, order = _native.order_from_sums(rs, cnt, rs, cnt, 1)        # exact sums: a tie is a tie in both
    assert route == _native.ORDER_DEVICE_EXACT and order.tolist() == [0, 1, 2, 3]
    apart = np.array([0.3, 0.7, 0.9, 1.9])
    assert _native.order_from_sums(apart, cnt, apart, cnt, 0)[0] == _native.ORDER_DEVICE_GAP


# ---- cv.likelihood_sweep(path="resident"), the native layer replaced -------------------------------------------------

def _matrix(n=12, seed=3):
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3))
    D = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))
    D[1, 7] = D[7, 1] = np.nan
    return D


SETS = [dict(N=2, k0=3.0, cooling_rate=0.02, c_repulsion=0.01), dict(N=3, k0=5.0, cooling_rate=0.01, c_repulsion=0.02)]


class _FakeHandle:
    declined = ()
    log = []

    def __init__(self, values, codes=None, preserve_order=False, **kw):
        _FakeHandle.log.append(("create", values.shape, codes is None, preserve_order))

    def cv_sweep(self, named, preserve_order, nd, k0, cr, cp, picks, draws, seeds, n_iter, eps, window, freq, precision,
                 schedule="auto"):
        nf = len(picks)
        _FakeHandle.log.append(("sweep", nf, preserve_order, [int(s) for s in seeds]))
        hsum, hcnt = 100.0 + np.arange(nf), np.ones(nf, np.int64)
        its, conv, ec = np.full(nf, 7, np.int32), np.ones(nf, np.int32), np.zeros(nf, np.int32)
        route = np.full(nf, _native.ORDER_DEVICE_GAP, np.int32)
        for f in self.declined:
            route[f], ec[f], hsum[f], hcnt[f], its[f], conv[f] = _native.ORDER_DECLINED, _native.ERR_UNSUPPORTED, 0.0, 0, 0, 0
        return hsum, hcnt, its, conv, ec, 1.5, route

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _FakeHandle.log.append(("close",))
        return False


def _fake_session_sweep(log):
    def sweep(cells, named, preserve_order, nd, k0, cr, cp, picks, draws, seeds, n_iter, eps, window=5, freq=3,
              precision="auto", device=-1, schedule="auto"):
        nf = len(picks)
        log.append(("session", [int(s) for s in seeds], list(nd)))
        return (np.array([float(s % 1000) for s in seeds]), np.ones(nf, np.int64), np.full(nf, 9, np.int32),
                np.zeros(nf, np.int32), np.zeros(nf, np.int32), 0.25)
    return sweep


def test_resident_path_reroutes_the_declined_folds_and_leaves_the_stream_where_session_does(monkeypatch):
    log = []
    monkeypatch.setattr(_native, "PreparedHandle", _FakeHandle)
    monkeypatch.setattr(_native, "cv_sweep_session", _fake_session_sweep(log))
    _FakeHandle.log = []
    _FakeHandle.declined = (1, 4, 5)
    D = _matrix()
    ra, rb = np.random.default_rng(5), np.random.default_rng(5)
    res, secs, n_emb, rerouted = cv.likelihood_sweep(D, SETS, 20, 1e-4, folds=3, rng=ra, path="resident")
    assert rerouted == 3 and n_emb == 6 and secs == 1.75
    assert _FakeHandle.log[0] == ("create", (12, 12), True, True)        # no codes in the data; preserve_order handle
    assert [e[0] for e in _FakeHandle.log] == ["create", "sweep", "close"]
    seeds = _FakeHandle.log[1][3]
    assert log == [("session", [seeds[f] for f in (1, 4, 5)], [2, 3, 3])]   # exactly the declined folds, in fold order
    want = [100.0 + f for f in range(6)]
    for f in (1, 4, 5):
        want[f] = float(seeds[f] % 1000)
    assert res[0]["fold_mae"] == want[:3] and res[1]["fold_mae"] == want[3:]
    assert res[0]["mean_iter"] == (7 + 9 + 7) / 3 and res[1]["mean_iter"] == (7 + 9 + 9) / 3

    log.clear()
    out = cv.likelihood_sweep(D, SETS, 20, 1e-4, folds=3, rng=rb, path="session")
    assert len(out) == 3 and log[0][1] == seeds                          # the same draws ...
    assert ra.bit_generator.state == rb.bit_generator.state              # ... and the stream in the same place

    # nothing declined: the cell list of the library is never asked for
    _FakeHandle.declined = ()
    monkeypatch.setattr(cv.FoldBuilder, "cells", lambda self: pytest.fail("the cell list was built"))
    res2, _, _, rerouted = cv.likelihood_sweep(D, SETS, 20, 1e-4, folds=3, rng=np.random.default_rng(5), path="resident")
    assert rerouted == 0 and res2[0]["fold_mae"] == [100.0, 101.0, 102.0]


def test_an_unknown_path_is_refused_with_the_widened_message():
    with pytest.raises(ValueError, match="'sparse', 'sparse-calls', 'dense', 'session' or 'resident'"):
        cv.likelihood_sweep(_matrix(), SETS, 20, 1e-4, folds=3, rng=np.random.default_rng(1), path="device")
