"""The fit report of a resident embedding on the device (run with -m gpu): topolow_layout_prep_fit_report and
_fit_order_stats against the host's own arithmetic on the distances `handle.post_metrics` returns, and
fit_statistics(handle=...) against its host form, the specification.

Exact: every count, min and max, every order statistic (bit for bit against np.sort of the host's v - est), and a
second call.  Sums: each device sum against math.fsum of the host's terms within 1e-12 * sum |term|.  Where that band
comes from: the terms have the host's bits (the same IEEE subtraction, division and product of the same operands); the
reduction adds at most n + ceil(n / 256) + 16 times, each add within 2^-53 relative of a partial sum that is at most
sum |term|, which at n <= 513 is < 6e-14 of sum |term|.  The centred sums get the same band: a mean that is off by
delta changes them by m delta^2, far below it."""
import math

import numpy as np
import pytest

from tests import prepare_layout_helpers as plh
from tests.resident_helpers import same_bits, start_positions
from topolow_amd import _native, core, cv, error_metrics as em

pytestmark = pytest.mark.gpu
BAND = 1e-12


def matrix(n, seed, codes=True, symmetric=True, special=True):
    """values (NaN = NA; a few +-Inf cells, zeros on the diagonal) and codes (or None) of a noisy distance matrix."""
    rng = np.random.default_rng(seed)
    pts = rng.normal(size=(n, 3))
    d = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1)) * (1.0 + 0.3 * rng.normal(size=(n, n)))
    d = np.abs(np.triu(d, 1))
    d = d + d.T
    hole = np.triu(rng.random((n, n)) < 0.4, 1)
    d[hole | hole.T] = np.nan
    cds = None
    if codes:
        u = np.triu(rng.random((n, n)), 1)
        u = u + u.T
        cds = np.zeros((n, n), dtype=np.int8)
        cds[(u > 0) & (u < 0.10)] = 1
        cds[(u >= 0.10) & (u < 0.15)] = -1
    if special and n >= 8:
        d[1, 3] = d[3, 1] = np.inf
        d[2, 6] = d[6, 2] = -np.inf
        d[4, 4] = np.nan
        d[5, 5] = 1.25
    if not symmetric:
        d[np.tril_indices(n, -1)] = np.nan        # cells in one triangle only
    return d, cds


def held_mask(n, picks):
    held = np.zeros((n, n), dtype=bool)
    if picks is not None and len(picks):
        p = np.asarray(picks, dtype=np.int64)
        held[p % n, p // n] = True
        held |= held.T
    return held


def host_view(h, values, codes, picks, pos):
    """What the device reads, in BUFFER coordinates: v, code, held per cell (a, b) of the ordered matrix as the handle's
    lines hold it, and est from the handle's own post-metrics pass."""
    n = h.n
    cds = np.zeros((n, n), dtype=np.int8) if codes is None else codes
    held = held_mask(n, picks)
    o = h.order
    if o is not None:
        ix = np.ix_(o, o)
        values, cds, held = values[ix], cds[ix], held[ix]
    if h.layout == "F":                              # a line is a column
        values, cds = values.T, cds.T
    est, _, _ = h.post_metrics(pos)
    fin = np.isfinite(values)
    member = {"in": fin & (cds == 0) & ~held, "out": fin & (cds == 0) & held, "all": fin}
    return values, est, member


def fsum_close(got, terms, what):
    terms = np.asarray(terms, dtype=np.float64).ravel()
    want, scale = math.fsum(terms), math.fsum(np.abs(terms))
    assert abs(got - want) <= BAND * scale, (what, got, want, scale)


def check_report(rep, v, est, member):
    e = v - est
    for name, mask in member.items():
        s, x, vv, rr = rep[name], e[mask], v[mask], est[mask]
        m = int(mask.sum())
        assert s["count"] == m, name
        if m == 0:
            assert math.isnan(s["min_e"]) and math.isnan(s["max_e"]) and s["sum_e"] == 0.0 and s["css_e"] == 0.0
            continue
        assert same_bits(np.float64(s["min_e"]), x.min()) and same_bits(np.float64(s["max_e"]), x.max()), name
        fsum_close(s["sum_e"], x, name + " sum_e")
        fsum_close(s["sum_abs_e"], np.abs(x), name + " sum_abs_e")
        mean = math.fsum(x) / m
        fsum_close(s["css_e"], (x - mean) ** 2, name + " css_e")
        if name == "all":
            assert s["pct_count"] == 0 and s["sum_pct"] == 0.0
            fsum_close(s["sum_v"], vv, "sum_v")
            fsum_close(s["sum_r"], rr, "sum_r")
            dv, dr = vv - math.fsum(vv) / m, rr - math.fsum(rr) / m
            fsum_close(s["css_v"], dv * dv, "css_v")
            fsum_close(s["css_r"], dr * dr, "css_r")
            fsum_close(s["css_vr"], dv * dr, "css_vr")
        else:
            pos = vv > 0
            p = x[pos] / vv[pos] * 100.0
            assert s["pct_count"] == int(pos.sum()), name
            fsum_close(s["sum_pct"], p, name + " sum_pct")
            fsum_close(s["sum_abs_pct"], np.abs(p), name + " sum_abs_pct")
            assert s["sum_v"] == 0.0 and s["css_vr"] == 0.0


def check_order_stats(h, pos, picks, rep, v, est, member):
    e = v - est
    for name, mask in member.items():
        x = np.sort(e[mask])
        m = x.size
        if m == 0:
            vals, got_m = h.fit_order_stats(pos, name, [0, 5], picks)
            assert got_m == 0 and np.isnan(vals).all()
            continue
        ranks = sorted({0, m - 1, m // 2, (m - 1) // 4, (3 * (m - 1)) // 4, min(1, m - 1), max(m - 2, 0)})
        ranks = ranks + [ranks[0]]                   # a rank asked for twice
        vals, got_m = h.fit_order_stats(pos, name, ranks, picks)
        assert got_m == m and same_bits(vals, x[ranks]), (name, vals, x[ranks])
        assert same_bits(vals[0], np.float64(rep[name]["min_e"])) and same_bits(vals[len(ranks) - 2], np.float64(rep[name]["max_e"]))


# n, ndim, layout, codes, reordered, picks ("none", "some", "all")
CASES = [(2, 1, "C", False, False, "some"), (63, 2, "F", True, True, "some"), (64, 5, "C", True, False, "none"),
         (65, 16, "F", False, True, "all"), (256, 5, "C", True, True, "some"), (257, 2, "F", True, False, "some"),
         (513, 5, "C", True, True, "some"), (513, 1, "F", False, False, "all")]


def picks_of(kind, n, seed):
    if kind == "none":
        return None
    if kind == "all":
        return np.arange(n * n, dtype=np.int64)
    return np.random.default_rng(seed).choice(n * n, max(1, n * n // 10), replace=False).astype(np.int64)


@pytest.mark.parametrize("n,ndim,layout,codes,reordered,pick_kind", CASES)
def test_report_and_order_statistics_against_the_host(n, ndim, layout, codes, reordered, pick_kind):
    values, cds = matrix(n, 100 + n + ndim, codes=codes)
    picks = picks_of(pick_kind, n, n)
    pos = np.random.default_rng(n).normal(size=(n, ndim)) * 1.5
    order = np.random.default_rng(n + 1).permutation(n) if reordered else None
    with _native.PreparedHandle(values, cds, preserve_order=not reordered, order=order, layout=layout) as h:
        assert (h.order is not None) == reordered
        v, est, member = host_view(h, values, cds, picks, pos)
        if pick_kind == "some" and n > 2:
            assert member["in"].any() and member["out"].any()
            assert (v - est)[member["in"]].min() < 0 < (v - est)[member["in"]].max()      # negative, zero, positive
            assert ((v - est)[member["in"]] == 0).any()
        if pick_kind == "all":
            assert not member["in"].any()
        rep = h.fit_report(pos, picks)
        check_report(rep, v, est, member)
        check_order_stats(h, pos, picks, rep, v, est, member)
        again = h.fit_report(pos, picks)             # the same bits on a second call
        for name in ("in", "out", "all"):
            assert again[name] == rep[name] or all(
                same_bits(np.float64(again[name][k]), np.float64(rep[name][k])) for k in rep[name])
        assert len(rep["seconds"]) == 3 and rep["seconds"][2] >= rep["seconds"][0] >= 0


@pytest.mark.parametrize("layout", ["C", "F"])
def test_an_asymmetric_matrix_with_cells_in_one_triangle(layout):
    n = 65
    values, cds = matrix(n, 9, codes=True, symmetric=False)
    picks = picks_of("some", n, 4)
    pos = np.random.default_rng(2).normal(size=(n, 2))
    with _native.PreparedHandle(values, cds, order=np.random.default_rng(3).permutation(n), layout=layout) as h:
        v, est, member = host_view(h, values, cds, picks, pos)
        assert member["out"].any() and not np.array_equal(np.isnan(v), np.isnan(v.T))
        rep = h.fit_report(pos, picks)
        check_report(rep, v, est, member)
        check_order_stats(h, pos, picks, rep, v, est, member)


def test_massive_ties_and_negative_ranks():
    """All positions zero, values drawn from three numbers: every error is one of three values (and 0 on the diagonal)."""
    n = 257
    rng = np.random.default_rng(5)
    values = rng.choice([1.0, 2.0, 3.5], size=(n, n))
    values = np.triu(values, 1) + np.triu(values, 1).T
    pos = np.zeros((n, 3))
    picks = picks_of("some", n, 6)
    with _native.PreparedHandle(values, None, preserve_order=True) as h:
        v, est, member = host_view(h, values, None, picks, pos)
        assert not est.any()
        rep = h.fit_report(pos, picks)
        check_report(rep, v, est, member)
        check_order_stats(h, pos, picks, rep, v, est, member)
        x = np.sort((v - est)[member["out"]])
        m = x.size
        up = _native.FIT_RANK_UPPER
        asked = [-1, -1 - 250000, -1 - (250000 + up), -1 - 500000, -1 - (500000 + up), -1 - 1000000, -1 - (1000000 + up)]
        want = [0, (m - 1) // 4, -((-(m - 1)) // 4), (m - 1) // 2, -((-(m - 1)) // 2), m - 1, m - 1]
        vals, got_m = h.fit_order_stats(pos, "out", asked, picks)
        assert got_m == m and same_bits(vals, x[want])


def test_a_needle_one_held_out_cell_in_n_squared():
    n = 513
    values, cds = matrix(n, 21, codes=True)
    values[400, 400] = 2.75
    pick = np.array([400 + 400 * n], dtype=np.int64)       # a diagonal cell: its mirror is itself
    pos = np.random.default_rng(8).normal(size=(n, 5))
    order = np.random.default_rng(9).permutation(n)
    with _native.PreparedHandle(values, cds, order=order) as h:
        q = int(np.flatnonzero(order == 400)[0])
        est, _, _ = h.post_metrics(pos)
        rep = h.fit_report(pos, pick)
        assert rep["out"]["count"] == 1 and rep["out"]["min_e"] == rep["out"]["max_e"] == 2.75 - est[q, q] == 2.75
        assert rep["out"]["sum_e"] == 2.75 and rep["out"]["css_e"] == 0.0 and rep["out"]["sum_pct"] == 100.0
        vals, m = h.fit_order_stats(pos, "out", [0], pick)
        assert m == 1 and vals[0] == 2.75
        none = h.fit_report(pos)
        assert none["in"]["count"] == rep["in"]["count"] + 1 and none["all"] == {**rep["all"]}


def test_errors_leave_the_handle_as_it_was():
    n = 65
    values, cds = matrix(n, 33, codes=True, special=False)
    pos = np.random.default_rng(1).normal(size=(n, 2))
    picks = picks_of("some", n, 2)
    with _native.PreparedHandle(values, cds, preserve_order=True) as h:
        fold_before = h.fold(picks, True, True)
        post_before = h.post_metrics(pos)
        rep_before = h.fit_report(pos, picks)

        def unchanged():
            fold_after, post_after = h.fold(picks, True, True), h.post_metrics(pos)
            assert same_bits(post_after[0], post_before[0]) and post_after[1:] == post_before[1:]
            assert fold_after[0] is None and same_bits(fold_after[1], fold_before[1]) and fold_after[2:4] == fold_before[2:4]
            for got, want in zip(fold_after[4] + fold_after[5], fold_before[4] + fold_before[5]):
                assert same_bits(got, want)
            empty = h.fold(np.zeros(0, dtype=np.int64), True, True)      # nothing is marked: the mask is empty
            assert empty[4][0].size == 0 and empty[5][0].size == 0
            rep_after = h.fit_report(pos, picks)
            assert all(rep_after[name] == rep_before[name] for name in ("in", "out", "all"))

        unchanged()
        m_in = rep_before["in"]["count"]
        for bad_picks in (np.array([3, n * n], dtype=np.int64), np.array([-1], dtype=np.int64)):
            with pytest.raises(_native.NativeError, match="lie outside the matrix") as exc:
                h.fit_report(pos, bad_picks)
            assert exc.value.code == _native.ERR_BAD_ARGUMENT
            with pytest.raises(_native.NativeError, match="lie outside the matrix"):
                h.fit_order_stats(pos, "all", [0], bad_picks)
            unchanged()
        with pytest.raises(_native.NativeError, match="not below the series' count %d" % m_in) as exc:
            h.fit_order_stats(pos, "in", [0, m_in], picks)
        assert exc.value.code == _native.ERR_BAD_ARGUMENT
        unchanged()
        vals, m = h.fit_order_stats(pos, "out", [0, 1, 2])                  # no picks: OUT is empty
        assert m == 0 and vals.shape == (3,) and np.isnan(vals).all()
        unchanged()
    with _native.PreparedHandle(plh.one_negative()) as declined:
        assert declined.declined
        for call in (lambda: declined.fit_report(np.zeros((33, 2))),
                     lambda: declined.fit_order_stats(np.zeros((33, 2)), "all", [0])):
            with pytest.raises(_native.NativeError, match="declined") as exc:
                call()
            assert exc.value.code == _native.ERR_BAD_ARGUMENT


def fields_agree(dev, host, intercept_scale):
    """Quantiles, min and max exact; the rest within the band of its sums.  Pearson's r, the slope and the interval are
    quotients of sums whose band is relative to sum |term|: the callers' predictions are correlated with the truth
    (r > 0.5), so sum |dv dr| <= sqrt(css_v css_r) < 2 |css_vr| and the band carries over with a small factor.
    intercept_scale: mean |r| + |slope| mean |v| over ALL, what the intercept's two terms are bounded by."""
    for a, b in ((dev.in_sample, host.in_sample), (dev.out_sample, host.out_sample)):
        assert a.n == b.n
        if a.n == 0:
            continue
        assert same_bits(np.float64(a.min), np.float64(b.min)) and same_bits(np.float64(a.max), np.float64(b.max))
        assert same_bits(a.quantiles, b.quantiles) and same_bits(np.float64(a.median), np.float64(b.median))
        assert a.mae == pytest.approx(b.mae, rel=BAND) and a.sd == pytest.approx(b.sd, rel=BAND)
        assert abs(a.mean - b.mean) <= BAND * b.mae
        # the percentage terms are bounded by their own absolute mean
        assert abs(a.mean_percentage_error - b.mean_percentage_error) <= BAND * b.mean_abs_percentage_error
        assert a.mean_abs_percentage_error == pytest.approx(b.mean_abs_percentage_error, rel=BAND)
    assert dev.n == host.n and dev.Completeness == host.Completeness and dev.probs == host.probs
    assert host.pearson_r > 0.5
    for k in ("mae", "pearson_r", "slope", "residual_sd", "prediction_interval"):
        assert getattr(dev, k) == pytest.approx(getattr(host, k), rel=4 * BAND), k
    assert abs(dev.intercept - host.intercept) <= 8 * BAND * intercept_scale


def intercept_scale(values, est, slope):
    fin = np.isfinite(values)
    return float(np.abs(est[fin]).mean() + abs(slope) * np.abs(values[fin]).mean())


@pytest.mark.parametrize("layout,reordered,pick_kind", [("C", False, "some"), ("F", True, "some"), ("C", True, "none")])
def test_fit_statistics_device_form_equals_the_host_form(layout, reordered, pick_kind):
    n = 257
    values, cds = matrix(n, 77, codes=True, special=False)
    values[5, 5] = 0.0
    picks = picks_of(pick_kind, n, 12)
    # the points the matrix was drawn around (matrix()'s first draw), disturbed: a fit, not noise
    pos = np.random.default_rng(77).normal(size=(n, 3)) + 0.1 * np.random.default_rng(4).normal(size=(n, 3))
    order = np.random.default_rng(6).permutation(n) if reordered else None
    if order is not None:
        pos = pos[order]
    probs = (0.1, 0.25, 0.5, 0.75)
    with _native.PreparedHandle(values, cds, preserve_order=not reordered, order=order, layout=layout) as h:
        dev = em.fit_statistics(None, handle=h, positions=pos, holdout=picks, probs=probs)
        est, _, _ = h.post_metrics(pos)
        with pytest.raises(ValueError, match="at most 8 ranks"):
            em.fit_statistics(None, handle=h, positions=pos, holdout=picks, probs=(0.0513, 0.1531, 0.3077, 0.4519, 0.6031, 0.8077))
    # the host form works in the ordered numbering, as the positions do
    held = held_mask(n, picks)
    truth = core.CodedMatrix(values, cds)
    if order is not None:
        truth, held = truth.reordered(order), held[np.ix_(order, order)]
    host = em.fit_statistics(truth, est, holdout=np.flatnonzero(held.ravel(order="F")), probs=probs)
    fields_agree(dev, host, intercept_scale(truth.values, est, host.slope))
    assert dev.seconds is not None and host.seconds is None
    assert (dev.out_sample.n > 0) == (pick_kind == "some")


def test_the_notebooks_summary_on_the_h3n2_panel():
    """One embedding of the H3N2 panel at the reference's best parameters with one fold of cv.make_folds held out: the
    summary the reference's notebook makes of the signed out-of-sample errors (mean, sd, median, Q1, Q3;
    methods-comparison-h3n2-hiv-denv.Rmd:2339-2349) from the handle equals the host form's on the same positions.  This
    pins that the summary is the one we compute; the statistical bands against the reference's file stay in
    tests/test_gpu_reference_results.py."""
    from tests import parity_problems as pp
    from tests.test_gpu_reference_results import best_params
    m = core.coded_matrix(pp.h3n2_matrix())
    params = best_params("H3N2")
    n = m.values.shape[0]
    fold = cv.make_folds(m.values, 20, np.random.default_rng(8))[0]
    masked = m.masked(fold % n, fold // n)
    with _native.PreparedHandle(masked.values, masked.codes, preserve_order=True) as train:
        res = train.optimize(start_positions(n, int(params["N"]), 3), n_iter=500, k0=params["k0"],
                             cooling_rate=params["cooling_rate"], c_repulsion=params["c_repulsion"],
                             relative_epsilon=1e-10, convergence_window=3, seed=900)
    with _native.PreparedHandle(m.values, m.codes, preserve_order=True) as h:
        dev = em.fit_statistics(None, handle=h, positions=res.positions, holdout=fold)
        est, _, _ = h.post_metrics(res.positions)
    host = em.fit_statistics(m, est, holdout=fold)
    oe = em.error_calculator_comparison(est, m, masked)["OutSampleError"]
    oe = oe[np.isfinite(oe)]
    assert dev.out_sample.n == host.out_sample.n == oe.size > 100
    assert same_bits(dev.out_sample.quantiles, host.out_sample.quantiles)
    assert dev.out_sample.median == host.out_sample.median == dev.out_sample.quantiles[1]
    assert dev.out_sample.quantiles[0] == pytest.approx(np.quantile(oe, 0.25), rel=1e-13)
    assert dev.out_sample.quantiles[2] == pytest.approx(np.quantile(oe, 0.75), rel=1e-13)
    assert dev.out_sample.median == pytest.approx(np.median(oe), rel=1e-13)
    assert abs(dev.out_sample.mean - host.out_sample.mean) <= BAND * host.out_sample.mae
    assert host.out_sample.mean == pytest.approx(oe.mean(), abs=1e-13 * host.out_sample.mae)
    assert dev.out_sample.sd == pytest.approx(host.out_sample.sd, rel=BAND)
    assert host.out_sample.sd == pytest.approx(oe.std(ddof=1), rel=1e-13)
    fields_agree(dev, host, intercept_scale(m.values, est, host.slope))
