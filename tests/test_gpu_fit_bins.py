"""The fit's binned diagnostics on the device (run with -m gpu): topolow_layout_prep_fit_extent, _fit_hist2d and
_fit_linear_bins against NumPy on what the device reads -- v, code and held per buffer cell, est from the handle's own
post-metrics pass (fit_bins_helpers.host_view) -- and embedding_quality_data(handle=...) against its host form.

Everything here is EQUAL, not close: the extremes have NumPy's bits, every count is np.histogram2d's, the linear bins'
integers are linear_bin_counts', and the density made from the device's integers has the bits of the one made from the
host's.  Only FitStatistics, which the new entries do not compute, keeps the fit report's band."""
import numpy as np
import pytest

from tests import prepare_layout_helpers as plh
from tests.fit_bins_helpers import axes_of, held_mask, host_view, matrix, picks_of
from tests.resident_helpers import same_bits
from topolow_amd import _native, core, error_metrics as em

pytestmark = pytest.mark.gpu
SERIES = ("in", "out", "all")
AXES = _native.FIT_AXES
PAIRS = (("true", "predicted"), ("true", "residual"), ("predicted", "error"), ("error", "residual"), ("residual", "true"))


def span(x, k):
    """k + 1 edges over the values' range (over [0, 1] where there are none, a width of 1 where it has none)."""
    return em._plot_edges(float(x.min()) if x.size else np.nan, float(x.max()) if x.size else np.nan, k)


def log_edges(x, k):
    """Non-uniform edges: log-spaced steps from below the smallest value to above the largest."""
    lo, hi = (float(x.min()), float(x.max())) if x.size else (0.0, 1.0)
    return lo - 1e-3 + (hi - lo + 2e-3) * (np.logspace(0.0, 2.0, k + 1) - 1.0) / 99.0


def check_hist2d(h, pos, picks, series, ax, xa, xe, ya, ye):
    counts, outside, m = h.fit_hist2d(pos, series, xa, xe, ya, ye, picks)
    want = np.histogram2d(ax[xa], ax[ya], bins=[xe, ye])[0]
    assert counts.dtype == np.int64 and counts.shape == want.shape == (len(xe) - 1, len(ye) - 1)
    assert np.array_equal(counts, want), (series, xa, ya, np.abs(counts - want).sum())
    assert m == ax[xa].size and counts.sum() + outside == m, (series, xa, ya)
    return counts, outside


def check_data_edges(h, pos, picks, series, ax, xa, ya):
    """Edges taken from the data: the first one ulp above the minimum (the minimum is outside), an inner edge equal to
    a cell's value (which falls in the upper bin), the last equal to the maximum (counted, not outside)."""
    x, y = ax[xa], ax[ya]
    distinct = np.unique(x)
    if distinct.size < 4 or np.unique(y).size < 2:
        return False
    inner = distinct[distinct.size // 2]
    xe = np.array([np.nextafter(distinct[0], np.inf), inner, distinct[-1]])
    ye = np.array([y.min(), y.max()])
    counts, outside = check_hist2d(h, pos, picks, series, ax, xa, xe, ya, ye)
    assert outside == int((x == distinct[0]).sum()) > 0
    assert counts[0, 0] == int(((x > distinct[0]) & (x < inner)).sum())
    assert counts[1, 0] == int((x >= inner).sum()) and int((x == inner).sum()) > 0 and int((x == distinct[-1]).sum()) > 0
    return True


# n, ndim, layout, codes, reordered, picks ("none", "some", "all")
CASES = [(2, 1, "C", False, False, "some"), (63, 2, "F", True, True, "some"), (64, 5, "C", True, False, "none"),
         (65, 16, "F", False, True, "all"), (256, 5, "C", True, True, "some"), (257, 2, "F", True, False, "some"),
         (513, 5, "C", True, True, "some")]


@pytest.mark.parametrize("n,ndim,layout,codes,reordered,pick_kind", CASES)
def test_extent_bins_and_linear_bins_equal_the_hosts(n, ndim, layout, codes, reordered, pick_kind):
    values, cds = matrix(n, 100 + n + ndim, codes=codes)
    picks = picks_of(pick_kind, n, n)
    pos = np.random.default_rng(n).normal(size=(n, ndim)) * 1.5
    order = np.random.default_rng(n + 1).permutation(n) if reordered else None
    data_edges_checked = 0
    with _native.PreparedHandle(values, cds, preserve_order=not reordered, order=order, layout=layout) as h:
        assert (h.order is not None) == reordered
        v, est, member = host_view(h, values, cds, picks, pos)
        if pick_kind == "none":
            assert not member["out"].any()
        for series in SERIES:
            ax = axes_of(v, est, member[series])
            m = ax["true"].size
            # -- the extent: NumPy's bits; NaN and 0 for an empty series
            extent, got_m = h.fit_extent(pos, series, picks)
            assert got_m == m and list(extent) == list(AXES)
            for name in AXES:
                if m == 0:
                    assert np.isnan(extent[name]).all()
                else:
                    assert same_bits(np.array(extent[name]), np.array([ax[name].min(), ax[name].max()])), (series, name)
            # -- 2-D counts: 1 x 1, 64 x 64, log-spaced, and edges taken from the data, over all four axes
            for xa, ya in PAIRS:
                x, y = ax[xa], ax[ya]
                one, _ = check_hist2d(h, pos, picks, series, ax, xa, span(x, 1), ya, span(y, 1))
                assert one[0, 0] == m                                       # the last edge is the maximum: counted
                _, outside = check_hist2d(h, pos, picks, series, ax, xa, span(x, 64), ya, span(y, 64))
                assert outside == 0
                check_hist2d(h, pos, picks, series, ax, xa, log_edges(x, 37), ya, log_edges(y, 5))
                # narrower than the data on both axes: cells outside on either side
                inner_x, inner_y = span(x, 9)[2:8], span(y, 7)[1:7]
                _, outside = check_hist2d(h, pos, picks, series, ax, xa, inner_x, ya, inner_y)
                assert outside > 0 or m < 4
                data_edges_checked += check_data_edges(h, pos, picks, series, ax, xa, ya)
            # -- the cap, both ways
            check_hist2d(h, pos, picks, series, ax, "error", span(ax["error"], 8192), "true", span(ax["true"], 1))
            check_hist2d(h, pos, picks, series, ax, "true", span(ax["true"], 1), "residual", span(ax["residual"], 8192))
            # -- linear bins: the host's integers, on every axis and at the smallest and the largest grid
            for name, grid in [(a, 512) for a in AXES] + [("residual", 2), ("residual", 4096), ("error", 3)]:
                x = ax[name]
                lo, up = (float(x.min()) - 0.3, float(x.max()) + 0.7) if m else (0.0, 1.0)
                count, frac, outside, total = h.fit_linear_bins(pos, series, name, lo, up, grid, picks)
                hc, hf, ho = em.linear_bin_counts(x, lo, up, grid)
                assert count.dtype == np.int64 and frac.dtype == np.uint64 and total == m
                assert np.array_equal(count, hc) and np.array_equal(frac, hf) and outside == ho == 0, (series, name, grid)
                if m and np.ptp(x) > 0:   # a grid inside the data: cells outside on both sides
                    lo, up = float(x.min()) + 0.25 * float(np.ptp(x)), float(x.max()) - 0.25 * float(np.ptp(x))
                    count, frac, outside, total = h.fit_linear_bins(pos, series, name, lo, up, grid, picks)
                    hc, hf, ho = em.linear_bin_counts(x, lo, up, grid)
                    assert np.array_equal(count, hc) and np.array_equal(frac, hf) and outside == ho >= 2 and total == m
                    # up is a cell's value: xpos = m - 1 or a rounding below it, and the host decides the same
                    count, frac, outside, total = h.fit_linear_bins(pos, series, name, lo, float(x.max()), grid, picks)
                    hc, hf, ho = em.linear_bin_counts(x, lo, float(x.max()), grid)
                    assert np.array_equal(count, hc) and np.array_equal(frac, hf) and outside == ho and total == m
            # -- density.default's own lo and up: nothing is outside, and the density has the host's bits
            if m >= 2:
                x = ax["residual"]
                host_density = em.density_default(x)
                _, _, lo, up = em.density_grid(float(x.min()), float(x.max()), host_density.bw)
                count, frac, outside, total = h.fit_linear_bins(pos, series, "residual", lo, up, 512, picks)
                assert outside == 0 and total == m and count.sum() == m
                dev_density = em.density_default(binned=(count, frac, lo, up, total), bw=host_density.bw, xmin=x.min(),
                                                 xmax=x.max())
                assert same_bits(dev_density.y, host_density.y) and same_bits(dev_density.x, host_density.x)
        # -- a second call returns the same arrays
        ax = axes_of(v, est, member["all"])
        xe, ye = span(ax["true"], 64), span(ax["error"], 64)
        first, second = (h.fit_hist2d(pos, "all", "true", xe, "error", ye, picks) for _ in range(2))
        assert np.array_equal(first[0], second[0]) and first[1:] == second[1:]
        first, second = (h.fit_linear_bins(pos, "all", "error", ye[0], ye[-1], 512, picks) for _ in range(2))
        assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1]) and first[2:] == second[2:]
        assert h.fit_extent(pos, "all", picks) == h.fit_extent(pos, "all", picks)
    assert data_edges_checked >= (10 if n > 2 else 0)


@pytest.mark.parametrize("layout", ["C", "F"])
def test_an_asymmetric_matrix_with_cells_in_one_triangle(layout):
    n = 65
    values, cds = matrix(n, 9, codes=True, symmetric=False)
    picks = picks_of("some", n, 4)
    pos = np.random.default_rng(2).normal(size=(n, 2))
    with _native.PreparedHandle(values, cds, order=np.random.default_rng(3).permutation(n), layout=layout) as h:
        v, est, member = host_view(h, values, cds, picks, pos)
        assert member["out"].any() and not np.array_equal(np.isnan(v), np.isnan(v.T))
        for series in SERIES:
            ax = axes_of(v, est, member[series])
            check_hist2d(h, pos, picks, series, ax, "true", span(ax["true"], 16), "predicted", span(ax["predicted"], 16))
            x = ax["residual"]
            got = h.fit_linear_bins(pos, series, "residual", x.min() - 1.0, x.max() + 1.0, 512, picks)
            hc, hf, ho = em.linear_bin_counts(x, x.min() - 1.0, x.max() + 1.0, 512)
            assert np.array_equal(got[0], hc) and np.array_equal(got[1], hf) and got[2:] == (ho, x.size)


def test_ties_every_lane_of_every_wave_adds_to_one_counter():
    """A constant matrix with all points at one position: all n^2 errors are identical."""
    n = 257
    values = np.full((n, n), 2.5)
    pos = np.zeros((n, 3))
    with _native.PreparedHandle(values, None, preserve_order=True) as h:
        extent, m = h.fit_extent(pos, "all")
        assert m == n * n and extent == {"true": (2.5, 2.5), "predicted": (0.0, 0.0), "error": (2.5, 2.5),
                                        "residual": (-2.5, -2.5)}
        xe, ye = np.linspace(0.0, 5.0, 65), np.linspace(-4.0, 4.0, 65)
        counts, outside, m = h.fit_hist2d(pos, "all", "error", xe, "residual", ye)
        kx, ky = int(np.searchsorted(xe, 2.5, side="right")) - 1, int(np.searchsorted(ye, -2.5, side="right")) - 1
        assert counts[kx, ky] == n * n == m == counts.sum() and outside == 0
        for name, value in (("error", 2.5), ("residual", -2.5), ("true", 2.5), ("predicted", 0.0)):
            lo, up, grid = -3.0, 3.1, 512
            count, frac, outside, total = h.fit_linear_bins(pos, "all", name, lo, up, grid)
            xpos = (value - lo) / ((up - lo) / (grid - 1))
            ix, q = int(np.floor(xpos)), int((xpos - np.floor(xpos)) * 4294967296.0)
            assert q > 0 and total == n * n and outside == 0
            assert count[ix] == n * n == count.sum() and int(frac[ix]) == n * n * q and np.count_nonzero(frac) == 1
        # every cell outside: nothing but the two totals
        count, frac, outside, total = h.fit_linear_bins(pos, "all", "error", 2.5 + 1e-9, 3.0, 64)
        assert not count.any() and not frac.any() and outside == total == n * n
        counts, outside, m = h.fit_hist2d(pos, "all", "error", np.array([2.5 + 1e-9, 3.0]), "true", np.array([0.0, 5.0]))
        assert not counts.any() and outside == m == n * n


@pytest.mark.parametrize("symmetric", [True, False])
def test_a_needle_one_held_out_pair_in_an_otherwise_empty_series(symmetric):
    n = 257
    values, cds = matrix(n, 21, codes=True, symmetric=symmetric)
    values[40, 200] = 3.25
    cds[40, 200] = cds[200, 40] = 0
    if symmetric:
        values[200, 40] = 3.25
    pick = np.array([40 + 200 * n], dtype=np.int64)              # row 40, column 200; its mirror is held out too
    pos = np.random.default_rng(8).normal(size=(n, 5))
    order = np.random.default_rng(9).permutation(n)
    with _native.PreparedHandle(values, cds, order=order) as h:
        qa, qb = int(np.flatnonzero(order == 40)[0]), int(np.flatnonzero(order == 200)[0])
        est, _, _ = h.post_metrics(pos)
        r, want = est[qa, qb], 2 if symmetric else 1
        assert est[qb, qa] == r
        extent, m = h.fit_extent(pos, "out", pick)
        assert m == want and extent["true"] == (3.25, 3.25) and extent["error"] == (3.25 - r, 3.25 - r)
        xe, ye = np.linspace(0.0, 8.0, 65), np.linspace(-8.0, 8.0, 129)
        counts, outside, m = h.fit_hist2d(pos, "out", "true", xe, "residual", ye, pick)
        kx, ky = int(np.searchsorted(xe, 3.25, side="right")) - 1, int(np.searchsorted(ye, r - 3.25, side="right")) - 1
        assert counts[kx, ky] == want == counts.sum() == m and outside == 0
        count, frac, outside, total = h.fit_linear_bins(pos, "out", "residual", -8.0, 8.0, 4096, pick)
        xpos = ((r - 3.25) + 8.0) / (16.0 / 4095)
        ix = int(np.floor(xpos))
        assert count[ix] == want == count.sum() == total and outside == 0
        assert int(frac[ix]) == want * int((xpos - ix) * 4294967296.0) and np.count_nonzero(frac) <= 1
        assert h.fit_extent(pos, "out")[1] == 0                  # no picks: the series is empty again


def test_refused_calls_leave_the_handle_as_it_was():
    n = 65
    values, cds = matrix(n, 33, codes=True, special=False)
    pos = np.random.default_rng(1).normal(size=(n, 2))
    picks = picks_of("some", n, 2)
    edges = np.linspace(-9.0, 9.0, 9)
    with _native.PreparedHandle(values, cds, preserve_order=True) as h:
        fold_before = h.fold(picks, True, True)
        rep_before = h.fit_report(pos, picks)
        bins_before = h.fit_hist2d(pos, "out", "true", edges, "error", edges, picks)

        def unchanged():
            rep_after = h.fit_report(pos, picks)
            assert all(rep_after[name] == rep_before[name] for name in SERIES)
            empty = h.fold(np.zeros(0, dtype=np.int64), True, True)      # nothing is marked: the mask is empty
            assert empty[4][0].size == 0 and empty[5][0].size == 0
            fold_after = h.fold(picks, True, True)
            assert same_bits(fold_after[1], fold_before[1]) and fold_after[2:4] == fold_before[2:4]
            assert h.fit_extent(pos, "out")[1] == 0                      # no picks, nobody held out
            bins_after = h.fit_hist2d(pos, "out", "true", edges, "error", edges, picks)
            assert np.array_equal(bins_after[0], bins_before[0]) and bins_after[1:] == bins_before[1:]

        unchanged()
        for bad_picks in (np.array([3, n * n], dtype=np.int64), np.array([-1], dtype=np.int64)):
            for call in (lambda: h.fit_extent(pos, "all", bad_picks),
                         lambda: h.fit_hist2d(pos, "all", "true", edges, "error", edges, bad_picks),
                         lambda: h.fit_linear_bins(pos, "all", "error", -1.0, 1.0, 512, bad_picks)):
                with pytest.raises(_native.NativeError, match="lie outside the matrix") as exc:
                    call()
                assert exc.value.code == _native.ERR_BAD_ARGUMENT
            unchanged()
        for call, word in ((lambda: h.fit_hist2d(pos, "all", "true", np.arange(130.0), "error", np.arange(65.0), picks), "nx \\* ny <= 8192"),
                           (lambda: h.fit_hist2d(pos, "all", "true", np.array([0.0, 1.0, 1.0]), "error", edges, picks), "strictly increasing"),
                           (lambda: h.fit_linear_bins(pos, "all", "error", -1.0, 1.0, 4097, picks), "2 <= m <= 4096"),
                           (lambda: h.fit_linear_bins(pos, "all", "error", 1.0, 1.0, 512, picks), "lo < up")):
            with pytest.raises(_native.NativeError, match=word) as exc:
                call()
            assert exc.value.code == _native.ERR_BAD_ARGUMENT
        unchanged()
    with _native.PreparedHandle(plh.one_negative()) as declined:
        assert declined.declined
        for call in (lambda: declined.fit_extent(np.zeros((33, 2)), "all"),
                     lambda: declined.fit_hist2d(np.zeros((33, 2)), "all", "true", edges, "error", edges),
                     lambda: declined.fit_linear_bins(np.zeros((33, 2)), "all", "error", -1.0, 1.0)):
            with pytest.raises(_native.NativeError, match="declined") as exc:
                call()
            assert exc.value.code == _native.ERR_BAD_ARGUMENT


@pytest.mark.parametrize("layout,reordered,pick_kind,series", [("C", False, "some", "all"), ("F", True, "some", "out"),
                                                               ("C", True, "none", "in")])
def test_embedding_quality_data_device_form_equals_the_host_form(layout, reordered, pick_kind, series):
    from tests.test_gpu_fit_report import fields_agree, intercept_scale
    n = 257
    values, cds = matrix(n, 77, codes=True, special=False)
    picks = picks_of(pick_kind, n, 12)
    # the points the matrix was drawn around (matrix()'s first draw), disturbed: a fit, not noise
    pos = np.random.default_rng(77).normal(size=(n, 3)) + 0.1 * np.random.default_rng(4).normal(size=(n, 3))
    order = np.random.default_rng(6).permutation(n) if reordered else None
    if order is not None:
        pos = pos[order]
    with _native.PreparedHandle(values, cds, preserve_order=not reordered, order=order, layout=layout) as h:
        dev = em.embedding_quality_data(handle=h, positions=pos, holdout=picks, series=series, bins=(48, 40))
        est, _, _ = h.post_metrics(pos)
    # the host form works in the ordered numbering, as the positions do
    held = held_mask(n, picks)
    truth = core.CodedMatrix(values, cds)
    if order is not None:
        truth, held = truth.reordered(order), held[np.ix_(order, order)]
    host = em.embedding_quality_data(truth, est, holdout=np.flatnonzero(held.ravel(order="F")), series=series, bins=(48, 40))
    assert dev.n == host.n > 1000 and dev.series == host.series == series
    for a, b in ((dev.scatter, host.scatter), (dev.residual_vs_true, host.residual_vs_true),
                 (dev.residual_vs_fitted, host.residual_vs_fitted)):
        assert (a.x_axis, a.y_axis) == (b.x_axis, b.y_axis)
        assert same_bits(a.x_edges, b.x_edges) and same_bits(a.y_edges, b.y_edges)
        assert a.counts.shape == (48, 40) and np.array_equal(a.counts, b.counts) and a.counts.dtype == b.counts.dtype
        assert a.outside == b.outside == 0 and a.n == b.n == a.counts.sum()
        assert np.array_equal(a.conditional_quantiles((0.25, 0.5, 0.75)), b.conditional_quantiles((0.25, 0.5, 0.75)),
                              equal_nan=True)
    assert dev.residual_density.bw == host.residual_density.bw and dev.residual_density.n == host.residual_density.n
    assert same_bits(dev.residual_density.x, host.residual_density.x)
    assert same_bits(dev.residual_density.y, host.residual_density.y)
    fields_agree(dev.statistics, host.statistics, intercept_scale(truth.values, est, host.statistics.slope))
