"""The host side of the fit's binned diagnostics (no device): bw_nrd0, density_default, the quantised linear binning,
BinnedCloud.conditional_quantiles and the host form of embedding_quality_data, which is the specification of the
device form (tests/test_gpu_fit_bins.py)."""
import math

import numpy as np
import pytest

from tests import parity_problems as pp
from topolow_amd import core, error_metrics as em


def test_bw_nrd0_by_hand_and_its_fall_backs():
    # 0.9 * min(sd, IQR / 1.34) * n^(-1/5); 32^(-1/5) = 1/2
    assert em.bw_nrd0(2.0, 1.34, 32) == pytest.approx(0.9 * 1.0 * 0.5, rel=1e-15)      # the IQR decides
    assert em.bw_nrd0(0.5, 1.34, 32) == pytest.approx(0.9 * 0.5 * 0.5, rel=1e-15)      # the sd decides
    assert em.bw_nrd0(3.0, 2.68, 100000) == pytest.approx(0.9 * 2.0 * 0.1, rel=1e-15)  # 10^5^(-1/5) = 1/10
    # more than half of the values tied: IQR = 0, so the sd
    assert em.bw_nrd0(2.0, 0.0, 32) == pytest.approx(0.9 * 2.0 * 0.5, rel=1e-15)
    # all values equal: sd = IQR = 0, so |x[1]|; and 1 where that is 0 as well
    assert em.bw_nrd0(0.0, 0.0, 32, first=-4.0) == pytest.approx(0.9 * 4.0 * 0.5, rel=1e-15)
    assert em.bw_nrd0(0.0, 0.0, 32) == pytest.approx(0.9 * 1.0 * 0.5, rel=1e-15)
    with pytest.raises(ValueError, match="at least 2"):
        em.bw_nrd0(1.0, 1.0, 1)
    x = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0])                        # quartiles (type 7): 2.5 and 14, sd 11.86...
    want = 0.9 * min(x.std(ddof=1), (14.0 - 2.5) / 1.34) * 6 ** -0.2
    assert em.density_default(x).bw == pytest.approx(want, rel=1e-15)


def _normal():
    return np.random.default_rng(1).normal(0.3, 1.7, size=2000)


def _bimodal():
    rng = np.random.default_rng(2)
    return np.concatenate([rng.normal(-2.0, 0.5, size=1200), rng.normal(3.0, 1.0, size=800)])


def _heavy_ties():
    rng = np.random.default_rng(3)          # a quarter of the values are one number, the rest lie on a grid of 0.25
    return np.concatenate([np.full(500, 1.5), np.round(rng.normal(0.0, 2.0, size=1500) * 4.0) / 4.0])


SAMPLES = {"normal": _normal, "bimodal": _bimodal, "heavy ties": _heavy_ties}

# |density_default - direct Gaussian sum| at density_default's 512 points, relative to the direct sum's peak, and the
# trapezoid integral minus 1, measured on this code (binning on 512 grid points over [lo, up], FFT, interpolation):
#   normal      2000 values   bw 0.33686    1.054e-03    integral - 1 = 9.771e-04
#   bimodal     2000 values   bw 0.498998   7.076e-04    integral - 1 = 9.743e-04
#   heavy ties  2000 values   bw 0.330456   1.547e-03    integral - 1 = 9.748e-04
# The integral's excess is density.default's own: its kernel ordinates are spaced 2 (up - lo) / (2 n - 1), its grid
# (up - lo) / (n - 1), so the kernel is 1 / (2 n - 1) = 1 / 1023 too wide in the grid's units.
# The band is twice the largest value seen.
DENSITY_BAND = 2 * 1.547e-03


def direct_density(x, at, bw):
    """(1 / (N bw)) sum phi((at - x_i) / bw)"""
    z = (at[:, None] - x[None, :]) / bw
    return np.exp(-0.5 * z * z).sum(axis=1) / (x.size * bw * math.sqrt(2.0 * math.pi))


@pytest.mark.parametrize("name", list(SAMPLES))
def test_density_default_against_the_direct_gaussian_sum(name):
    x = SAMPLES[name]()
    assert x.size <= 2000
    d = em.density_default(x)
    assert d.x.shape == d.y.shape == (512,) and d.n == x.size
    assert d.x[0] == x.min() - 3 * d.bw and d.x[-1] == x.max() + 3 * d.bw
    ref = direct_density(x, d.x, d.bw)
    worst = np.abs(d.y - ref).max() / ref.max()
    integral = float(np.sum(0.5 * (d.y[1:] + d.y[:-1]) * np.diff(d.x)))
    print(name, "bw", d.bw, "worst", worst, "integral - 1", integral - 1.0)
    assert worst <= DENSITY_BAND
    assert abs(integral - 1.0) <= DENSITY_BAND
    # the binned form from the host's own bins is the raw form, bit for bit
    from_, to, lo, up = em.density_grid(float(x.min()), float(x.max()), d.bw)
    count, frac, outside = em.linear_bin_counts(x, lo, up, 512)
    assert outside == 0 and count.sum() == x.size and count[511] == 0 and frac[511] == 0
    again = em.density_default(binned=(count, frac, lo, up, x.size), bw=d.bw, xmin=x.min(), xmax=x.max())
    assert np.array_equal(again.y, d.y) and np.array_equal(again.x, d.x)
    with pytest.raises(ValueError, match="density_grid"):
        em.density_default(binned=(count, frac, lo, up + 1.0, x.size), bw=d.bw, xmin=x.min(), xmax=x.max())


def bindist_masses(x, lo, up, m):
    """R's BinDist with unit weights, unquantised, in its own order of operations."""
    y = np.zeros(m)
    delta = (up - lo) / (m - 1)
    for xi in x:
        xpos = (xi - lo) / delta
        ix = math.floor(xpos)
        fx = xpos - ix
        if 0 <= ix <= m - 2:
            y[ix] += 1.0 - fx
            y[ix + 1] += fx
        elif ix == -1:
            y[0] += fx
        elif ix == m - 1:
            y[ix] += 1.0 - fx
    return y


@pytest.mark.parametrize("name", list(SAMPLES))
def test_quantised_masses_against_bindist(name):
    x = SAMPLES[name]()
    bw = em.density_default(x).bw
    _, _, lo, up = em.density_grid(float(x.min()), float(x.max()), bw)
    for m in (2, 64, 512):
        count, frac, outside = em.linear_bin_counts(x, lo, up, m)
        assert outside == 0 and count.dtype == np.int64 and frac.dtype == np.uint64
        mass = em.linear_bin_masses(count, frac)
        assert np.abs(mass - bindist_masses(x, lo, up, m)).max() <= 2.0 ** -32 * x.size
        assert mass.sum() == pytest.approx(x.size, rel=1e-12)
    # values outside [lo, up) of the grid are counted as such, the upper end included
    count, frac, outside = em.linear_bin_counts(np.array([-0.5, 0.0, 0.25, 1.0, 1.5, 0.999]), 0.0, 1.0, 3)
    assert outside == 3 and count.tolist() == [2, 1, 0] and frac.tolist() == [2 ** 31, int(0.998 * 2 ** 32), 0]


def test_the_fraction_sums_are_exact_integers():
    rng = np.random.default_rng(4)
    x = rng.random(5000)
    count, frac, _ = em.linear_bin_counts(x, 0.0, 1.0, 5)
    xpos = x / 0.25
    for g in range(4):
        sel = np.floor(xpos) == g
        assert count[g] == int(sel.sum())
        assert int(frac[g]) == sum(int((p - g) * 4294967296.0) for p in xpos[sel])


def test_conditional_quantiles_on_a_hand_made_table():
    counts = np.array([[0, 4, 0, 4], [0, 0, 0, 0], [2, 0, 0, 0], [1, 1, 1, 1]], dtype=np.int64)
    cloud = em.BinnedCloud("true", "predicted", np.arange(5.0), np.array([0.0, 1.0, 2.0, 4.0, 8.0]), counts, 0, 15)
    q = cloud.conditional_quantiles((0.0, 0.25, 0.5, 0.75, 1.0))
    assert q.shape == (5, 4)
    # x-bin 0: 4 points in [1, 2), 4 in [4, 8): the cumulative count reaches 2 half-way through [1, 2), 4 at its end
    assert q[:, 0].tolist() == [1.0, 1.5, 2.0, 6.0, 8.0]
    assert np.isnan(q[:, 1]).all()                                          # an empty x-bin
    assert q[:, 2].tolist() == [0.0, 0.25, 0.5, 0.75, 1.0]                  # one y-bin: linear inside it
    assert q[:, 3].tolist() == [0.0, 1.0, 2.0, 4.0, 8.0]
    assert np.array_equal(cloud.conditional_quantiles()[0], q[2], equal_nan=True)
    with pytest.raises(ValueError, match="probs"):
        cloud.conditional_quantiles((1.5,))
    assert "loess" in em.BinnedCloud.conditional_quantiles.__doc__ and "DEVIATION" in em.BinnedCloud.conditional_quantiles.__doc__


def test_bin_counts_2d_is_histogram2d_on_the_edge_cases():
    x = np.array([0.0, 1.0, 1.0, 2.0, 3.0, 3.0000000000000004, -1e-300, 2.5])
    y = np.array([5.0, 5.0, 6.0, 7.0, 7.0, 5.0, 5.0, 4.999])
    xe, ye = np.array([0.0, 1.0, 3.0]), np.array([5.0, 6.0, 7.0])
    counts, outside = em.bin_counts_2d(x, y, xe, ye)
    want = np.histogram2d(x, y, bins=[xe, ye])[0]
    assert np.array_equal(counts, want) and counts.tolist() == [[1, 0], [1, 3]] and outside == 3
    for bad in ([0.0, 0.0, 1.0], [0.0, np.nan], [1.0], [0.0, np.inf]):
        with pytest.raises(ValueError, match="strictly increasing"):
            em.bin_counts_2d(x, y, bad, ye)


@pytest.fixture(scope="module")
def h3n2():
    m = core.coded_matrix(pp.h3n2_matrix())
    n = m.values.shape[0]
    rng = np.random.default_rng(11)
    pos = rng.normal(size=(n, 3)) * 2.0
    pred = np.sqrt(((pos[:, None] - pos[None]) ** 2).sum(-1))
    cells = np.flatnonzero(np.isfinite(m.values).ravel(order="F"))
    picks = rng.choice(cells, cells.size // 20, replace=False)
    return m, pred, picks


@pytest.mark.parametrize("series", ["in", "out", "all"])
def test_embedding_quality_data_host_form_on_the_h3n2_panel(h3n2, series):
    m, pred, picks = h3n2
    n = m.values.shape[0]
    q = em.embedding_quality_data(m, pred, holdout=picks, series=series, bins=(48, 32))
    held = np.zeros((n, n), dtype=bool)
    held[picks % n, picks // n] = True
    held |= held.T
    fin = np.isfinite(m.values)
    mask = {"in": fin & (m.codes == 0) & ~held, "out": fin & (m.codes == 0) & held, "all": fin}[series]
    v, r = m.values[mask], pred[mask]
    assert q.n == v.size > 100 and q.series == series
    assert q.statistics.n == int(fin.sum()) and (q.statistics.in_sample.n, q.statistics.out_sample.n) == (
        int((fin & (m.codes == 0) & ~held).sum()), int((fin & (m.codes == 0) & held).sum()))
    for cloud, x, y in ((q.scatter, v, r), (q.residual_vs_true, v, r - v), (q.residual_vs_fitted, r, v - r)):
        assert cloud.counts.shape == (48, 32) and cloud.x_edges.shape == (49,) and cloud.y_edges.shape == (33,)
        want = np.histogram2d(x, y, bins=[cloud.x_edges, cloud.y_edges])[0]
        assert np.array_equal(cloud.counts, want.astype(np.int64))
        assert cloud.counts.sum() + cloud.outside == cloud.n == q.n
        assert cloud.outside == 0                                            # the default edges span the series
        assert cloud.conditional_quantiles((0.5,)).shape == (1, 48)
    assert q.scatter.x_edges[0] == 0.0 and q.scatter.x_edges[-1] == v.max() and q.scatter.y_edges[-1] == r.max()
    assert q.residual_vs_true.y_edges[0] == (r - v).min() and q.residual_vs_fitted.y_edges[-1] == (v - r).max()
    if series == "all":
        assert q.scatter.counts.sum() == q.statistics.n                     # the scatter's total is the titles' n
    # the density is density.default of the residuals, up to the float32 rounding of the sd inside the bandwidth
    d, raw = q.residual_density, em.density_default(r - v)
    assert d.n == q.n and d.bw == pytest.approx(raw.bw, rel=1e-7)
    assert np.abs(d.y - np.interp(d.x, raw.x, raw.y)).max() <= 1e-5 * raw.y.max()
    again = em.density_default(r - v, bw=d.bw)
    assert np.array_equal(again.y, d.y) and np.array_equal(again.x, d.x)


def test_embedding_quality_data_small_cases():
    truth = np.array([["0", "2", ">3"], ["2", "0", "4"], [">3", "4", "0"]], dtype=object)
    pred = np.array([[0.0, 1.5, 2.5], [1.5, 0.0, 5.0], [2.5, 5.0, 0.0]])
    q = em.embedding_quality_data(truth, pred, series="out", bins=(4, 4))    # no hold-out: an empty series
    assert q.n == 0 and q.residual_density is None and q.statistics.n == 9
    for cloud in (q.scatter, q.residual_vs_true, q.residual_vs_fitted):
        assert not cloud.counts.any() and cloud.outside == 0 and np.isnan(cloud.conditional_quantiles()).all()
    q = em.embedding_quality_data(truth, pred, series="in", bins=(2, 2))     # the diagonal counts: 3 cells at (0, 0)
    assert q.n == 7 and q.scatter.counts[0, 0] == 3 and q.scatter.counts.sum() == 7
    assert q.residual_density is not None and q.residual_density.n == 7
    with pytest.raises(ValueError, match="series"):
        em.embedding_quality_data(truth, pred, series="both")
    with pytest.raises(ValueError, match="bins"):
        em.embedding_quality_data(truth, pred, bins=(128, 128))
    doc = em.embedding_quality_data.__doc__
    assert "masks the diagonal" in doc and "DEVIATION" in doc
    import topolow_amd
    for name in ("embedding_quality_data", "EmbeddingQualityData", "BinnedCloud", "Density", "density_default", "bw_nrd0"):
        assert name in topolow_amd.__all__ and getattr(topolow_amd, name) is getattr(em, name)
