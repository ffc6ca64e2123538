"""topolow_amd.error_metrics on the host: the reference's error_calculator_comparison (R/error_metrics.R:55-144) and
calculate_prediction_interval (:160-202), the Student-t quantile the package computes without SciPy, R's type-7
quantile from order statistics, and fit_statistics' host form -- the specification of the device form
(tests/test_gpu_fit_report.py)."""
import math
import os

import numpy as np
import pytest

import topolow_amd
from topolow_amd import core, error_metrics as em

TRUE = np.array([[0.0, 1.0, 2.0], [1.0, 0.0, 3.0], [2.0, 3.0, 0.0]])      # R/error_metrics.R:40


def _pred():
    return TRUE + np.random.default_rng(3).normal(0.0, 0.1, (3, 3))         # :41


def test_reference_example_1_everything_is_in_sample():
    pred = _pred()
    out = em.error_calculator_comparison(pred, TRUE)
    assert set(out) == {"InSampleError", "OutSampleError", "Completeness", "InSamplePercentageError",
                        "OutSamplePercentageError"}
    want = (TRUE - pred).ravel(order="F")
    np.testing.assert_array_equal(out["InSampleError"], want)
    assert np.isnan(out["OutSampleError"]).all() and np.isnan(out["OutSamplePercentageError"]).all()
    pos = TRUE.ravel(order="F") > 0
    np.testing.assert_array_equal(out["InSamplePercentageError"][pos], want[pos] / TRUE.ravel(order="F")[pos] * 100.0)
    assert np.isnan(out["InSamplePercentageError"][~pos]).all()            # the diagonal: truth 0
    assert out["Completeness"] == 1.0                                       # no hold-out: predictions / truths = 9 / 9


def test_reference_example_2_one_held_out_pair():
    pred = _pred()
    inp = TRUE.copy()
    inp[0, 2] = inp[2, 0] = np.nan                                          # :48
    out = em.error_calculator_comparison(pred, TRUE, inp)
    held = np.isnan(inp).ravel(order="F")
    want = (TRUE - pred).ravel(order="F")
    np.testing.assert_array_equal(out["OutSampleError"][held], want[held])
    assert np.isnan(out["OutSampleError"][~held]).all() and np.isnan(out["InSampleError"][held]).all()
    np.testing.assert_array_equal(out["OutSamplePercentageError"][held], want[held] / 2.0 * 100.0)
    assert out["Completeness"] == 1.0
    base = topolow_amd.cv.error_calculator_comparison(pred, TRUE, inp)      # the partial form is untouched and contained
    for k, v in base.items():
        np.testing.assert_array_equal(out[k], v)


def test_threshold_strings_leave_in_and_out_but_stay_in_all():
    truth = np.array([["0", "<2", "3"], ["<2", "0", ">4"], ["3", ">4", "0"]], dtype=object)
    pred = np.array([[0.1, 1.5, 2.5], [1.5, 0.2, 5.0], [2.5, 5.0, 0.3]])
    out = em.error_calculator_comparison(pred, truth)
    assert int((~np.isnan(out["InSampleError"])).sum()) == 5                # diagonal and the pair (0, 2)
    fs = em.fit_statistics(truth, pred, holdout=[2])                        # cell (2, 0) and its mirror
    assert (fs.in_sample.n, fs.out_sample.n, fs.n) == (3, 2, 9)
    assert fs.out_sample.min == fs.out_sample.max == 0.5
    numeric = np.array([[0, 2, 3], [2, 0, 4], [3, 4, 0.0]])
    assert fs.mae == pytest.approx(np.abs(numeric - pred).mean(), rel=1e-15)
    # holding out a threshold cell moves nothing between IN and OUT
    fs2 = em.fit_statistics(truth, pred, holdout=[1])
    assert (fs2.in_sample.n, fs2.out_sample.n, fs2.n) == (5, 0, 9)


def test_named_matrices_are_reordered_and_a_mismatch_raises_the_references_text():
    pred = _pred()
    names = ["a", "b", "c"]
    perm = [2, 0, 1]
    shuffled = pred[np.ix_(perm, perm)]
    out = em.error_calculator_comparison(shuffled, core.RMatrix(TRUE, names), pred_names=[names[q] for q in perm])
    np.testing.assert_array_equal(out["InSampleError"], (TRUE - pred).ravel(order="F"))
    with pytest.raises(ValueError, match="Row and column names must match between matrices after ordering"):
        em.error_calculator_comparison(shuffled, core.RMatrix(TRUE, names), pred_names=["a", "b", "x"])
    with pytest.raises(ValueError, match="All matrices must have the same dimensions"):
        em.error_calculator_comparison(pred[:2, :2], TRUE)


def test_both_completeness_branches():
    pred = _pred()
    inp = TRUE.copy()
    inp[0, 2] = inp[2, 0] = np.nan
    part = pred.copy()
    part[0, 2] = np.nan                                                     # one of the two validation cells predicted
    assert em.error_calculator_comparison(part, TRUE, inp)["Completeness"] == 0.5
    assert em.fit_statistics(TRUE, part, input_dissimilarities=inp).Completeness == 0.5
    assert em.fit_statistics(TRUE, part, holdout=[6]).Completeness == 0.5  # 0 + 2 * 3: the same pair as picks
    truth = TRUE.copy()
    truth[0, 1] = truth[1, 0] = np.nan                                      # no hold-out: 8 predictions / 7 truths
    assert em.error_calculator_comparison(part, truth)["Completeness"] == pytest.approx(8 / 7)
    assert em.fit_statistics(truth, part).Completeness == pytest.approx(8 / 7)
    assert em.error_calculator_comparison(pred, np.full((3, 3), np.nan))["Completeness"] == 0


def test_every_validation_message_of_the_prediction_interval():
    pred = _pred()
    with pytest.raises(ValueError, match="Both inputs must be matrices"):
        em.calculate_prediction_interval(TRUE, [1.0, 2.0])
    with pytest.raises(ValueError, match="Both inputs must be matrices"):
        em.calculate_prediction_interval("x", pred)
    with pytest.raises(ValueError, match="Matrices must have the same dimensions"):
        em.calculate_prediction_interval(TRUE, pred[:2, :2])
    for level in (0.0, 1.0, -0.5, 1.5, "0.9"):
        with pytest.raises(ValueError, match="confidence_level must be between 0 and 1"):
            em.calculate_prediction_interval(TRUE, pred, level)
    with pytest.raises(ValueError, match="Matrices must have at least 2 rows/columns for meaningful prediction intervals"):
        em.calculate_prediction_interval(np.zeros((1, 1)), np.zeros((1, 1)))
    lonely = np.full((3, 3), np.nan)
    lonely[0, 1] = 1.0
    with pytest.raises(ValueError, match="Fewer than 2 valid paired observations found. Cannot calculate prediction interval."):
        em.calculate_prediction_interval(lonely, pred)
    # the reference's order: the matrix check comes before the level, the level before the size
    with pytest.raises(ValueError, match="Both inputs must be matrices"):
        em.calculate_prediction_interval(TRUE, None, 7)
    with pytest.raises(ValueError, match="confidence_level"):
        em.calculate_prediction_interval(np.zeros((1, 1)), np.zeros((1, 1)), 7)


def test_prediction_interval_is_qt_times_sd_over_the_all_rule():
    truth = np.array([["0", "<2", "3"], ["<2", "0", ">4"], ["3", ">4", "NA"]], dtype=object)
    pred = _pred() * 1.3
    numeric = np.array([[0, 2, 3], [2, 0, 4], [3, 4, np.nan]])
    res = (numeric - pred).ravel()[:8]
    want = em.student_t_quantile(0.975, 7) * res.std(ddof=1)
    assert em.calculate_prediction_interval(truth, pred) == pytest.approx(want, rel=1e-14)
    assert em.fit_statistics(truth, pred).prediction_interval == pytest.approx(want, rel=1e-13)
    assert em.calculate_prediction_interval(truth, pred, 0.5) == pytest.approx(em.student_t_quantile(0.75, 7) * res.std(ddof=1))


# qt((1 + level) / 2, df): 20 digits of a 50-digit solve of I_x(df / 2, 1 / 2) / 2 = (1 - level) / 2 (mpmath 1.3), and what
# scipy.stats.t.ppf (SciPy 1.15.3) returned for the same arguments.  Generated once, pasted.
LEVELS = (0.8, 0.95, 0.999)
T_EXACT = {1: (3.0776835371752541331, 12.706204736174693314, 636.61924876878972983),
           2: (1.8856180831641270225, 4.3026527297494617894, 31.599054576445363413),
           5: (1.4758840488244812516, 2.5705818356363147828, 6.8688266258812751318),
           30: (1.3104150253913957112, 2.0422724563012378878, 3.6459586350420628079),
           10 ** 4: (1.2816362297304776706, 1.9602012398906258778, 3.2914999659416356914),
           10 ** 7: (1.2815516502030830147, 1.9599642217672051104, 3.2905277044652534353)}
T_SCIPY = {1: (3.0776835372078066, 12.706204736432095, 636.6192487687896),
           2: (1.8856180831641507, 4.302652729696142, 31.599054577041514),
           5: (1.4758840488558216, 2.570581835636314, 6.868826625881279),
           30: (1.310415025391396, 2.0422724563012373, 3.6459586349971502),
           10 ** 4: (1.2816362297304775, 1.960201239890626, 3.2914999659416355),
           10 ** 7: (1.281551650203083, 1.959964221767205, 3.290527704465253)}
SCIPY_OWN_ERROR = 5e-11     # T_SCIPY against T_EXACT: up to 2.1e-11 relative (df 1, 2, 5, 30), SciPy's inverse, not ours


def own_bound(df, t):
    """student_t_quantile's docstring: 1e-12 from the continued fraction's stopping rule and the prefactor; where
    t^2 > 3 the fraction runs in x = df / (df + t^2), whose rounding adds 2^-52 df / t^2."""
    return 1e-12 + (2.0 ** -52 * df / (t * t) if t * t > 3.0 else 0.0)


@pytest.mark.parametrize("df", sorted(T_EXACT))
def test_t_quantile_against_pinned_constants(df):
    for level, exact, scipy_value in zip(LEVELS, T_EXACT[df], T_SCIPY[df]):
        got = em.student_t_quantile((1.0 + level) / 2.0, df)
        assert abs(got / exact - 1.0) <= own_bound(df, exact), (df, level, got, exact)
        assert abs(got / scipy_value - 1.0) <= own_bound(df, exact) + SCIPY_OWN_ERROR, (df, level, got, scipy_value)
        assert abs(scipy_value / exact - 1.0) <= SCIPY_OWN_ERROR                      # the constant above holds
        assert em.student_t_quantile((1.0 - level) / 2.0, df) == pytest.approx(-got, rel=1e-9)
    assert em.student_t_quantile(0.5, df) == 0.0
    assert math.isnan(em.student_t_quantile(1.0, df)) and math.isnan(em.student_t_quantile(0.3, 0))


def test_t_quantile_against_scipy_itself():
    stats = pytest.importorskip("scipy.stats")
    for df in (1, 3, 17, 250, 123456, 3 * 10 ** 6):
        for level in (0.8, 0.9, 0.99, 0.9999):
            p = (1.0 + level) / 2.0
            want = float(stats.t.ppf(p, df))
            assert abs(em.student_t_quantile(p, df) / want - 1.0) <= own_bound(df, want) + SCIPY_OWN_ERROR


def test_the_package_does_not_import_scipy():
    import subprocess
    import sys
    code = "import sys, topolow_amd, topolow_amd.error_metrics; sys.exit(1 if 'scipy' in sys.modules else 0)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert subprocess.run([sys.executable, "-c", code], cwd=root).returncode == 0


@pytest.mark.parametrize("values", [[5.0], [2.0, -1.0], [1.0, 1.0, 1.0, 2.0, 2.0, 7.0, 7.0, 7.0, 7.0],
                                    list(np.random.default_rng(0).normal(size=101)),
                                    list(np.random.default_rng(1).integers(-2, 3, size=40).astype(float))])
def test_type7_quantiles_against_numpy(values):
    x = np.sort(np.asarray(values))
    probs = [0.0, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.75, 0.9, 1.0]
    calls = []

    def order_stats(ranks):
        calls.append(list(ranks))
        return x[list(ranks)]
    got = em.type7_quantiles(x.size, probs, order_stats)
    want = np.quantile(x, probs)
    scale = np.abs(x).max()
    np.testing.assert_allclose(got, want, rtol=0, atol=4 * np.finfo(float).eps * scale)    # NumPy's lerp rounds otherwise
    assert got[0] == x[0] and got[-1] == x[-1] and (x.size % 2 == 0 or got[4] == x[x.size // 2])
    for p, g in zip(probs, got):                                            # a quantile inside a run of ties is the tie
        lo, hi = x[int(math.floor((x.size - 1) * p))], x[int(math.ceil((x.size - 1) * p))]
        assert lo <= g <= hi and (lo != hi or g == lo)
    assert len(calls) == 1 and calls[0] == sorted(set(calls[0])) and max(calls[0]) < x.size
    assert np.isnan(em.type7_quantiles(0, [0.5], order_stats)).all() and len(calls) == 1
    with pytest.raises(ValueError):
        em.type7_quantiles(3, [1.5], order_stats)


def test_fit_statistics_host_form_against_numpy():
    rng = np.random.default_rng(11)
    n = 23
    pts = rng.normal(size=(n, 3))
    dist = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1))
    truth = dist * (1 + 0.2 * rng.normal(size=(n, n)))
    truth = np.triu(truth, 1) + np.triu(truth, 1).T
    truth[rng.random((n, n)) < 0.2] = np.nan
    truth[3, 4] = np.inf                                                    # left out of every series
    codes = np.zeros((n, n), dtype=np.int8)
    codes[5, 6] = codes[6, 5] = 1
    picks = rng.choice(n * n, 60, replace=False)
    fs = em.fit_statistics(core.CodedMatrix(truth, codes), dist, holdout=picks, probs=(0.1, 0.25, 0.5, 0.75))
    held = np.zeros((n, n), dtype=bool)
    held[picks % n, picks // n] = True
    held |= held.T
    fin = np.isfinite(truth)
    e = truth - dist
    for got, mask in ((fs.in_sample, fin & (codes == 0) & ~held), (fs.out_sample, fin & (codes == 0) & held)):
        x = e[mask]
        assert got.n == x.size and got.min == x.min() and got.max == x.max()
        assert got.mean == pytest.approx(x.mean(), rel=1e-13) and got.sd == pytest.approx(x.std(ddof=1), rel=1e-13)
        assert got.mae == pytest.approx(np.abs(x).mean(), rel=1e-13)
        np.testing.assert_allclose(got.quantiles, np.quantile(x, [0.1, 0.25, 0.5, 0.75]), rtol=1e-13, atol=1e-15)
        assert got.median == pytest.approx(np.median(x), rel=1e-13, abs=1e-15)
        v = truth[mask]
        pct = x[v > 0] / v[v > 0] * 100
        assert got.mean_percentage_error == pytest.approx(pct.mean(), rel=1e-12)
        assert got.mean_abs_percentage_error == pytest.approx(np.abs(pct).mean(), rel=1e-12)
    v, r = truth[fin], dist[fin]
    assert fs.n == v.size and fs.mae == pytest.approx(np.abs(v - r).mean(), rel=1e-13)
    assert fs.pearson_r == pytest.approx(np.corrcoef(r, v)[0, 1], rel=1e-12)
    slope, intercept = np.polyfit(v, r, 1)                                  # lm(pred ~ true)
    assert fs.slope == pytest.approx(slope, rel=1e-11) and fs.intercept == pytest.approx(intercept, rel=1e-9, abs=1e-12)
    assert fs.residual_sd == pytest.approx((v - r).std(ddof=1), rel=1e-13)
    assert fs.prediction_interval == pytest.approx(em.student_t_quantile(0.975, v.size - 1) * (v - r).std(ddof=1), rel=1e-13)
    assert fs.Completeness == 1.0
    # input_dissimilarities marks the same hold-out as the picks
    inp = np.where(held, np.nan, truth)
    fs2 = em.fit_statistics(core.CodedMatrix(truth, codes), dist, input_dissimilarities=core.CodedMatrix(inp, codes),
                            probs=(0.1, 0.25, 0.5, 0.75))
    assert fs2.out_sample.n == fs.out_sample.n and fs2.out_sample.sd == fs.out_sample.sd
    assert fs2.in_sample.median == fs.in_sample.median


def test_fit_statistics_argument_errors():
    with pytest.raises(ValueError, match="confidence_level"):
        em.fit_statistics(TRUE, _pred(), confidence_level=1.0)
    with pytest.raises(ValueError, match="host form"):
        em.fit_statistics(TRUE)
    with pytest.raises(ValueError, match="same dimensions"):
        em.fit_statistics(TRUE, np.zeros((2, 2)))
    with pytest.raises(ValueError, match="not both"):
        em.fit_statistics(TRUE, _pred(), input_dissimilarities=TRUE, holdout=[1])
    with pytest.raises(ValueError, match="picks"):
        em.fit_statistics(TRUE, _pred(), holdout=[9])
    empty = em.fit_statistics(TRUE, _pred())                                # no hold-out: OUT is empty, not an error
    assert empty.out_sample.n == 0 and math.isnan(empty.out_sample.mean) and np.isnan(empty.out_sample.quantiles).all()


def test_all_holds_the_new_names():
    for name in ("error_calculator_comparison", "calculate_prediction_interval", "fit_statistics", "FitStatistics"):
        assert name in topolow_amd.__all__ and hasattr(topolow_amd, name)
    assert topolow_amd.error_calculator_comparison is em.error_calculator_comparison
