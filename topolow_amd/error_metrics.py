"""The evaluation of a fit (reference R/error_metrics.R): `error_calculator_comparison` (:55-144),
`calculate_prediction_interval` (:160-202), and `fit_statistics`, which gathers what the reference prints about a fit --
the statistics of `scatterplot_fitted_vs_true` (R/visualization.R:2626-2648: MAE, Pearson's r, the regression line, the
prediction interval) and the summary its notebook makes of the signed errors
(inst/examples/methods-comparison-h3n2-hiv-denv.Rmd:2339-2349: mean, sd, median, Q1, Q3).

`fit_statistics(D, predicted, ...)` is the host form in NumPy and the specification of the device form,
`fit_statistics(D, handle=h, positions=P, holdout=picks)`, which runs on the matrix a PreparedHandle keeps on the device
(topolow_layout_prep_fit_report / _fit_order_stats, include/topolow_relax.h) and touches nothing of size n x n on the
host.  The device form is taken only when a handle is passed.

A cell belongs to zero or more of three series: IN (finite, no threshold prefix, not held out), OUT (finite, no
prefix, held out) and ALL (finite, with or without a prefix, held out or not: `extract_numeric_values`).  The diagonal
counts.  DEVIATION from the reference: cells that are +-Inf are left out of every series, as `post_metrics` leaves them
out; in the reference they would turn every statistic into Inf or NaN.  This holds for `fit_statistics` in both forms;
`error_calculator_comparison` and `calculate_prediction_interval` are the reference's functions as they are.

`embedding_quality_data` returns the data behind the reference's diagnostic plots of a fit
(`scatterplot_fitted_vs_true`, R/visualization.R:2616-2701; `plot_embedding_quality`, R/diagnostics.R:128-183) without
their point clouds: exact 2-D bin counts (`BinnedCloud`, whose conditional quantiles replace the plots' loess), the
residual density as `density.default` computes it (`density_default`, `bw_nrd0`) and the FitStatistics.  It has the same
two forms; the device form reads the resident matrix through topolow_layout_prep_fit_extent / _fit_hist2d /
_fit_linear_bins."""
import math
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Sequence

import numpy as np

from . import _native, cv
from .core import _as_rmatrix, coded_matrix

__all__ = ["error_calculator_comparison", "calculate_prediction_interval", "fit_statistics", "FitStatistics",
           "SeriesStatistics", "student_t_quantile", "type7_quantiles", "bw_nrd0", "density_grid", "linear_bin_counts",
           "linear_bin_masses", "density_default", "Density", "BinnedCloud", "bin_counts_2d", "embedding_quality_data",
           "EmbeddingQualityData"]


# --------------------------------------------------------------------------------------
# error_calculator_comparison
# --------------------------------------------------------------------------------------
def error_calculator_comparison(predicted, true, input_=None, pred_names=None, true_names=None) -> Dict:
    """R/error_metrics.R:55-144, complete: `cv.error_calculator_comparison`'s InSampleError, OutSampleError (vectors
    over the cells in column-major order, NaN = NA) and Completeness, plus InSamplePercentageError and
    OutSamplePercentageError: error / truth * 100 where the truth is > 0, NA elsewhere (:116-124)."""
    out = cv.error_calculator_comparison(predicted, true, input_, pred_names, true_names)
    truth = cv._numeric(true).ravel(order="F")
    positive = ~np.isnan(truth) & (truth > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        for name in ("InSample", "OutSample"):
            out[name + "PercentageError"] = np.where(positive, out[name + "Error"] / truth * 100.0, np.nan)
    return out


# --------------------------------------------------------------------------------------
# Student's t quantile without SciPy
# --------------------------------------------------------------------------------------
def _log_gamma_ratio_half(b: float) -> float:
    """ln Gamma(b + 1/2) - ln Gamma(b).  Below 40 both lgammas are below 110 in size, so their difference is good to
    ~3e-14 absolute; from 40 on the asymptotic series, whose first omitted term is below 1e-17."""
    if b < 40.0:
        return math.lgamma(b + 0.5) - math.lgamma(b)
    r = 1.0 / b
    r2 = r * r
    return 0.5 * math.log(b) + r * (-1.0 / 8.0 + r2 * (1.0 / 192.0 + r2 * (-1.0 / 640.0 + r2 * (17.0 / 14336.0))))


def _beta_cf(a: float, b: float, x: float) -> float:
    """The continued fraction of the incomplete beta function by the modified Lentz method; it converges in
    O(sqrt(max(a, b))) steps for x < (a + 1) / (a + b + 2)."""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    if abs(d) < tiny:
        d = tiny
    d = 1.0 / d
    h = d
    for m in range(1, 200001):
        m2 = 2 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        if abs(d) < tiny:
            d = tiny
        c = 1.0 + aa / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        if abs(d) < tiny:
            d = tiny
        c = 1.0 + aa / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 2e-16:
            return h
    raise ArithmeticError("the incomplete beta continued fraction did not converge")


def _t_upper_tail(t: float, df: float) -> float:
    """P(T > t) for t >= 0: I_x(df / 2, 1 / 2) / 2 with x = df / (df + t^2), the regularised incomplete beta function.
    1 - x = t^2 / (df + t^2) and ln x = -log1p(t^2 / df) are formed directly, so nothing cancels for large df."""
    if t <= 0.0:
        return 0.5
    a, b = 0.5 * df, 0.5
    u = t * t / df
    x, y = 1.0 / (1.0 + u), u / (1.0 + u)           # x, 1 - x
    log_x, log_y = -math.log1p(u), math.log(u) - math.log1p(u)
    log_front = a * log_x + b * log_y + _log_gamma_ratio_half(a) - 0.5 * math.log(math.pi)   # 1 / B(a, 1/2)
    if x < (a + 1.0) / (a + b + 2.0):
        inc = math.exp(log_front) * _beta_cf(a, b, x) / a
    else:
        inc = 1.0 - math.exp(log_front) * _beta_cf(b, a, y) / b
    return 0.5 * inc


def student_t_quantile(p: float, df: float) -> float:
    """stats::qt(p, df) for 0 < p < 1 and df > 0: the upper tail P(T > t) = 1 - p solved for t by bisection (the tail is
    monotone), to the last bits of t.
    Accuracy, for p >= 0.9 (where dt / t = (dq / q) * q / (t f(t)) and q / (t f(t)) < 1.6): the continued fraction stops
    at 2e-16 per step and the prefactor's exponent is good to 1e-13, which keeps 1e-12 relative.  Where t^2 > 3 the
    fraction runs in x = df / (df + t^2), and the rounding of x, 2^-53, is a relative error 2^-53 (df + t^2) / t^2 of
    1 - x, on which the fraction depends with about unit sensitivity: there the bound is 1e-12 + 2^-52 df / t^2 -- 6e-11
    at df = 10^7, t = 1.96; nothing a prediction interval can show."""
    p, df = float(p), float(df)
    if not (0.0 < p < 1.0) or not df > 0.0:
        return math.nan
    if p == 0.5:
        return 0.0
    if p < 0.5:
        return -student_t_quantile(1.0 - p, df)
    q = 1.0 - p           # exact for 0.5 <= p < 1
    lo, hi = 0.0, 1.0
    while _t_upper_tail(hi, df) > q:
        lo, hi = hi, 2.0 * hi
        if hi > 1e300:
            return math.inf
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if not (lo < mid < hi):
            break
        if _t_upper_tail(mid, df) > q:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


# --------------------------------------------------------------------------------------
# calculate_prediction_interval
# --------------------------------------------------------------------------------------
def calculate_prediction_interval(dissimilarity_matrix, predicted, confidence_level=0.95) -> float:
    """R/error_metrics.R:160-202: qt((1 + level) / 2, m - 1) * sd(truth - predicted) over the cells where both are not
    NA, the truth by `extract_numeric_values` (threshold cells count with the number behind the prefix).  The
    reference's four validation messages, in its order, as ValueError."""
    truth_m = coded_matrix(dissimilarity_matrix)
    pred_m = _as_rmatrix(predicted)
    if truth_m is None or pred_m is None:
        raise ValueError("Both inputs must be matrices")
    pred = np.asarray(pred_m.values, dtype=np.float64)
    if truth_m.values.shape != pred.shape:
        raise ValueError("Matrices must have the same dimensions")
    if (isinstance(confidence_level, bool) or not isinstance(confidence_level, (int, float, np.integer, np.floating))
            or not (0 < confidence_level < 1)):
        raise ValueError("confidence_level must be between 0 and 1")
    if truth_m.values.shape[0] < 2:
        raise ValueError("Matrices must have at least 2 rows/columns for meaningful prediction intervals")
    truth = truth_m.values.ravel(order="F")
    predv = pred.ravel(order="F")
    valid = ~np.isnan(truth) & ~np.isnan(predv)
    m = int(valid.sum())
    if m < 2:
        raise ValueError("Fewer than 2 valid paired observations found. Cannot calculate prediction interval.")
    residuals = truth[valid] - predv[valid]
    return student_t_quantile((1.0 + float(confidence_level)) / 2.0, m - 1) * float(np.std(residuals, ddof=1))


# --------------------------------------------------------------------------------------
# fit_statistics
# --------------------------------------------------------------------------------------
def type7_quantiles(m: int, probs: Sequence[float], order_stats: Callable[[Sequence[int]], Sequence[float]]) -> np.ndarray:
    """R's quantile(type = 7) of m values at `probs` from their order statistics: h = (m - 1) p, the value at rank
    floor(h) plus (h - floor(h)) times the step to the next rank.  `order_stats(ranks)` returns the values at the given
    0-based ranks of the ascending values (ranks ascending and unique); it is called once.  m = 0 gives NaN."""
    probs = [float(p) for p in probs]
    if any(not (0.0 <= p <= 1.0) for p in probs):
        raise ValueError("probs must lie in [0, 1]")
    if m <= 0 or not probs:
        return np.full(len(probs), np.nan)
    plan = []
    for p in probs:
        h = (m - 1) * p
        lo = min(int(math.floor(h)), m - 1)
        frac = h - lo
        plan.append((lo, min(lo + 1, m - 1) if frac > 0.0 else lo, frac))
    ranks = sorted({r for lo, hi, _ in plan for r in (lo, hi)})
    got = dict(zip(ranks, (float(v) for v in order_stats(ranks))))
    return np.array([got[lo] + frac * (got[hi] - got[lo]) if hi != lo else got[lo] for lo, hi, frac in plan])


@dataclass
class SeriesStatistics:
    """The signed errors truth - predicted of one series (IN or OUT)."""
    n: int
    mean: float
    sd: float            # n - 1 in the denominator; NaN for n < 2
    mae: float
    min: float
    max: float
    quantiles: np.ndarray   # R's type 7, at FitStatistics.probs
    median: float
    mean_percentage_error: float        # over the cells with truth > 0 (R/error_metrics.R:116-124)
    mean_abs_percentage_error: float


@dataclass
class FitStatistics:
    in_sample: SeriesStatistics
    out_sample: SeriesStatistics
    Completeness: float
    probs: tuple
    # over ALL (scatterplot_fitted_vs_true, calculate_prediction_interval)
    n: int
    mae: float
    pearson_r: float
    slope: float         # of predicted ~ true
    intercept: float
    residual_sd: float   # sd(truth - predicted), n - 1
    prediction_interval: float
    seconds: Optional[list] = None   # device form: pass 1, pass 2 and the whole of the report


def _div(x, y):
    return x / y if y else math.nan


def _series_from_moments(s: Dict, probs, order_stats) -> SeriesStatistics:
    """s: count, sum_e, sum_abs_e, min_e, max_e, css_e, pct_count, sum_pct, sum_abs_pct."""
    m = int(s["count"])
    q = type7_quantiles(m, list(probs) + [0.5], order_stats)
    return SeriesStatistics(
        n=m, mean=_div(s["sum_e"], m), sd=math.sqrt(s["css_e"] / (m - 1)) if m > 1 else math.nan,
        mae=_div(s["sum_abs_e"], m), min=float(s["min_e"]) if m else math.nan, max=float(s["max_e"]) if m else math.nan,
        quantiles=q[:-1], median=float(q[-1]), mean_percentage_error=_div(s["sum_pct"], int(s["pct_count"])),
        mean_abs_percentage_error=_div(s["sum_abs_pct"], int(s["pct_count"])))


def _completeness(n_out: int, n_validation: int, n_predictions: int, n_possible: int) -> float:
    """R/error_metrics.R:131-138, both branches."""
    if n_validation > 0:
        return n_out / n_validation
    return n_predictions / n_possible if n_possible > 0 else 0.0


def _assemble(moments: Dict, probs, order_stats_of, n_validation, n_predictions, n_possible, confidence_level,
              seconds=None):
    a = moments["all"]
    m = int(a["count"])
    ins = _series_from_moments(moments["in"], probs, order_stats_of("in"))
    outs = _series_from_moments(moments["out"], probs, order_stats_of("out"))
    vv, rr, vr = a["css_v"], a["css_r"], a["css_vr"]
    slope = vr / vv if m > 0 and vv > 0 else math.nan
    residual_sd = math.sqrt(a["css_e"] / (m - 1)) if m > 1 else math.nan
    return FitStatistics(
        in_sample=ins, out_sample=outs,
        Completeness=_completeness(outs.n, n_validation, n_predictions, n_possible), probs=tuple(probs),
        n=m, mae=_div(a["sum_abs_e"], m), pearson_r=vr / math.sqrt(vv * rr) if m > 1 and vv > 0 and rr > 0 else math.nan,
        slope=slope, intercept=_div(a["sum_r"], m) - slope * _div(a["sum_v"], m), residual_sd=residual_sd,
        prediction_interval=student_t_quantile((1.0 + confidence_level) / 2.0, m - 1) * residual_sd if m > 1 else math.nan,
        seconds=seconds)


def _host_moments(e: np.ndarray, v: np.ndarray, r: np.ndarray, with_vr: bool) -> Dict:
    """The fields of topolow_fit_series from the series' errors, truths and predictions; every sum two-pass."""
    m = int(e.size)
    out = dict(count=m, sum_e=float(np.sum(e)), sum_abs_e=float(np.sum(np.abs(e))),
               min_e=float(e.min()) if m else math.nan, max_e=float(e.max()) if m else math.nan,
               pct_count=0, sum_pct=0.0, sum_abs_pct=0.0, sum_v=0.0, sum_r=0.0, css_e=0.0, css_v=0.0, css_r=0.0, css_vr=0.0)
    if m:
        out["css_e"] = float(np.sum((e - out["sum_e"] / m) ** 2))
    if with_vr:
        out["sum_v"], out["sum_r"] = float(np.sum(v)), float(np.sum(r))
        if m:
            dv, dr = v - out["sum_v"] / m, r - out["sum_r"] / m
            out["css_v"], out["css_r"], out["css_vr"] = float(np.sum(dv * dv)), float(np.sum(dr * dr)), float(np.sum(dv * dr))
    else:
        pos = v > 0
        p = e[pos] / v[pos] * 100.0
        out["pct_count"], out["sum_pct"], out["sum_abs_pct"] = int(pos.sum()), float(np.sum(p)), float(np.sum(np.abs(p)))
    return out


def _holdout_mask(n: int, input_dissimilarities, holdout) -> np.ndarray:
    """The held-out cells, n x n bool: where `input_dissimilarities` is NA under as.numeric (R/error_metrics.R:90-95)
    but the truth is not, or the picks of `holdout` (linear column-major indices r + c * n) and their mirrors."""
    if input_dissimilarities is not None and holdout is not None:
        raise ValueError("give input_dissimilarities or holdout, not both")
    held = np.zeros((n, n), dtype=bool)
    if input_dissimilarities is not None:
        im = coded_matrix(input_dissimilarities)
        if im is None or im.values.shape != (n, n):
            raise ValueError("All matrices must have the same dimensions")
        held = np.isnan(im.as_numeric())
    elif holdout is not None:
        picks = np.asarray(holdout, dtype=np.int64).reshape(-1)
        if picks.size and (picks.min() < 0 or picks.max() >= n * n):
            raise ValueError("holdout picks must be linear column-major indices 0 .. n * n - 1")
        r, c = picks % n, picks // n
        held[r, c] = True
        held[c, r] = True
    return held


def fit_statistics(dissimilarity_matrix, predicted=None, *, input_dissimilarities=None, holdout=None, positions=None,
                   handle: Optional["_native.PreparedHandle"] = None, probs=(0.25, 0.5, 0.75),
                   confidence_level=0.95) -> FitStatistics:
    """What the reference reports about a fit, as one FitStatistics (see the module's text for the series and the Inf
    deviation).  Per series IN and OUT: n, mean, sd, mae, min, max, the type-7 quantiles at `probs`, the median, the
    mean and mean-absolute percentage error.  Completeness by the reference's rule (over finite cells).  Over ALL: n,
    mae, Pearson's r, slope and intercept of predicted ~ true, the residual sd and the prediction interval.

    Host form (no `handle`): `predicted` is the n x n matrix of predicted dissimilarities (NaN: no prediction; such
    cells are in no series); the held-out cells are those NA in `input_dissimilarities` but not in the truth, or the
    picks of `holdout` and their mirrors.  NumPy on n x n temporaries; this form is the specification.

    Device form (`handle=` a PreparedHandle of this matrix and `positions=` n x ndim, row q for the q-th point of the
    handle's ordered matrix; `dissimilarity_matrix` and `predicted` may be None): one fit_report and at most two
    fit_order_stats calls on the resident matrix.  The held-out cells are `holdout` only, in the caller's numbering;
    the predictions are the distances between the positions, which must be finite.  At most four distinct `probs`
    apart from 0.5 (eight ranks per call)."""
    if not (0 < confidence_level < 1):
        raise ValueError("confidence_level must be between 0 and 1")
    probs = tuple(float(p) for p in probs)
    if handle is not None:
        if positions is None:
            raise ValueError("the device form needs positions")
        if input_dissimilarities is not None:
            raise ValueError("the device form takes the held-out cells as holdout picks")
        pos = np.asarray(positions, dtype=np.float64)
        if pos.ndim != 2 or pos.shape[0] != handle.n or not np.isfinite(pos).all():
            raise ValueError("positions must be a finite n x ndim matrix")
        picks = None if holdout is None else np.asarray(holdout, dtype=np.int64).reshape(-1)
        rep = handle.fit_report(pos, picks)

        def order_stats_of(series):
            def order_stats(ranks):
                if len(ranks) > _native.FIT_MAX_RANKS:
                    raise ValueError("the device form serves at most %d ranks per series" % _native.FIT_MAX_RANKS)
                vals, _ = handle.fit_order_stats(pos, series, ranks, picks)
                return vals
            return order_stats
        n_in, n_out = int(rep["in"]["count"]), int(rep["out"]["count"])
        return _assemble(rep, probs, order_stats_of, n_out, handle.n * handle.n, n_in + n_out, confidence_level,
                         seconds=list(rep["seconds"]))
    truth_m = coded_matrix(dissimilarity_matrix)
    if truth_m is None or predicted is None:
        raise ValueError("the host form needs the dissimilarity matrix and the predicted matrix")
    pred = np.asarray(predicted.to_numpy() if hasattr(predicted, "to_numpy") else predicted, dtype=np.float64)
    n = truth_m.values.shape[0]
    if truth_m.values.shape != (n, n) or pred.shape != (n, n):
        raise ValueError("All matrices must have the same dimensions")
    v_all, codes = truth_m.values, truth_m.codes
    held = _holdout_mask(n, input_dissimilarities, holdout)
    finite, has_pred = np.isfinite(v_all), ~np.isnan(pred)
    member = {"in": finite & (codes == 0) & ~held & has_pred, "out": finite & (codes == 0) & held & has_pred,
              "all": finite & has_pred}
    err = v_all - pred
    moments, sorted_errors = {}, {}
    for name, mask in member.items():
        e = err[mask]
        moments[name] = _host_moments(e, v_all[mask], pred[mask], with_vr=name == "all")
        sorted_errors[name] = np.sort(e)
    n_validation = int((finite & (codes == 0) & held).sum())
    return _assemble(moments, probs, lambda name: (lambda ranks: sorted_errors[name][list(ranks)]), n_validation,
                     int(has_pred.sum()), int((finite & (codes == 0)).sum()), confidence_level)


# --------------------------------------------------------------------------------------
# density.default
# --------------------------------------------------------------------------------------
def bw_nrd0(sd: float, iqr: float, n: int, first: float = 0.0) -> float:
    """stats::bw.nrd0 from the sample's sd (n - 1), interquartile range (type 7) and size:
    0.9 * min(sd, IQR / 1.34) * n^(-1/5).  R's fall-backs where that minimum is 0: sd, then |x[1]| (`first`: with sd = 0
    every value equals the first one), then 1."""
    if n < 2:
        raise ValueError("need at least 2 data points")
    lo = min(float(sd), float(iqr) / 1.34)
    if not lo:
        lo = float(sd) or abs(float(first)) or 1.0
    return 0.9 * lo * float(n) ** (-0.2)


def density_grid(xmin: float, xmax: float, bw: float, cut: float = 3.0):
    """density.default's ranges: (from, to, lo, up) = (min - cut bw, max + cut bw, from - 4 bw, to + 4 bw).  The density
    is returned on [from, to]; the masses are binned on [lo, up]."""
    from_, to = xmin - cut * bw, xmax + cut * bw
    return from_, to, from_ - 4.0 * bw, to + 4.0 * bw


def linear_bin_counts(x, lo: float, up: float, m: int):
    """The host twin of topolow_layout_prep_fit_linear_bins: (count int64[m], frac uint64[m], outside) of the values x.
    delta = (up - lo) / (m - 1), xpos = (x - lo) / delta, ix = floor(xpos), fx = xpos - ix; for 0 <= ix <= m - 2 a value
    adds 1 to count[ix] and (uint64)(fx * 2^32) to frac[ix]; every other value is outside.  IEEE f64 throughout, as on
    the device: the integers are the same."""
    x = np.asarray(x, dtype=np.float64).ravel()
    m = int(m)
    if not (2 <= m <= _native.FIT_MAX_GRID) or not (math.isfinite(lo) and math.isfinite(up) and lo < up):
        raise ValueError("2 <= m <= %d and finite lo < up are required" % _native.FIT_MAX_GRID)
    delta = (float(up) - float(lo)) / float(m - 1)
    xpos = (x - float(lo)) / delta
    fl = np.floor(xpos)
    ok = (fl >= 0.0) & (fl <= float(m - 2))
    ix = fl[ok].astype(np.int64)
    q = ((xpos[ok] - fl[ok]) * 4294967296.0).astype(np.uint64)
    count = np.bincount(ix, minlength=m).astype(np.int64)
    # exact in f64: each half is below 2^16 and there are fewer than 2^32 values
    hi = np.bincount(ix, weights=(q >> np.uint64(16)).astype(np.float64), minlength=m).astype(np.uint64)
    low = np.bincount(ix, weights=(q & np.uint64(0xFFFF)).astype(np.float64), minlength=m).astype(np.uint64)
    return count, (hi << np.uint64(16)) + low, int(x.size - ix.size)


def linear_bin_masses(count, frac) -> np.ndarray:
    """mass[g] = (count[g] - S[g]) + S[g - 1] with S = frac * 2^-32: what R's BinDist puts on grid point g (times N).
    DEVIATION from BinDist: fx is quantised to 2^-32, which moves a value's mass by at most 2^-32 of itself."""
    count = np.asarray(count, dtype=np.float64)
    s = np.asarray(frac, dtype=np.uint64).astype(np.float64) * 2.0 ** -32
    mass = count - s
    mass[1:] += s[:-1]
    return mass


@dataclass
class Density:
    """density.default's result: y at the n points x over [from, to], and the bandwidth."""
    x: np.ndarray
    y: np.ndarray
    bw: float
    n: int               # the values behind it


def density_default(x=None, *, binned=None, bw: Optional[float] = None, xmin: Optional[float] = None,
                    xmax: Optional[float] = None, n: int = 512, cut: float = 3.0) -> Density:
    """stats::density.default with its defaults (bw = "nrd0", n = 512, cut = 3, Gaussian kernel), restated.

    Either the raw values `x` (bw, xmin, xmax taken from them where not given), or `binned=(count, frac, lo, up, total)`
    as topolow_layout_prep_fit_linear_bins returns them, with `bw`, `xmin` and `xmax` of the values -- lo and up must be
    density_grid(xmin, xmax, bw, cut)'s.  Both go through the same quantised masses (linear_bin_counts,
    linear_bin_masses): the raw form is the specification of the binned one.

    The steps: from = min - cut bw, to = max + cut bw, lo = from - 4 bw, up = to + 4 bw; the masses / total on the
    n-point grid over [lo, up], zero-padded to 2 n; kords = seq(0, 2 (up - lo), length 2 n) with its upper half
    mirrored negative; dnorm(kords, sd = bw); pmax(0, Re(ifft(fft(y) conj(fft(kords))))[1:n]); linear interpolation
    from the grid onto seq(from, to, length n).  n above 512 is rounded up to a power of two for the grid, as R does.
    DEVIATION: the 2^-32 quantisation of linear_bin_masses."""
    n_out = int(n)
    grid = max(n_out, 512)
    if grid > 512:
        grid = 1 << int(math.ceil(math.log2(grid)))
    if binned is None:
        xs = np.asarray(x, dtype=np.float64).ravel()
        if xs.size < 2 or not np.isfinite(xs).all():
            raise ValueError("need at least 2 finite data points")
        if bw is None:
            srt = np.sort(xs)
            q = type7_quantiles(xs.size, (0.25, 0.75), lambda ranks: srt[list(ranks)])
            bw = bw_nrd0(float(np.std(xs, ddof=1)), float(q[1] - q[0]), xs.size, float(xs[0]))
        xmin = float(xs.min()) if xmin is None else xmin
        xmax = float(xs.max()) if xmax is None else xmax
    elif bw is None or xmin is None or xmax is None:
        raise ValueError("the binned form needs bw, xmin and xmax")
    bw = float(bw)
    if not (bw > 0.0 and math.isfinite(bw)):
        raise ValueError("'bw' is not positive.")
    from_, to, lo, up = density_grid(float(xmin), float(xmax), bw, cut)
    if binned is None:
        count, frac, _ = linear_bin_counts(xs, lo, up, grid)
        total = xs.size
    else:
        count, frac, blo, bup, total = binned
        if float(blo) != lo or float(bup) != up or len(count) != grid or len(frac) != grid:
            raise ValueError("the bins were not made on density_grid(xmin, xmax, bw, cut)'s lo and up with the grid's size")
    y = np.zeros(2 * grid)
    y[:grid] = linear_bin_masses(count, frac) / float(total)
    kords = np.linspace(0.0, 2.0 * (up - lo), 2 * grid)
    kords[grid + 1:] = -kords[grid - 1:0:-1]
    kords = np.exp(-0.5 * (kords / bw) ** 2) / (bw * math.sqrt(2.0 * math.pi))
    conv = np.maximum(0.0, np.fft.ifft(np.fft.fft(y) * np.conj(np.fft.fft(kords))).real[:grid])
    xout = np.linspace(from_, to, n_out)
    return Density(x=xout, y=np.interp(xout, np.linspace(lo, up, grid), conv), bw=bw, n=int(total))


# --------------------------------------------------------------------------------------
# the diagnostic plots' clouds, binned
# --------------------------------------------------------------------------------------
def _bin_of(x: np.ndarray, edges: np.ndarray) -> np.ndarray:
    """np.histogram's rule with explicit edges: k with edges[k] <= x < edges[k + 1], the last bin closed above; -1
    outside.  Found by comparing against the edges, as on the device."""
    nb = edges.size - 1
    k = np.searchsorted(edges, x, side="right") - 1
    k[x == edges[-1]] = nb - 1
    k[(k < 0) | (k >= nb)] = -1
    return k


def bin_counts_2d(x, y, x_edges, y_edges):
    """The host twin of topolow_layout_prep_fit_hist2d: (counts int64[nx, ny], outside)."""
    xe, ye = np.asarray(x_edges, dtype=np.float64), np.asarray(y_edges, dtype=np.float64)
    for e in (xe, ye):
        if e.ndim != 1 or e.size < 2 or not np.isfinite(e).all() or not (np.diff(e) > 0).all():
            raise ValueError("edges must be finite and strictly increasing")
    nx, ny = xe.size - 1, ye.size - 1
    if nx * ny > _native.FIT_MAX_BINS:
        raise ValueError("at most %d bins" % _native.FIT_MAX_BINS)
    kx = _bin_of(np.asarray(x, dtype=np.float64).ravel(), xe)
    ky = _bin_of(np.asarray(y, dtype=np.float64).ravel(), ye)
    inside = (kx >= 0) & (ky >= 0)
    counts = np.bincount(kx[inside] * ny + ky[inside], minlength=nx * ny).astype(np.int64).reshape(nx, ny)
    return counts, int(kx.size - inside.sum())


@dataclass
class BinnedCloud:
    """A point cloud as exact 2-D bin counts: counts[kx, ky] over x_edges x y_edges (np.histogram2d's rule), the points
    outside the edges, and the cloud's size n = counts.sum() + outside."""
    x_axis: str
    y_axis: str
    x_edges: np.ndarray
    y_edges: np.ndarray
    counts: np.ndarray
    outside: int
    n: int

    def conditional_quantiles(self, probs=(0.5,)) -> np.ndarray:
        """[len(probs), nx]: per x-bin the y at which the cumulative count over the y-bins reaches p * c (c the x-bin's
        count), linear inside the y-bin that reaches it; NaN for an empty x-bin.  p = 0 gives the lower edge of the
        first y-bin that holds a point, p = 1 the upper edge of the last.
        This is the trend line of the plots.  DEVIATION: it replaces the reference's `loess` and `geom_smooth` curves
        deliberately -- a loess over the 3 * 10^7 points of a large map is not something R finishes either, and the
        points do not exist here; a conditional median read off the exact counts does the plot's job."""
        probs = [float(p) for p in probs]
        if any(not (0.0 <= p <= 1.0) for p in probs):
            raise ValueError("probs must lie in [0, 1]")
        nx = self.counts.shape[0]
        out = np.full((len(probs), nx), np.nan)
        for kx in range(nx):
            row = self.counts[kx]
            c = int(row.sum())
            if c == 0:
                continue
            cum = np.cumsum(row)
            filled = np.flatnonzero(row)
            for q, p in enumerate(probs):
                t = p * c
                ky = int(filled[np.searchsorted(cum[filled], t, side="left")]) if t <= cum[filled[-1]] else int(filled[-1])
                before = float(cum[ky] - row[ky])
                out[q, kx] = self.y_edges[ky] + (t - before) / float(row[ky]) * (self.y_edges[ky + 1] - self.y_edges[ky])
        return out


@dataclass
class EmbeddingQualityData:
    series: str
    n: int                              # the series' cells
    scatter: BinnedCloud                # true x predicted
    residual_vs_true: BinnedCloud       # true x (predicted - true)
    residual_vs_fitted: BinnedCloud     # predicted x (true - predicted)
    residual_density: Optional[Density]   # of predicted - true; None for fewer than 2 cells
    statistics: FitStatistics


def _plot_edges(lo: float, hi: float, bins: int) -> np.ndarray:
    """bins + 1 edges from lo to hi; a range without width (or none: an empty series) gets one of width 1 around it."""
    if not (math.isfinite(lo) and math.isfinite(hi)):
        lo, hi = 0.0, 1.0
    if not hi > lo:
        lo, hi = lo - 0.5, hi + 0.5
    return np.linspace(lo, hi, int(bins) + 1)


def embedding_quality_data(dissimilarity_matrix=None, predicted=None, *, positions=None,
                           handle: Optional["_native.PreparedHandle"] = None, holdout=None, series="all", bins=(64, 64),
                           confidence_level=0.95) -> EmbeddingQualityData:
    """The data behind the reference's three diagnostic plots of a fit -- `scatterplot_fitted_vs_true`
    (R/visualization.R:2616-2701: predicted against true, residual against fitted) and `plot_embedding_quality`
    (R/diagnostics.R:128-183: estimated against input, residual against input, the density of the residuals) -- without
    the point clouds: exact 2-D bin counts (BinnedCloud; its conditional_quantiles are the trend line, which replaces
    the plots' loess / geom_smooth, see there), the residual density as density.default computes it (density_default),
    and the FitStatistics the plots' titles and lines come from (fit_statistics, unchanged).

    `series`: "in", "out" or "all", as fit_statistics (see the module's text).  The diagonal counts, as in the fit
    report.  DEVIATION: `plot_embedding_quality` masks the diagonal; here it is a cell like any other (a diagonal of
    zeros adds n points at the origin of the scatter).  +-Inf cells are in no series.
    `bins`: (x bins, y bins) of every cloud, at most 8192 together.  Default edges: np.linspace from 0 (or the minimum,
    where that is negative) to the series' maximum on the true and predicted axes, as the plots' limits; from the
    minimum to the maximum on the residual axes.

    Host form (no `handle`): `predicted` is the n x n matrix of predicted dissimilarities, `holdout` picks as in
    fit_statistics.  NumPy on n x n temporaries; this form is the specification.
    Device form (`handle=` and `positions=`, as fit_statistics): fit_statistics as it is, one fit_extent, one
    fit_order_stats (the quartiles of the bandwidth), three fit_hist2d and one fit_linear_bins on the resident matrix;
    nothing of size n x n reaches the host.  All counts equal the host form's; so does the density wherever the
    bandwidth does: the sd behind it comes from FitStatistics, whose sums differ between the forms in their last bits,
    and enters the bandwidth rounded to float32 so that those bits do not move the grid."""
    if series not in ("in", "out", "all"):
        raise ValueError('series must be "in", "out" or "all"')
    bx, by = (int(b) for b in bins)
    if bx < 1 or by < 1 or bx * by > _native.FIT_MAX_BINS:
        raise ValueError("bins must be at least 1 x 1 and at most %d together" % _native.FIT_MAX_BINS)
    if handle is not None:
        stats = fit_statistics(None, handle=handle, positions=positions, holdout=holdout, confidence_level=confidence_level)
        pos = np.asarray(positions, dtype=np.float64)
        picks = None if holdout is None else np.asarray(holdout, dtype=np.int64).reshape(-1)
        extent, m = handle.fit_extent(pos, series, picks)

        def hist2d(xa, xe, ya, ye):
            counts, outside, _ = handle.fit_hist2d(pos, series, xa, xe, ya, ye, picks)
            return counts, outside

        def order_stats(ranks):
            return handle.fit_order_stats(pos, series, ranks, picks)[0]

        def linear_bins(lo, up, grid):
            count, frac, _, total = handle.fit_linear_bins(pos, series, "residual", lo, up, grid, picks)
            return count, frac, lo, up, total
    else:
        stats = fit_statistics(dissimilarity_matrix, predicted, holdout=holdout, confidence_level=confidence_level)
        truth_m = coded_matrix(dissimilarity_matrix)
        pred = np.asarray(predicted.to_numpy() if hasattr(predicted, "to_numpy") else predicted, dtype=np.float64)
        n = truth_m.values.shape[0]
        held = _holdout_mask(n, None, holdout)
        finite, plain = np.isfinite(truth_m.values) & ~np.isnan(pred), truth_m.codes == 0
        mask = {"in": finite & plain & ~held, "out": finite & plain & held, "all": finite}[series]
        v, r = truth_m.values[mask], pred[mask]
        axes = {"true": v, "predicted": r, "error": v - r, "residual": r - v}
        m = int(v.size)
        extent = {k: (float(a.min()), float(a.max())) if m else (math.nan, math.nan) for k, a in axes.items()}
        sorted_e = np.sort(axes["error"])

        def hist2d(xa, xe, ya, ye):
            return bin_counts_2d(axes[xa], axes[ya], xe, ye)

        def order_stats(ranks):
            return sorted_e[list(ranks)]

        def linear_bins(lo, up, grid):
            count, frac, _ = linear_bin_counts(axes["residual"], lo, up, grid)
            return count, frac, lo, up, m

    def edges_from_zero(axis, k):
        return _plot_edges(min(0.0, extent[axis][0]) if m else math.nan, extent[axis][1], k)

    def cloud(xa, xe, ya, ye):
        counts, outside = hist2d(xa, xe, ya, ye)
        return BinnedCloud(xa, ya, xe, ye, counts, outside, m)

    true_x, fitted_x = edges_from_zero("true", bx), edges_from_zero("predicted", bx)
    scatter = cloud("true", true_x, "predicted", edges_from_zero("predicted", by))
    res_true = cloud("true", true_x, "residual", _plot_edges(*extent["residual"], by))
    res_fitted = cloud("predicted", fitted_x, "error", _plot_edges(*extent["error"], by))
    density = None
    if m >= 2:
        sd = {"in": stats.in_sample.sd, "out": stats.out_sample.sd, "all": stats.residual_sd}[series]
        q = type7_quantiles(m, (0.25, 0.75), order_stats)      # of v - r; r - v has the same interquartile range
        rmin, rmax = extent["residual"]
        bw = bw_nrd0(float(np.float32(sd)), float(q[1] - q[0]), m, rmin)
        _, _, lo, up = density_grid(rmin, rmax, bw)
        density = density_default(binned=linear_bins(lo, up, 512), bw=bw, xmin=rmin, xmax=rmax)
    return EmbeddingQualityData(series=series, n=m, scatter=scatter, residual_vs_true=res_true,
                                residual_vs_fitted=res_fitted, residual_density=density, statistics=stats)
