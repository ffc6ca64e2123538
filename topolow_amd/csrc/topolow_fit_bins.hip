// topolow_amd/csrc/topolow_fit_bins.hip -- the fit's binned diagnostics of libtopolow_relax.so (relax_fit_bins.h;
// reference R/visualization.R:2616-2701, R/diagnostics.R:128-183): the extent of a series, exact 2-D bin counts and
// the linear bins of density() from a prepared handle's resident matrix.  A source of its own, so that the fold source
// keeps its kernels to itself; arguments are checked and picks marked by the fit report's functions
// (fit_check_arguments, fit_check_series, fit_run: topolow_prep_fold.hip through topolow_prep.h).

#include "topolow_prep.h"
#define TOPOLOW_FIT_CELL_ONLY   // relax_fit.h: the cell function and the block reduction, not the report's kernels
#include "relax_fit_bins.h"

static_assert(kFitMaxBins == TOPOLOW_FIT_MAX_BINS && kFitMaxGrid == TOPOLOW_FIT_MAX_GRID &&
              TOPOLOW_FIT_AXIS_RESIDUAL == kFitAxes - 1, "relax_fit_bins.h and the header disagree");

namespace {

int fit_check_axis(const char* entry, const char* name, int32_t axis, char* errbuf, size_t errlen) {
  if (axis >= TOPOLOW_FIT_AXIS_TRUE && axis <= TOPOLOW_FIT_AXIS_RESIDUAL) return TOPOLOW_OK;
  set_err(errbuf, errlen, "%s: unknown %s %d (TOPOLOW_FIT_AXIS_TRUE, _PREDICTED, _ERROR or _RESIDUAL)", entry, name, axis);
  return TOPOLOW_ERR_BAD_ARGUMENT;
}

// edges[0 .. nb]: finite and strictly increasing
int fit_check_edges(const char* entry, const char* name, const double* edges, int32_t nb, char* errbuf, size_t errlen) {
  for (int k = 0; k <= nb; ++k) {
    if (std::isfinite(edges[k]) && (k == 0 || edges[k - 1] < edges[k])) continue;
    set_err(errbuf, errlen, "%s: %s must be finite and strictly increasing (entry %d)", entry, name, k);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  return TOPOLOW_OK;
}

}  // namespace

extern "C" {

int topolow_layout_prep_fit_extent(topolow_layout_prep* p, const double* positions, int32_t ndim, const int64_t* picks,
                                   int64_t n_picks, int32_t series, double* out, int64_t* count_out, char* errbuf,
                                   size_t errlen) {
  const char* entry = "topolow_layout_prep_fit_extent";
  if (const int rca = fit_check_arguments(entry, p, positions, ndim, picks, n_picks, out && count_out ? (const void*)out : nullptr,
                                          errbuf, errlen))
    return rca;
  if (const int rcs = fit_check_series(entry, series, errbuf, errlen)) return rcs;
  if (const int rcu = prep_check_usable(p, errbuf, errlen)) return rcu;
  return fit_run(p, positions, ndim, picks, n_picks, errbuf, errlen, [&](const FitInputs& in) {
    const int n = p->n;
    const size_t N = (size_t)n;
    DevBuf<FitLineExtent> dlines;
    prep_alloc(dlines, N, "the lines' extents");
    std::vector<FitLineExtent> le(N);
    hipLaunchKernelGGL(bins_extent_kernel, dim3(n), dim3(kFitThreads), 0, in.stream, in.pos, n, ndim, in.vals, in.codes,
                       in.ord, in.mask, series, dlines.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(le.data(), dlines.p, N * sizeof(FitLineExtent), hipMemcpyDeviceToHost, in.stream));
    HIP_TRY(hipStreamSynchronize(in.stream));
    double mn[kFitAxes], mx[kFitAxes];
    int64_t count = 0;
    for (int k = 0; k < kFitAxes; ++k) { mn[k] = INFINITY; mx[k] = -INFINITY; }
    for (size_t a = 0; a < N; ++a) {
      count += le[a].count;
      for (int k = 0; k < kFitAxes; ++k) {
        mn[k] = std::fmin(mn[k], le[a].mn[k]);
        mx[k] = std::fmax(mx[k], le[a].mx[k]);
      }
    }
    for (int k = 0; k < kFitAxes; ++k) {
      out[2 * k] = count ? mn[k] : NAN;
      out[2 * k + 1] = count ? mx[k] : NAN;
    }
    *count_out = count;
  });
}

int topolow_layout_prep_fit_hist2d(topolow_layout_prep* p, const double* positions, int32_t ndim, const int64_t* picks,
                                   int64_t n_picks, int32_t series, int32_t x_axis, const double* x_edges, int32_t nx,
                                   int32_t y_axis, const double* y_edges, int32_t ny, int64_t* counts_out,
                                   int64_t* outside_out, int64_t* count_out, char* errbuf, size_t errlen) {
  const char* entry = "topolow_layout_prep_fit_hist2d";
  if (const int rca = fit_check_arguments(entry, p, positions, ndim, picks, n_picks,
                                          x_edges && y_edges && counts_out && outside_out && count_out ? (const void*)counts_out : nullptr,
                                          errbuf, errlen))
    return rca;
  if (const int rcs = fit_check_series(entry, series, errbuf, errlen)) return rcs;
  if (const int rcx = fit_check_axis(entry, "x_axis", x_axis, errbuf, errlen)) return rcx;
  if (const int rcy = fit_check_axis(entry, "y_axis", y_axis, errbuf, errlen)) return rcy;
  if (nx < 1 || ny < 1 || (int64_t)nx * ny > TOPOLOW_FIT_MAX_BINS) {
    set_err(errbuf, errlen, "%s: nx >= 1, ny >= 1 and nx * ny <= %d are required (got %d x %d)", entry,
            TOPOLOW_FIT_MAX_BINS, nx, ny);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (const int rce = fit_check_edges(entry, "x_edges", x_edges, nx, errbuf, errlen)) return rce;
  if (const int rce = fit_check_edges(entry, "y_edges", y_edges, ny, errbuf, errlen)) return rce;
  if (const int rcu = prep_check_usable(p, errbuf, errlen)) return rcu;
  return fit_run(p, positions, ndim, picks, n_picks, errbuf, errlen, [&](const FitInputs& in) {
    const int n = p->n;
    const size_t bins = (size_t)nx * ny, n_edges = (size_t)nx + ny + 2, lds = fit_hist2d_lds(nx, ny);
    std::vector<double> edges(x_edges, x_edges + nx + 1);
    edges.insert(edges.end(), y_edges, y_edges + ny + 1);
    std::vector<unsigned long long> got(bins + 2);
    DevBuf<double> dedges;
    DevBuf<unsigned long long> dout;
    prep_alloc(dedges, n_edges, "the bin edges");
    prep_alloc(dout, bins + 2, "the bin counts");
    HIP_TRY(hipMemcpyAsync(dedges.p, edges.data(), n_edges * 8, hipMemcpyHostToDevice, in.stream));
    HIP_TRY(hipMemsetAsync(dout.p, 0, (bins + 2) * 8, in.stream));
    if (lds > 64 * 1024)
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&bins_hist2d_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(bins_hist2d_kernel, dim3(n), dim3(kFitThreads), lds, in.stream, in.pos, n, ndim, in.vals, in.codes,
                       in.ord, in.mask, series, x_axis, y_axis, dedges.p, nx, ny, dout.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(got.data(), dout.p, (bins + 2) * 8, hipMemcpyDeviceToHost, in.stream));
    HIP_TRY(hipStreamSynchronize(in.stream));
    for (size_t q = 0; q < bins; ++q) counts_out[q] = (int64_t)got[q];
    *outside_out = (int64_t)got[bins];
    *count_out = (int64_t)got[bins + 1];
  });
}

int topolow_layout_prep_fit_linear_bins(topolow_layout_prep* p, const double* positions, int32_t ndim,
                                        const int64_t* picks, int64_t n_picks, int32_t series, int32_t axis, double lo,
                                        double up, int32_t m, int64_t* count_out, uint64_t* frac_out,
                                        int64_t* outside_out, int64_t* total_out, char* errbuf, size_t errlen) {
  const char* entry = "topolow_layout_prep_fit_linear_bins";
  if (const int rca = fit_check_arguments(entry, p, positions, ndim, picks, n_picks,
                                          count_out && frac_out && outside_out && total_out ? (const void*)count_out : nullptr,
                                          errbuf, errlen))
    return rca;
  if (const int rcs = fit_check_series(entry, series, errbuf, errlen)) return rcs;
  if (const int rcx = fit_check_axis(entry, "axis", axis, errbuf, errlen)) return rcx;
  if (m < 2 || m > TOPOLOW_FIT_MAX_GRID) {
    set_err(errbuf, errlen, "%s: 2 <= m <= %d is required (got %d)", entry, TOPOLOW_FIT_MAX_GRID, m);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (!std::isfinite(lo) || !std::isfinite(up) || !(lo < up)) {
    set_err(errbuf, errlen, "%s: lo < up, both finite, is required (got %g, %g)", entry, lo, up);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  const double delta = (up - lo) / (double)(m - 1);
  if (!std::isfinite(delta) || !(delta > 0.0)) {
    set_err(errbuf, errlen, "%s: (up - lo) / (m - 1) must be finite and positive (got %g)", entry, delta);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (const int rcu = prep_check_usable(p, errbuf, errlen)) return rcu;
  if ((int64_t)p->n * p->n >= ((int64_t)1 << 32)) {
    set_err(errbuf, errlen, "%s: n * n < 2^32 is required, so that a bin's fraction sum fits 64 bits (n = %d)", entry, p->n);
    return TOPOLOW_ERR_UNSUPPORTED;
  }
  return fit_run(p, positions, ndim, picks, n_picks, errbuf, errlen, [&](const FitInputs& in) {
    const int n = p->n;
    const size_t M = (size_t)m;
    std::vector<unsigned long long> got(2 * M + 2);
    DevBuf<unsigned long long> dout;
    prep_alloc(dout, 2 * M + 2, "the linear bins");
    HIP_TRY(hipMemsetAsync(dout.p, 0, (2 * M + 2) * 8, in.stream));
    hipLaunchKernelGGL(bins_linear_kernel, dim3(n), dim3(kFitThreads), fit_linear_lds(m), in.stream, in.pos, n, ndim,
                       in.vals, in.codes, in.ord, in.mask, series, axis, lo, delta, m, dout.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(got.data(), dout.p, (2 * M + 2) * 8, hipMemcpyDeviceToHost, in.stream));
    HIP_TRY(hipStreamSynchronize(in.stream));
    for (size_t q = 0; q < M; ++q) {
      count_out[q] = (int64_t)got[q];
      frac_out[q] = (uint64_t)got[M + q];
    }
    *outside_out = (int64_t)got[2 * M];
    *total_out = (int64_t)got[2 * M + 1];
  });
}

}  // extern "C"
