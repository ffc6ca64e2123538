// topolow_amd/csrc/relax_fit_bins.h -- the point clouds of the fit's diagnostic plots without the points: the extent of
// a series, exact 2-D bin counts over explicit edges, and the mass distribution of density()'s linear binning
// (reference R/visualization.R:2616-2701 scatterplot_fitted_vs_true, R/diagnostics.R:128-183 plot_embedding_quality;
// host pipeline: topolow_layout_prep_fit_extent / _fit_hist2d / _fit_linear_bins in topolow_fit_bins.hip; the NumPy
// specification: topolow_amd/error_metrics.py, embedding_quality_data).
//
// As relax_fit.h: one workgroup per LINE of the handle's buffer, every cell read and scored by fit_cell, the series by
// FitCell::in.  A cell offers four quantities (TOPOLOW_FIT_AXIS_*): v, r, v - r, r - v.
//
// The kernels are a source's of their own (topolow_fit_bins.hip), so they are bins_*, not fit_*: the fit_* kernels are
// topolow_prep_fold.hip's.  That source defines TOPOLOW_FIT_CELL_ONLY before it includes this header, and relax_fit.h
// then gives the cell function and the block reduction without its kernels: each kernel is compiled exactly once.
//
// Counters live in LDS (u32: a line has fewer than 2^32 cells; the fraction sums u64) and are flushed with one global
// 64-bit integer add per counter that is not 0, into a buffer the host zeroed.  Integer atomics only: the results do not
// depend on any order.  The cells outside the bins and the series' count are kept per lane, added over the wave by a
// shuffle tree and flushed once per wave.
#pragma once

#include "relax_fit.h"

namespace topolow {

constexpr int kFitAxes = 4;         // TOPOLOW_FIT_AXIS_TRUE, _PREDICTED, _ERROR, _RESIDUAL
constexpr int kFitMaxBins = 8192;   // TOPOLOW_FIT_MAX_BINS
constexpr int kFitMaxGrid = 4096;   // TOPOLOW_FIT_MAX_GRID

__device__ inline double fit_axis(const FitCell& c, int axis) {
  return axis == 0 ? c.v : axis == 1 ? c.r : axis == 2 ? c.e : c.r - c.v;
}

// x[0 .. K) of every lane added over the wave; lane 0 adds what is not 0 to out[0 .. K).
template <int K>
__device__ inline void fit_wave_flush(unsigned int (&x)[K], unsigned long long* __restrict__ out) {
  for (int k = 0; k < K; ++k)
    for (int off = 32; off > 0; off >>= 1) x[k] += __shfl_down(x[k], off, 64);
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < K; ++k)
      if (x[k]) atomicAdd(&out[k], (unsigned long long)x[k]);
}

// ---- the extent: min and max of the four quantities over one series ------------------------------------------------
struct FitLineExtent {   // one per line
  double mn[kFitAxes], mx[kFitAxes];   // +Inf / -Inf where the line holds no cell of the series
  uint32_t count, pad;
};

__global__ __launch_bounds__(kFitThreads) void bins_extent_kernel(
    const double* __restrict__ pos, int n, int dim, const double* __restrict__ vals, const int8_t* __restrict__ codes,
    const int32_t* __restrict__ ord, const uint32_t* __restrict__ mask, int series, FitLineExtent* __restrict__ lines) {
  __shared__ double part_min[kFitWaves][kFitAxes], part_max[kFitWaves][kFitAxes];
  __shared__ uint32_t part_cnt[kFitWaves][1];
  const int a = blockIdx.x;
  if (a >= n) return;
  double mn[kFitAxes], mx[kFitAxes];
  uint32_t cnt[1] = {0};
  for (int k = 0; k < kFitAxes; ++k) { mn[k] = INFINITY; mx[k] = -INFINITY; }
  for (int b = threadIdx.x; b < n; b += kFitThreads) {
    const FitCell c = fit_cell(a, b, pos, n, dim, vals, codes, ord, mask);
    if (!c.in(series)) continue;
    ++cnt[0];
    for (int k = 0; k < kFitAxes; ++k) {
      const double x = fit_axis(c, k);
      mn[k] = ::fmin(mn[k], x);
      mx[k] = ::fmax(mx[k], x);
    }
  }
  fit_block_reduce(mn, part_min, FitMin());
  fit_block_reduce(mx, part_max, FitMax());
  fit_block_reduce(cnt, part_cnt, FitAdd());
  if (threadIdx.x == 0) {
    FitLineExtent& o = lines[a];
    for (int k = 0; k < kFitAxes; ++k) { o.mn[k] = mn[k]; o.mx[k] = mx[k]; }
    o.count = cnt[0];
    o.pad = 0;
  }
}

// ---- 2-D bin counts over explicit edges ----------------------------------------------------------------------------
// The bin of x among edges[0 .. nb]: k with edges[k] <= x < edges[k + 1], the last bin closed above (NumPy's
// histogram rule); -1 outside.  Found by comparing against the edges themselves: the number of edges <= x, by bisection.
__device__ inline int fit_bin_of(const double* edges, int nb, double x) {
  int lo = 0, hi = nb + 1;   // the count of edges <= x lies in [lo, hi]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (edges[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  if (lo == 0) return -1;                                // below the first edge (or NaN)
  if (lo == nb + 1) return x == edges[nb] ? nb - 1 : -1;   // the last edge itself, or above it
  return lo - 1;
}

constexpr size_t fit_hist2d_lds(int nx, int ny) { return (size_t)(nx + ny + 2) * 8 + (size_t)nx * (size_t)ny * 4; }

// edges: x_edges[0 .. nx] then y_edges[0 .. ny] (device).  out: nx * ny counts (y fastest), then [outside, count].
// Dynamic LDS: fit_hist2d_lds(nx, ny) bytes -- the edges, then the counters.
__global__ __launch_bounds__(kFitThreads) void bins_hist2d_kernel(
    const double* __restrict__ pos, int n, int dim, const double* __restrict__ vals, const int8_t* __restrict__ codes,
    const int32_t* __restrict__ ord, const uint32_t* __restrict__ mask, int series, int x_axis, int y_axis,
    const double* __restrict__ edges, int nx, int ny, unsigned long long* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fit_smem[];
  double* ex = reinterpret_cast<double*>(fit_smem);
  double* ey = ex + nx + 1;
  unsigned int* h = reinterpret_cast<unsigned int*>(ey + ny + 1);
  const int a = blockIdx.x;
  if (a >= n) return;
  const int bins = nx * ny;
  for (int q = threadIdx.x; q < nx + ny + 2; q += kFitThreads) ex[q] = edges[q];
  for (int q = threadIdx.x; q < bins; q += kFitThreads) h[q] = 0;
  __syncthreads();
  unsigned int tail[2] = {0, 0};   // outside, count
  for (int b = threadIdx.x; b < n; b += kFitThreads) {
    const FitCell c = fit_cell(a, b, pos, n, dim, vals, codes, ord, mask);
    if (!c.in(series)) continue;
    ++tail[1];
    const int kx = fit_bin_of(ex, nx, fit_axis(c, x_axis)), ky = fit_bin_of(ey, ny, fit_axis(c, y_axis));
    if (kx < 0 || ky < 0) ++tail[0];
    else atomicAdd(&h[kx * ny + ky], 1u);
  }
  __syncthreads();
  for (int q = threadIdx.x; q < bins; q += kFitThreads)
    if (h[q]) atomicAdd(&out[q], (unsigned long long)h[q]);
  fit_wave_flush(tail, out + bins);
}

// ---- density()'s linear binning (R's BinDist), in integers -----------------------------------------------------------
// xpos = (x - lo) / delta, ix = floor(xpos), fx = xpos - ix; for 0 <= ix <= m - 2 the cell adds 1 to count[ix] and
// (uint64)(fx * 2^32) to frac[ix]; every other cell of the series is outside.  Plain IEEE f64 subtraction, division,
// floor and a product with a power of two -- nothing here may be contracted or reassociated: NumPy must get the same
// integers.
struct FitLinearBin { long long ix; unsigned long long q; };   // ix = -1: outside

__device__ inline FitLinearBin fit_linear_bin(double x, double lo, double delta, int m) {
#pragma clang fp contract(off)
  const double xpos = (x - lo) / delta;
  const double fl = ::floor(xpos);
  if (!(fl >= 0.0 && fl <= (double)(m - 2))) return {-1, 0ull};
  const double fx = xpos - fl;
  return {(long long)fl, (unsigned long long)(fx * 4294967296.0)};
}

constexpr size_t fit_linear_lds(int m) { return (size_t)m * 12; }

// out: m counts, m fraction sums, then [outside, total].  Dynamic LDS: fit_linear_lds(m) bytes -- the u64 sums first.
__global__ __launch_bounds__(kFitThreads) void bins_linear_kernel(
    const double* __restrict__ pos, int n, int dim, const double* __restrict__ vals, const int8_t* __restrict__ codes,
    const int32_t* __restrict__ ord, const uint32_t* __restrict__ mask, int series, int axis, double lo, double delta,
    int m, unsigned long long* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fit_smem[];
  unsigned long long* frac = reinterpret_cast<unsigned long long*>(fit_smem);
  unsigned int* count = reinterpret_cast<unsigned int*>(frac + m);
  const int a = blockIdx.x;
  if (a >= n) return;
  for (int q = threadIdx.x; q < m; q += kFitThreads) { frac[q] = 0ull; count[q] = 0u; }
  __syncthreads();
  unsigned int tail[2] = {0, 0};   // outside, total
  for (int b = threadIdx.x; b < n; b += kFitThreads) {
    const FitCell c = fit_cell(a, b, pos, n, dim, vals, codes, ord, mask);
    if (!c.in(series)) continue;
    ++tail[1];
    const FitLinearBin g = fit_linear_bin(fit_axis(c, axis), lo, delta, m);
    if (g.ix < 0) { ++tail[0]; continue; }
    atomicAdd(&count[g.ix], 1u);
    if (g.q) atomicAdd(&frac[g.ix], g.q);
  }
  __syncthreads();
  for (int q = threadIdx.x; q < m; q += kFitThreads) {
    if (count[q]) atomicAdd(&out[q], (unsigned long long)count[q]);
    if (frac[q]) atomicAdd(&out[m + q], frac[q]);
  }
  fit_wave_flush(tail, out + 2 * (size_t)m);
}

}  // namespace topolow
