// topolow_amd/csrc/relax_fit.h -- the fit report of a resident embedding: the signed errors truth - distance of the
// handle's matrix against a set of positions, their moments per series and their exact order statistics (reference
// R/error_metrics.R:55-202, R/visualization.R:2626-2648; host pipeline: topolow_layout_prep_fit_report /
// _fit_order_stats in topolow_prep_fold.hip; the NumPy specification: topolow_amd/error_metrics.py, fit_statistics).
//
// As relax_post.h's resident kernel: BUFFER coordinates, one workgroup per LINE a of the handle's buffer, the matrix
// gathered through ord (nullable) -- cell (a, b) is B[ord[a] * n + ord[b]] -- so the source line is contiguous and the
// lanes gather inside it; 8-byte accesses, consecutive lanes on consecutive addresses for ord and the positions' rows.
//
// A cell belongs to zero or more of three series:
//   IN   its value is finite, its code is 0 and it is not held out
//   OUT  its value is finite, its code is 0 and it is held out (its bit of the fold mask is set)
//   ALL  its value is finite, whatever its code and whether held out or not (extract_numeric_values' rule)
// The diagonal counts.  NaN cells are NA; +-Inf cells are left out of every series, as post-metrics leaves them out
// (the reference would turn every statistic into Inf or NaN).
//
// No floating-point atomics: every sum is reduced in post_metrics_kernel's fixed order -- each lane over its indices in
// ascending order, the 64 lanes of a wave by a shuffle tree, the four waves in wave order -- into one partial per line;
// the host adds the lines in index order.  The histograms of the select are integer atomics.
//
// The cell function and the block reduction serve relax_fit_bins.h as well, whose kernels are another source's: that
// source defines TOPOLOW_FIT_CELL_ONLY and gets everything above the first kernel, and no kernel.
#pragma once

#include "relax_common.h"
#include "relax_prep_device.h"

namespace topolow {

constexpr int kFitThreads = 256;
constexpr int kFitWaves = kFitThreads / 64;
constexpr int kFitSeries = 3;      // TOPOLOW_FIT_IN, _OUT, _ALL
constexpr int kFitMaxRanks = 8;    // TOPOLOW_FIT_MAX_RANKS

// One cell of the ordered matrix against the positions.
struct FitCell {
  double r;      // ||p_a - p_b||: the bits of topolow_est_distances
  double v;      // the truth, as stored (threshold cells: the number behind the prefix)
  double e;      // v - r
  int code;      // 0, 1 (">"), -1 ("<")
  bool held;     // the fold bit of the SOURCE cell; false where no picks were given (mask == nullptr)
  __device__ bool in(int series) const {
    const bool finite = __builtin_isfinite(v);
    return series == 2 ? finite : finite && code == 0 && held == (series == 1);
  }
};

// The one place a cell is read and scored; all three kernels call it.
__device__ inline FitCell fit_cell(int a, int b, const double* __restrict__ pos, int n, int dim,
                                   const double* __restrict__ vals, const int8_t* __restrict__ codes,
                                   const int32_t* __restrict__ ord, const uint32_t* __restrict__ mask) {
  FitCell c;
  c.r = post_distance(pos + (size_t)a * dim, pos + (size_t)b * dim, dim);
  const size_t cell = (size_t)(ord != nullptr ? ord[a] : a) * (size_t)n + (size_t)(ord != nullptr ? ord[b] : b);
  c.v = vals[cell];
  c.code = codes != nullptr ? (int)codes[cell] : 0;
  c.held = mask != nullptr && fold_bit(mask, cell);
  c.e = c.v - c.r;
  return c;
}

struct FitAdd { template <typename T> __device__ T operator()(T x, T y) const { return x + y; } };
struct FitMin { __device__ double operator()(double x, double y) const { return ::fmin(x, y); } };
struct FitMax { __device__ double operator()(double x, double y) const { return ::fmax(x, y); } };

// x[0 .. K) of every lane -> the workgroup's K totals in thread 0, in the fixed order: shuffle tree over the wave, then
// the waves in wave order.  part: kFitWaves x K words of LDS of this call's own.
template <typename T, int K, typename Op>
__device__ inline void fit_block_reduce(T (&x)[K], T (*part)[K], Op op) {
  for (int k = 0; k < K; ++k)
    for (int off = 32; off > 0; off >>= 1) x[k] = op(x[k], (T)__shfl_down(x[k], off, 64));
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < K; ++k) part[wave][k] = x[k];
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 0; k < K; ++k) {
      T t = part[0][k];
      for (int w = 1; w < kFitWaves; ++w) t = op(t, part[w][k]);
      x[k] = t;
    }
}

#ifndef TOPOLOW_FIT_CELL_ONLY

// ---- pass 1: counts, sums, extremes -------------------------------------------------------------------------------
struct FitLineSums {   // one per line
  // [0 .. 3): sum e per series; [3 .. 6): sum |e|; [6 .. 8): sum p of IN, OUT; [8 .. 10): sum |p|; [10]: sum v of ALL;
  // [11]: sum r of ALL.  p = e / v * 100 over the cells with v > 0 (R/error_metrics.R:116-124).
  double sum[12];
  double min_e[kFitSeries], max_e[kFitSeries];   // +Inf / -Inf where the line holds no cell of the series
  uint32_t count[kFitSeries], pct_count[2], pad;
};

__global__ __launch_bounds__(kFitThreads) void fit_sums_kernel(
    const double* __restrict__ pos, int n, int dim, const double* __restrict__ vals, const int8_t* __restrict__ codes,
    const int32_t* __restrict__ ord, const uint32_t* __restrict__ mask, FitLineSums* __restrict__ lines) {
  __shared__ double part_sum[kFitWaves][12], part_min[kFitWaves][kFitSeries], part_max[kFitWaves][kFitSeries];
  __shared__ uint32_t part_cnt[kFitWaves][5];
  const int a = blockIdx.x;
  if (a >= n) return;
  double sum[12], mn[kFitSeries], mx[kFitSeries];
  uint32_t cnt[5] = {0, 0, 0, 0, 0};
  for (int k = 0; k < 12; ++k) sum[k] = 0.0;
  for (int s = 0; s < kFitSeries; ++s) { mn[s] = INFINITY; mx[s] = -INFINITY; }
  for (int b = threadIdx.x; b < n; b += kFitThreads) {
    const FitCell c = fit_cell(a, b, pos, n, dim, vals, codes, ord, mask);
    for (int s = 0; s < kFitSeries; ++s) {
      if (!c.in(s)) continue;
      ++cnt[s];
      sum[s] += c.e;
      sum[3 + s] += ::fabs(c.e);
      mn[s] = ::fmin(mn[s], c.e);
      mx[s] = ::fmax(mx[s], c.e);
      if (s < 2 && c.v > 0.0) {
        const double p = c.e / c.v * 100.0;
        ++cnt[3 + s];
        sum[6 + s] += p;
        sum[8 + s] += ::fabs(p);
      }
      if (s == 2) {
        sum[10] += c.v;
        sum[11] += c.r;
      }
    }
  }
  fit_block_reduce(sum, part_sum, FitAdd());
  fit_block_reduce(mn, part_min, FitMin());
  fit_block_reduce(mx, part_max, FitMax());
  fit_block_reduce(cnt, part_cnt, FitAdd());
  if (threadIdx.x == 0) {
    FitLineSums& o = lines[a];
    for (int k = 0; k < 12; ++k) o.sum[k] = sum[k];
    for (int s = 0; s < kFitSeries; ++s) { o.min_e[s] = mn[s]; o.max_e[s] = mx[s]; o.count[s] = cnt[s]; }
    o.pct_count[0] = cnt[3];
    o.pct_count[1] = cnt[4];
    o.pad = 0;
  }
}

// ---- pass 2: sums about the means the host formed from pass 1's totals ---------------------------------------------
struct FitMeans { double e[kFitSeries], v, r; };   // v, r: of ALL

struct FitLineCentred {   // one per line
  // [0 .. 3): sum (e - mean e)^2 per series; of ALL: [3] sum (v - mean v)^2, [4] sum (r - mean r)^2,
  // [5] sum (v - mean v)(r - mean r)
  double css[6];
};

__global__ __launch_bounds__(kFitThreads) void fit_centred_kernel(
    const double* __restrict__ pos, int n, int dim, const double* __restrict__ vals, const int8_t* __restrict__ codes,
    const int32_t* __restrict__ ord, const uint32_t* __restrict__ mask, FitMeans means,
    FitLineCentred* __restrict__ lines) {
  __shared__ double part[kFitWaves][6];
  const int a = blockIdx.x;
  if (a >= n) return;
  double css[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < n; b += kFitThreads) {
    const FitCell c = fit_cell(a, b, pos, n, dim, vals, codes, ord, mask);
    for (int s = 0; s < kFitSeries; ++s) {
      if (!c.in(s)) continue;
      const double de = c.e - means.e[s];
      css[s] += de * de;
      if (s == 2) {
        const double dv = c.v - means.v, dr = c.r - means.r;
        css[3] += dv * dv;
        css[4] += dr * dr;
        css[5] += dv * dr;
      }
    }
  }
  fit_block_reduce(css, part, FitAdd());
  if (threadIdx.x == 0)
    for (int k = 0; k < 6; ++k) lines[a].css[k] = css[k];
}

// ---- exact order statistics: one pass of a radix select over prep_order_key(e) of one series ----------------------
// spec_select_kernel's pattern for up to kFitMaxRanks ranks at once: the digit (key >> shift) & 255 of every error of
// the series whose key agrees with prefix[r] in the bits above the digit goes to hist[r]; shift = 56 (no bits above:
// every error of the series counts, so hist[0] adds up to the series' count), 48, ..., 0.  Counts go to LDS first, one
// global integer add per (workgroup, rank, digit) that is not 0.  The errors are recomputed from fit_cell in every pass.
struct FitSelect {
  unsigned long long hist[kFitMaxRanks][256];
};
struct FitPrefixes { unsigned long long key[kFitMaxRanks]; };

__global__ __launch_bounds__(kFitThreads) void fit_select_kernel(
    const double* __restrict__ pos, int n, int dim, const double* __restrict__ vals, const int8_t* __restrict__ codes,
    const int32_t* __restrict__ ord, const uint32_t* __restrict__ mask, int series, int shift, int n_ranks,
    FitPrefixes prefixes, FitSelect* __restrict__ out) {
  __shared__ unsigned int h[kFitMaxRanks][256];
  __shared__ unsigned long long above_of[kFitMaxRanks];
  const int a = blockIdx.x;
  if (a >= n) return;
  const bool first = shift == 56;
  for (int r = 0; r < n_ranks; ++r) h[r][threadIdx.x] = 0;
  if ((int)threadIdx.x < n_ranks) above_of[threadIdx.x] = first ? 0ull : prefixes.key[threadIdx.x] >> (shift + 8);
  __syncthreads();
  for (int b = threadIdx.x; b < n; b += kFitThreads) {
    const FitCell c = fit_cell(a, b, pos, n, dim, vals, codes, ord, mask);
    if (!c.in(series)) continue;
    const unsigned long long key = prep_order_key(c.e);
    const unsigned int digit = (unsigned int)(key >> shift) & 255u;
    const unsigned long long above = first ? 0ull : key >> (shift + 8);
    for (int r = 0; r < n_ranks; ++r)
      if (above == above_of[r]) atomicAdd(&h[r][digit], 1u);
  }
  __syncthreads();
  for (int r = 0; r < n_ranks; ++r)
    if (h[r][threadIdx.x]) atomicAdd(&out->hist[r][threadIdx.x], (unsigned long long)h[r][threadIdx.x]);
}

#endif  // TOPOLOW_FIT_CELL_ONLY

}  // namespace topolow
