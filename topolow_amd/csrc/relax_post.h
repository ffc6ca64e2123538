// topolow_amd/csrc/relax_post.h -- the post-metrics kernels: est_distances alone, and est_distances with the terms of
// mae in one pass (reference R/core.R:474-481; host pipelines: topolow_est_distances_rows, topolow_post_metrics in
// topolow_post.hip).  Plain __global__ functions: topolow_post.hip alone includes this header.
#pragma once

#include "relax_common.h"

namespace topolow {

constexpr int kPostThreads = 256;

// est_distances = as.matrix(dist(positions)) (reference R/core.R:474), f64, rows [row0, row0 + rows).
// positions: n x dim row-major f64; out: rows x n f64, row-major (the full matrix is symmetric, so
// R's column-major reading of an n x n result is the same matrix).
__global__ __launch_bounds__(kPostThreads) void pdist_kernel(const double* __restrict__ pos, int n, int dim, int row0,
                                                             int rows, double* __restrict__ out) {
  const int j = blockIdx.y * kPostThreads + threadIdx.x;   // grid: x = row of the block, y = 256-column group
  const int r = blockIdx.x;
  if (j >= n || r >= rows) return;
  const int i = row0 + r;
  double s = 0.0;
  for (int d = 0; d < dim; ++d) {
    const double dev = pos[(size_t)i * dim + d] - pos[(size_t)j * dim + d];
    s += dev * dev;
  }
  out[(size_t)r * n + j] = ::sqrt(s);
}

// One workgroup per column of a tile of columns [col0, col0 + cols) of the caller's column-major n x n matrices.
//   vals   cols x n f64: the tile of `values`, column after column (the caller's own layout)
//   codes  cols x n i32 or nullptr
//   est    cols x n f64 out or nullptr: est[c * n + i] = ||p_i - p_(col0 + c)||
//   col_sum / col_cnt   n entries each; this launch writes [col0, col0 + cols)
// Lane l of the workgroup walks rows l, l + 256, ...: 8-byte accesses, consecutive lanes on consecutive
// addresses.  The distance is pdist_kernel's own arithmetic (a sequential s += dev * dev over the coordinates,
// then ::sqrt), so est is bit-identical to topolow_est_distances.
// A column's partial is reduced in one fixed order -- each lane over its rows in ascending order, the 64 lanes
// of a wave by a shuffle tree, the four waves in wave order -- and belongs to the column alone: it does not
// depend on the tile the column arrived in, nor on whether est is written.  No atomics.
__global__ __launch_bounds__(kPostThreads) void post_metrics_kernel(
    const double* __restrict__ pos, int n, int dim, int col0, int cols, const double* __restrict__ vals,
    const int32_t* __restrict__ codes, double* __restrict__ est, double* __restrict__ col_sum,
    uint32_t* __restrict__ col_cnt) {
  __shared__ double wave_sum[kPostThreads / 64];
  __shared__ uint32_t wave_cnt[kPostThreads / 64];
  const int c = blockIdx.x;
  if (c >= cols) return;
  const int j = col0 + c;
  const size_t base = (size_t)c * (size_t)n;
  const double* pj = pos + (size_t)j * dim;
  double sum = 0.0;
  uint32_t cnt = 0;
  for (int i = threadIdx.x; i < n; i += kPostThreads) {
    const double r = post_distance(pj, pos + (size_t)i * dim, dim);
    if (est != nullptr) est[base + i] = r;
    const double v = vals[base + i];
    const bool counts = __builtin_isfinite(v) && (codes == nullptr || codes[base + i] == 0);
    if (counts) {
      sum += ::fabs(v - r);
      ++cnt;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    sum += __shfl_down(sum, off, 64);
    cnt += __shfl_down(cnt, off, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { wave_sum[wave] = sum; wave_cnt[wave] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = wave_sum[0];
    uint32_t k = wave_cnt[0];
    for (int w = 1; w < kPostThreads / 64; ++w) { t += wave_sum[w]; k += wave_cnt[w]; }
    col_sum[j] = t;
    col_cnt[j] = k;
  }
}

// The same pass over a matrix that is resident on the device (topolow_layout_prep_post_metrics): one workgroup per
// LINE of the handle's buffer -- line a holds B[a * n + b], b contiguous; a row of the matrix for a row-major handle,
// a column for a column-major one -- of the matrix gathered through ord (nullable: the input order was kept):
// cell (a, b) is B[ord[a] * n + ord[b]].  The source line ord[a] is contiguous and the lanes gather within it, as
// prep_dense_kernel does; ord itself and the est tile are read and written with consecutive lanes on consecutive
// addresses.
//   vals / codes   n x n f64 / int8 (codes nullable: all zero)
//   est            lines x n f64 out or nullptr: est[(a - line0) * n + b] = ||p_a - p_b||; the matrix is symmetric bit
//                  for bit, so the caller's layout does not show
//   line_sum / line_cnt   n entries each; this launch writes [line0, line0 + lines)
// The distance, the counting rule and the order of the reduction are post_metrics_kernel's, line for column: the
// partial of line a has the bits that kernel gives for column a of the matrix whose column a is this line.
__global__ __launch_bounds__(kPostThreads) void post_metrics_resident_kernel(
    const double* __restrict__ pos, int n, int dim, int line0, int lines, const double* __restrict__ vals,
    const int8_t* __restrict__ codes, const int32_t* __restrict__ ord, double* __restrict__ est,
    double* __restrict__ line_sum, uint32_t* __restrict__ line_cnt) {
  __shared__ double wave_sum[kPostThreads / 64];
  __shared__ uint32_t wave_cnt[kPostThreads / 64];
  const int c = blockIdx.x;
  if (c >= lines) return;
  const int j = line0 + c;
  const size_t base = (size_t)c * (size_t)n;
  const size_t src = (size_t)(ord != nullptr ? ord[j] : j) * (size_t)n;
  const double* pj = pos + (size_t)j * dim;
  double sum = 0.0;
  uint32_t cnt = 0;
  for (int i = threadIdx.x; i < n; i += kPostThreads) {
    const double r = post_distance(pj, pos + (size_t)i * dim, dim);
    if (est != nullptr) est[base + i] = r;
    const size_t cell = src + (size_t)(ord != nullptr ? ord[i] : i);
    const double v = vals[cell];
    const bool counts = __builtin_isfinite(v) && (codes == nullptr || codes[cell] == 0);
    if (counts) {
      sum += ::fabs(v - r);
      ++cnt;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    sum += __shfl_down(sum, off, 64);
    cnt += __shfl_down(cnt, off, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { wave_sum[wave] = sum; wave_cnt[wave] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = wave_sum[0];
    uint32_t k = wave_cnt[0];
    for (int w = 1; w < kPostThreads / 64; ++w) { t += wave_sum[w]; k += wave_cnt[w]; }
    line_sum[j] = t;
    line_cnt[j] = k;
  }
}

}  // namespace topolow
