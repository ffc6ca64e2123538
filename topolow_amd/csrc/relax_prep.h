// topolow_amd/csrc/relax_prep.h -- the pre-processing kernels: ordering sums, degrees, dense fill, edge list
// (reference R/core.R:269-436; host pipeline: topolow_layout_prep_create / _fetch in topolow_prep.hip, the one source
// that includes this header).  The device functions they build on, which the fold, fit and spectrum kernels use as
// well, are in relax_prep_device.h.
//
// Every kernel works in BUFFER coordinates: the caller's n x n buffer is read as B[a * n + b], a the slow index and
// b the contiguous one.  For a column-major matrix a is the column, for a row-major one (transposed != 0) the row;
// the host maps "slow"/"fast" to "row"/"column" and no transposed copy is made.
#pragma once

#include "relax_prep_device.h"

namespace topolow {

// First pass: one workgroup per tile of the lines that begin at slow0 (a chunk of whole 64-line blocks).
__global__ __launch_bounds__(kPrepThreads) void prep_sums_kernel(
    const double* __restrict__ vals, const int8_t* __restrict__ codes, int n, int slow0,
    double* __restrict__ part_slow_sum, int32_t* __restrict__ part_slow_cnt, double* __restrict__ part_fast_sum,
    int32_t* __restrict__ part_fast_cnt, uint8_t* __restrict__ diag_counts, PrepTotals* __restrict__ totals) {
  prep_tile_sums(vals, n, slow0 / kPrepTile + blockIdx.y, part_slow_sum, part_slow_cnt, part_fast_sum, part_fast_cnt,
                 diag_counts, PrepSumsCells{codes, totals});
}

// One thread per point: its partials added in block order.  out_sum / out_cnt are 2 x n: slow lines, then fast lines.
__global__ __launch_bounds__(kPrepThreads) void prep_finish_sums_kernel(
    int n, int n_blocks, const double* __restrict__ part_slow_sum, const int32_t* __restrict__ part_slow_cnt,
    const double* __restrict__ part_fast_sum, const int32_t* __restrict__ part_fast_cnt, double* __restrict__ out_sum,
    int32_t* __restrict__ out_cnt) {
  const int q = blockIdx.x * kPrepThreads + threadIdx.x;
  if (q >= n) return;
  double ss = 0.0, fs = 0.0;
  int32_t sc = 0, fc = 0;
  for (int blk = 0; blk < n_blocks; ++blk) {
    const size_t at = (size_t)blk * n + q;
    ss += part_slow_sum[at];
    sc += part_slow_cnt[at];
    fs += part_fast_sum[at];
    fc += part_fast_cnt[at];
  }
  out_sum[q] = ss;
  out_cnt[q] = sc;
  out_sum[(size_t)n + q] = fs;
  out_cnt[(size_t)n + q] = fc;
}

// Second pass, dense fill (R/core.R:340-374, 429-436) of the matrix gathered through ord: G[a][b] = B[ord[a]][ord[b]].
// U = G with NA as +Inf, C = its code (0 where NA).  A cell of the matrix's upper triangle keeps U, the mirrored cell
// takes the same U, so the result is symmetric bit for bit and reads the same in either layout.  One workgroup per
// 64 x 64 tile that holds upper cells: the source line ord[a] is contiguous and the lanes gather within it; the
// mirrored tile is written through LDS so that both stores have lanes on consecutive addresses.  Tiles wholly below
// the diagonal return at once: their mirror writes them.
//   upper_a_lt_b   != 0: the matrix's upper triangle is a < b (row-major buffer); 0: b < a (column-major)
__global__ __launch_bounds__(kPrepThreads) void prep_dense_kernel(
    const double* __restrict__ vals, const int8_t* __restrict__ codes, int n, const int32_t* __restrict__ ord,
    int upper_a_lt_b, double* __restrict__ dense, int32_t* __restrict__ tdense) {
  const int tb = blockIdx.x, ta = blockIdx.y;
  const bool diag_tile = ta == tb;
  if (!diag_tile && (upper_a_lt_b ? ta > tb : tb > ta)) return;
  __shared__ double U[kPrepTile][kPrepTile + 1];
  __shared__ int32_t Cd[kPrepTile][kPrepTile + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = tb * kPrepTile + lane;
  const size_t ob = b < n ? (size_t)ord[b] : 0;
  for (int r = wave; r < kPrepTile; r += kPrepWaves) {
    const int a = ta * kPrepTile + r;
    double u = __builtin_inf();
    int32_t c = 0;
    if (a < n && b < n) {
      const size_t cell = (size_t)ord[a] * (size_t)n + ob;
      const double v = vals[cell];
      if (!__builtin_isnan(v)) {
        u = v;
        c = codes != nullptr ? (int32_t)codes[cell] : 0;
      }
    }
    U[r][lane] = u;
    Cd[r][lane] = c;
  }
  __syncthreads();
  if (diag_tile) {
    for (int r = wave; r < kPrepTile; r += kPrepWaves) {
      const int a = ta * kPrepTile + r;
      if (a < n && b < n) {
        const bool upper = upper_a_lt_b ? r <= lane : lane <= r;
        const size_t at = (size_t)a * (size_t)n + (size_t)b;
        dense[at] = upper ? U[r][lane] : U[lane][r];
        tdense[at] = upper ? Cd[r][lane] : Cd[lane][r];
      }
    }
    return;
  }
  const int a2 = ta * kPrepTile + lane;
  for (int r = wave; r < kPrepTile; r += kPrepWaves) {
    const int a = ta * kPrepTile + r;
    if (a < n && b < n) {
      const size_t at = (size_t)a * (size_t)n + (size_t)b;
      dense[at] = U[r][lane];
      tdense[at] = Cd[r][lane];
    }
    const int b2 = tb * kPrepTile + r;   // the mirrored tile: slow index from this tile's fast block
    if (a2 < n && b2 < n) {
      const size_t at = (size_t)b2 * (size_t)n + (size_t)a2;
      dense[at] = U[lane][r];
      tdense[at] = Cd[lane][r];
    }
  }
}

// Edges of column j: the cells i < j of the dense fill that are not +Inf.  The fill is symmetric, so column j is
// line j of the buffer in either layout: contiguous reads.
__global__ __launch_bounds__(kPrepThreads) void prep_edge_count_kernel(const double* __restrict__ dense, int n,
                                                                        int32_t* __restrict__ col_edges) {
  const int j = blockIdx.x;
  const double* line = dense + (size_t)j * (size_t)n;
  int32_t k[1] = {0};
  for (int i = threadIdx.x; i < j; i += kPrepThreads) k[0] += line[i] != __builtin_inf() ? 1 : 0;
  prep_column_counts(k);
  if (threadIdx.x == 0) col_edges[j] = k[0];
}

// Column j's edges go to [edge_off[j], edge_off[j + 1]) in ascending i: which(arr.ind = TRUE) order (R/core.R:383-402).
__global__ __launch_bounds__(kPrepThreads) void prep_edge_write_kernel(
    const double* __restrict__ dense, const int32_t* __restrict__ tdense, int n, const int64_t* __restrict__ edge_off,
    int32_t* __restrict__ edge_i, int32_t* __restrict__ edge_j, double* __restrict__ edge_dist,
    int32_t* __restrict__ edge_thresh) {
  const int j = blockIdx.x;
  const size_t line = (size_t)j * (size_t)n;
  int64_t base[1] = {edge_off[j]}, e[1];
  for (int i0 = 0; i0 < j; i0 += kPrepThreads) {   // uniform over the workgroup
    const int i = i0 + threadIdx.x;
    const double d = i < j ? dense[line + i] : __builtin_inf();
    const bool valid[1] = {d != __builtin_inf()};
    prep_rank_trip(valid, base, e);
    if (valid[0]) {
      edge_i[e[0]] = i;
      edge_j[e[0]] = j;
      edge_dist[e[0]] = d;
      edge_thresh[e[0]] = tdense[line + i];
    }
  }
}

// The raw reordered matrix, CodedMatrix.reordered(order) in the buffer's own layout: out[a][b] = B[ord[a]][ord[b]].
// One workgroup per line a; the source line ord[a] is read by all of it and stays in L2.
__global__ __launch_bounds__(kPrepThreads) void prep_reorder_kernel(
    const double* __restrict__ vals, const int8_t* __restrict__ codes, int n, const int32_t* __restrict__ ord,
    double* __restrict__ out_vals, int8_t* __restrict__ out_codes) {
  const int a = blockIdx.x;
  const size_t src = (size_t)ord[a] * (size_t)n, dst = (size_t)a * (size_t)n;
  for (int b = threadIdx.x; b < n; b += kPrepThreads) {
    const size_t cell = src + (size_t)ord[b];
    if (out_vals != nullptr) out_vals[dst + b] = vals[cell];
    if (out_codes != nullptr) out_codes[dst + b] = codes[cell];
  }
}

}  // namespace topolow
