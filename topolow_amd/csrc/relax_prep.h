// topolow_amd/csrc/relax_prep.h -- the pre-processing kernels: ordering sums, degrees, dense fill, edge list
// (reference R/core.R:269-436; host pipeline: topolow_layout_prep_* in topolow_prep.hip).
//
// Every kernel works in BUFFER coordinates: the caller's n x n buffer is read as B[a * n + b], a the slow index and
// b the contiguous one.  For a column-major matrix a is the column, for a row-major one (transposed != 0) the row;
// the host maps "slow"/"fast" to "row"/"column" and no transposed copy is made.
#pragma once

#include "relax_prep_rank.h"

namespace topolow {

// f64 -> u64, monotone over -Inf..+Inf; never 0 (the smallest image, that of -Inf, is 0x000f...).
__device__ inline unsigned long long prep_order_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ inline unsigned long long prep_wave_sum(unsigned long long x) {
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;
}
__device__ inline unsigned long long prep_wave_max(unsigned long long x) {
  for (int off = 32; off > 0; off >>= 1) x = max(x, (unsigned long long)__shfl_down(x, off, 64));
  return x;
}
// A wave's share x of a whole-matrix total: lane 0 adds it (kMax: takes the maximum with it) where it is not 0.
template <bool kMax = false>
__device__ inline void prep_flush(unsigned long long* total, unsigned long long x) {
  x = kMax ? prep_wave_max(x) : prep_wave_sum(x);
  if ((threadIdx.x & 63) == 0 && x) kMax ? atomicMax(total, x) : atomicAdd(total, x);
}

// The sums pass of one 64 x 64 tile (slow block ta, fast block tb = blockIdx.x), shared with the masked sums of a fold
// (relax_prep_fold.h).  The tile goes to LDS once -- lanes along the contiguous index, 8-byte loads, consecutive lanes
// on consecutive addresses -- with cells that are not kept, the diagonal and cells past n as 0.0, and a flag per kept
// cell.  Then thread t < 64 adds slow line t of the tile and thread 64 + t fast line t, both sequentially in index
// order from 0.0: the partial of (point, block of 64 cells) is the same bits along either direction, whatever the
// layout and whatever the grid.  part_slow_* [tb * n + a]: slow line a over fast block tb; part_fast_* [ta * n + b]:
// fast line b over slow block ta; diag_counts[a]: is the diagonal cell kept (the counts include it, the sums do not).
// Cells is the per-cell policy: kept(cell, v) -- does B[cell] = v count?; count(a, b, cell, v) -- a kept cell's share
// of the caller's totals; flush() -- after the tile, the wave's totals to memory, one lane per wave.
template <typename Cells>
__device__ inline void prep_tile_sums(const double* __restrict__ vals, int n, int ta,
                                      double* __restrict__ part_slow_sum, int32_t* __restrict__ part_slow_cnt,
                                      double* __restrict__ part_fast_sum, int32_t* __restrict__ part_fast_cnt,
                                      uint8_t* __restrict__ diag_counts, Cells cells) {
  __shared__ double tile[kPrepTile][kPrepTile + 1];
  __shared__ uint8_t flag[kPrepTile][kPrepTile + 4];
  const int tb = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = tb * kPrepTile + lane;
  for (int r = wave; r < kPrepTile; r += kPrepWaves) {
    const int a = ta * kPrepTile + r;
    double x = 0.0;
    uint8_t f = 0;
    if (a < n && b < n) {
      const size_t cell = (size_t)a * (size_t)n + (size_t)b;
      const double v = vals[cell];
      if (cells.kept(cell, v)) {
        f = 1;
        if (a != b) x = v;
        cells.count(a, b, cell, v);
      }
      if (a == b) diag_counts[a] = f;
    }
    tile[r][lane] = x;
    flag[r][lane] = f;
  }
  cells.flush();
  __syncthreads();
  auto add_line = [&](bool slow, int blk, int p, double* __restrict__ sum, int32_t* __restrict__ cnt) {
    if (p >= n) return;   // point p's line `lane` of the tile, over block blk of the other index
    double s = 0.0;
    int32_t k = 0;
    for (int q = 0; q < kPrepTile; ++q) {
      s += slow ? tile[lane][q] : tile[q][lane];
      k += slow ? flag[lane][q] : flag[q][lane];
    }
    sum[(size_t)blk * n + p] = s;
    cnt[(size_t)blk * n + p] = k;
  };
  if (wave == 0) add_line(true, tb, ta * kPrepTile + lane, part_slow_sum, part_slow_cnt);
  else if (wave == 1) add_line(false, ta, b, part_fast_sum, part_fast_cnt);
}

// The full matrix's cells: every non-NA cell is kept; c is its code, read beside the value whether it is kept or not.
struct PrepSumsCells {
  const int8_t* __restrict__ codes;
  PrepTotals* __restrict__ totals;
  int c = 0;
  PrepTotals t = {};
  __device__ bool kept(size_t cell, double v) {
    c = codes != nullptr ? (int)codes[cell] : 0;
    return !__builtin_isnan(v);
  }
  __device__ void count(int, int, size_t, double v) {
    const double scaled = v * 1024.0;
    if (__builtin_isinf(v)) ++t.n_infinite;
    if (v < 0.0) ++t.n_negative;
    if (!(v >= 0.0 && v < 1048576.0 && scaled == ::floor(scaled))) ++t.n_inexact;
    if (c != 0) return;
    t.max_key = max(t.max_key, prep_order_key(v));
    if (__builtin_isfinite(v) && v != 0.0) ++t.n_finite_nonzero;
  }
  __device__ void flush() {
    prep_flush(&totals->n_finite_nonzero, t.n_finite_nonzero);
    prep_flush(&totals->n_infinite, t.n_infinite);
    prep_flush(&totals->n_negative, t.n_negative);
    prep_flush(&totals->n_inexact, t.n_inexact);
    prep_flush<true>(&totals->max_key, t.max_key);
  }
};

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
