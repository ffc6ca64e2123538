// topolow_amd/csrc/relax_prep_device.h -- the device functions the pre-processing kernels share: the order key, the
// fold mask's bit test, the wave reductions of the totals, the sums pass of one tile and the full matrix's cell policy;
// through relax_prep_rank.h the ranked compaction.  Included by relax_prep.h, relax_prep_fold.h, relax_fit.h and
// relax_spectrum.h.  No kernels here: any source may include it.
//
// Everything works in BUFFER coordinates: the caller's n x n buffer is read as B[a * n + b], a the slow index and
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

// One bit per cell of the handle's buffer (the fold mask of relax_prep_fold.h): bit a * n + b for the cell B[a * n + b].
__device__ inline bool fold_bit(const uint32_t* __restrict__ mask, size_t cell) {
  return (mask[cell >> 5] >> (cell & 31)) & 1u;
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

}  // namespace topolow
