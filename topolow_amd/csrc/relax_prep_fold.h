// topolow_amd/csrc/relax_prep_fold.h -- one cross-validation fold prepared from a resident handle: the fold mask, the
// ordering sums and degrees of the masked matrix, the held-out pairs and the scored cells (host pipeline:
// topolow_layout_prep_fold / _cv_sweep in topolow_relax.hip; the host twin on the cell list: relax_fold.h, fold_pairs).
//
// A fold is its picks -- linear column-major indices r + c * n -- and their mirrors (fold_dropped).  The kernels work
// on a FOLD MASK, one bit per cell of the handle's buffer, bit a * n + b for the cell B[a * n + b]; it lives in the
// handle and is cleared at the end of every fold.
//
// Folds are held out of SYMMETRIC matrices only (fold_symmetry_kernel decides it once per handle: the condition of
// fold_cells_symmetric).  A symmetric matrix reads the same row- or column-major, so every kernel here treats the
// handle's buffer as COLUMN-major whatever `transposed` says: the slow index a is the column, the contiguous index b
// the row, and a pick IS its bit index.  Nothing here writes vals or codes.
#pragma once

#include "relax_prep.h"

namespace topolow {

// Integer counts and a maximum, as PrepTotals: atomics do not make them depend on the grid.
struct FoldTotals {
  unsigned long long max_key;        // prep_order_key of the largest kept non-NA code-0 value; 0: there is none
  unsigned long long n_upper;        // kept non-NA cells strictly above the diagonal (row < column)
  unsigned long long n_bad_picks;    // picks outside [0, n * n): counted, written nowhere
  unsigned long long n_asymmetric;   // off-diagonal cells that differ from their mirror (fold_symmetry_kernel)
};

__device__ inline bool fold_bit(const uint32_t* __restrict__ mask, size_t cell) {
  return (mask[cell >> 5] >> (cell & 31)) & 1u;
}

// mark: one thread per pick sets the bits of (r, c) and (c, r).  A pick listed twice, or together with its mirror,
// sets a bit twice, which is setting it once: no sort, no de-duplication.
__global__ __launch_bounds__(kPrepThreads) void fold_mark_kernel(const long long* __restrict__ picks, long long n_picks,
                                                                  int n, uint32_t* __restrict__ mask,
                                                                  FoldTotals* __restrict__ totals) {
  const long long q = (long long)blockIdx.x * kPrepThreads + threadIdx.x;
  if (q >= n_picks) return;
  const long long x = picks[q];
  if (x < 0 || x >= (long long)n * n) {
    atomicAdd(&totals->n_bad_picks, 1ull);
    return;
  }
  const long long r = x % n, c = x / n, y = c + r * n;
  atomicOr(&mask[x >> 5], 1u << (x & 31));
  atomicOr(&mask[y >> 5], 1u << (y & 31));
}

// The first pass of prep_sums_kernel on the masked matrix: a masked cell is NA.  Same 64 x 64 tiles through LDS, same
// partial per (point, block of 64 cells) added in index order from 0.0, same diag_counts; of the totals the fold needs
// the maximum (-> numeric_max) and the kept upper-triangle count (-> n_edges).  prep_finish_sums_kernel adds the
// partials as it does for the full matrix.  Grid: (blocks of b, blocks of a).
__global__ __launch_bounds__(kPrepThreads) void fold_sums_kernel(
    const double* __restrict__ vals, const int8_t* __restrict__ codes, const uint32_t* __restrict__ mask, int n,
    double* __restrict__ part_slow_sum, int32_t* __restrict__ part_slow_cnt, double* __restrict__ part_fast_sum,
    int32_t* __restrict__ part_fast_cnt, uint8_t* __restrict__ diag_counts, FoldTotals* __restrict__ totals) {
  __shared__ double tile[kPrepTile][kPrepTile + 1];
  __shared__ uint8_t flag[kPrepTile][kPrepTile + 4];
  const int tb = blockIdx.x, ta = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = tb * kPrepTile + lane;
  unsigned long long upper = 0, max_key = 0;
  for (int r = wave; r < kPrepTile; r += kPrepWaves) {
    const int a = ta * kPrepTile + r;
    double x = 0.0;
    uint8_t f = 0;
    if (a < n && b < n) {
      const size_t cell = (size_t)a * (size_t)n + (size_t)b;
      const double v = vals[cell];
      if (!__builtin_isnan(v) && !fold_bit(mask, cell)) {
        f = 1;
        if (a != b) x = v;
        if (b < a) ++upper;
        if (codes == nullptr || codes[cell] == 0) {
          const unsigned long long key = prep_order_key(v);
          max_key = key > max_key ? key : max_key;
        }
      }
      if (a == b) diag_counts[a] = f;
    }
    tile[r][lane] = x;
    flag[r][lane] = f;
  }
  upper = prep_wave_sum(upper);
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long other = __shfl_down(max_key, off, 64);
    max_key = other > max_key ? other : max_key;
  }
  if (lane == 0) {
    if (upper) atomicAdd(&totals->n_upper, upper);
    if (max_key) atomicMax(&totals->max_key, max_key);
  }
  __syncthreads();
  if (threadIdx.x < kPrepTile) {
    const int r = threadIdx.x, a = ta * kPrepTile + r;
    if (a < n) {
      double s = 0.0;
      int32_t k = 0;
      for (int q = 0; q < kPrepTile; ++q) { s += tile[r][q]; k += flag[r][q]; }
      part_slow_sum[(size_t)tb * n + a] = s;
      part_slow_cnt[(size_t)tb * n + a] = k;
    }
  } else if (threadIdx.x < 2 * kPrepTile) {
    const int l = threadIdx.x - kPrepTile, bb = tb * kPrepTile + l;
    if (bb < n) {
      double s = 0.0;
      int32_t k = 0;
      for (int q = 0; q < kPrepTile; ++q) { s += tile[q][l]; k += flag[q][l]; }
      part_fast_sum[(size_t)ta * n + bb] = s;
      part_fast_cnt[(size_t)ta * n + bb] = k;
    }
  }
}

// What the compaction lists of cell (row b, column a): a held-out PAIR when it is masked, not NA and b < a; a SCORED
// cell when it is masked, not NA and numeric (code 0), every mirror on its own, the diagonal included.  The mask is
// read for every cell, value and code only where it is set: a fold masks a few per cent of the cells.
__device__ inline void fold_cell_kind(const double* __restrict__ vals, const int8_t* __restrict__ codes,
                                      const uint32_t* __restrict__ mask, size_t cell, int a, int b, bool* pair,
                                      bool* scored, double* value) {
  *pair = false;
  *scored = false;
  *value = 0.0;
  if (!fold_bit(mask, cell)) return;
  const double v = vals[cell];
  if (__builtin_isnan(v)) return;   // a masked NA cell is in no list, as on the host
  *value = v;
  *pair = b < a;
  *scored = codes == nullptr || codes[cell] == 0;
}

// Column a's held-out pairs and scored cells, counted.  One workgroup per column: line a of the buffer, contiguous.
__global__ __launch_bounds__(kPrepThreads) void fold_compact_count_kernel(
    const double* __restrict__ vals, const int8_t* __restrict__ codes, const uint32_t* __restrict__ mask, int n,
    int32_t* __restrict__ col_pairs, int32_t* __restrict__ col_scored) {
  __shared__ int32_t wave_cnt[2][kPrepWaves];
  const int a = blockIdx.x;
  const size_t line = (size_t)a * (size_t)n;
  int32_t kp = 0, ks = 0;
  for (int b = threadIdx.x; b < n; b += kPrepThreads) {
    bool pair, scored;
    double v;
    fold_cell_kind(vals, codes, mask, line + b, a, b, &pair, &scored, &v);
    kp += pair ? 1 : 0;
    ks += scored ? 1 : 0;
  }
  for (int off = 32; off > 0; off >>= 1) {
    kp += __shfl_down(kp, off, 64);
    ks += __shfl_down(ks, off, 64);
  }
  if ((threadIdx.x & 63) == 0) { wave_cnt[0][threadIdx.x >> 6] = kp; wave_cnt[1][threadIdx.x >> 6] = ks; }
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t tp = 0, ts = 0;
    for (int w = 0; w < kPrepWaves; ++w) { tp += wave_cnt[0][w]; ts += wave_cnt[1][w]; }
    col_pairs[a] = tp;
    col_scored[a] = ts;
  }
}

// The stable compaction, in the manner of prep_edge_write_kernel: column a's pairs go to [pair_off[a], pair_off[a + 1])
// and its scored cells to [score_off[a], score_off[a + 1]), both in ascending row -- the pairs sorted by (j, i), the
// scored cells in ascending column-major index with their truth from vals.  A cell's slot is its rank in that order,
// never what an atomic returned: the lists do not depend on timing.
__global__ __launch_bounds__(kPrepThreads) void fold_compact_write_kernel(
    const double* __restrict__ vals, const int8_t* __restrict__ codes, const uint32_t* __restrict__ mask, int n,
    const int64_t* __restrict__ pair_off, const int64_t* __restrict__ score_off, int32_t* __restrict__ pair_i,
    int32_t* __restrict__ pair_j, int32_t* __restrict__ score_r, int32_t* __restrict__ score_c,
    double* __restrict__ score_truth) {
  __shared__ int32_t wave_cnt[2][kPrepWaves];
  const int a = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t line = (size_t)a * (size_t)n;
  int64_t pbase = pair_off[a], sbase = score_off[a];
  if (pair_off[a + 1] == pbase && score_off[a + 1] == sbase) return;   // uniform: nothing of this column is listed
  for (int b0 = 0; b0 < n; b0 += kPrepThreads) {   // uniform over the workgroup
    const int b = b0 + threadIdx.x;
    bool pair = false, scored = false;
    double v = 0.0;
    if (b < n) fold_cell_kind(vals, codes, mask, line + b, a, b, &pair, &scored, &v);
    const unsigned long long pm = __ballot(pair), sm = __ballot(scored);
    if (lane == 0) { wave_cnt[0][wave] = __popcll(pm); wave_cnt[1][wave] = __popcll(sm); }
    __syncthreads();
    int32_t pbefore = 0, pall = 0, sbefore = 0, sall = 0;
    for (int w = 0; w < kPrepWaves; ++w) {
      pbefore += w < wave ? wave_cnt[0][w] : 0;
      pall += wave_cnt[0][w];
      sbefore += w < wave ? wave_cnt[1][w] : 0;
      sall += wave_cnt[1][w];
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    if (pair) {
      const int64_t e = pbase + pbefore + __popcll(pm & below);
      pair_i[e] = b;
      pair_j[e] = a;
    }
    if (scored) {
      const int64_t e = sbase + sbefore + __popcll(sm & below);
      score_r[e] = b;
      score_c[e] = a;
      score_truth[e] = v;
    }
    pbase += pall;
    sbase += sall;
    __syncthreads();
  }
}

// The held-out pairs in session labels, lo < hi: inv (nullable) maps the caller's label to the session's.
__global__ __launch_bounds__(kPrepThreads) void fold_pair_labels_kernel(const int32_t* __restrict__ pair_i,
                                                                         const int32_t* __restrict__ pair_j,
                                                                         long long n_pairs, const int* __restrict__ inv,
                                                                         int* __restrict__ lo, int* __restrict__ hi) {
  const long long q = (long long)blockIdx.x * kPrepThreads + threadIdx.x;
  if (q >= n_pairs) return;
  int x = pair_i[q], y = pair_j[q];
  if (inv != nullptr) { x = inv[x]; y = inv[y]; }
  lo[q] = x < y ? x : y;
  hi[q] = x < y ? y : x;
}

// The points a scored cell (r, c) is scored against: order[r], order[c] where an order is given (an unnamed,
// reordered fold: fold_pairs), then the session's label of that point where inv is given.  out may be the input.
__global__ __launch_bounds__(kPrepThreads) void fold_score_points_kernel(
    const int32_t* score_r, const int32_t* score_c, long long n_scored, const int32_t* __restrict__ order,
    const int* __restrict__ inv, int* out_i, int* out_j) {
  const long long q = (long long)blockIdx.x * kPrepThreads + threadIdx.x;
  if (q >= n_scored) return;
  int x = score_r[q], y = score_c[q];
  if (order != nullptr) { x = order[x]; y = order[y]; }
  if (inv != nullptr) { x = inv[x]; y = inv[y]; }
  out_i[q] = x;
  out_j[q] = y;
}

// Once per handle: does every off-diagonal cell have a mirror with the same value bits, the same NA-ness and the same
// code (two NA cells agree whatever they carry)?  One workgroup per pair of mirrored tiles, ta <= tb: tile (ta, tb)
// goes to LDS, tile (tb, ta) is read against its transpose; both reads have lanes on consecutive addresses.
__global__ __launch_bounds__(kPrepThreads) void fold_symmetry_kernel(const double* __restrict__ vals,
                                                                      const int8_t* __restrict__ codes, int n,
                                                                      FoldTotals* __restrict__ totals) {
  const int tb = blockIdx.x, ta = blockIdx.y;
  if (ta > tb) return;
  __shared__ unsigned long long bits[kPrepTile][kPrepTile + 1];
  __shared__ int8_t code[kPrepTile][kPrepTile + 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = wave; r < kPrepTile; r += kPrepWaves) {
    const int a = ta * kPrepTile + r, b = tb * kPrepTile + lane;
    unsigned long long w = 0;
    int8_t c = 0;
    if (a < n && b < n) {
      const size_t cell = (size_t)a * (size_t)n + (size_t)b;
      w = (unsigned long long)__double_as_longlong(vals[cell]);
      c = codes != nullptr ? codes[cell] : (int8_t)0;
    }
    bits[r][lane] = w;
    code[r][lane] = c;
  }
  __syncthreads();
  unsigned long long bad = 0;
  for (int r = wave; r < kPrepTile; r += kPrepWaves) {
    const int a = tb * kPrepTile + r, b = ta * kPrepTile + lane;   // the mirror of LDS cell [lane][r]
    if (a < n && b < n && a != b) {
      const size_t cell = (size_t)a * (size_t)n + (size_t)b;
      const double v = vals[cell];
      const unsigned long long w = bits[lane][r];
      const bool na = __builtin_isnan(v), mirror_na = __builtin_isnan(__longlong_as_double((long long)w));
      if (na != mirror_na) {
        ++bad;
      } else if (!na) {
        const int8_t c = codes != nullptr ? codes[cell] : (int8_t)0;
        if ((unsigned long long)__double_as_longlong(v) != w || c != code[lane][r]) ++bad;
      }
    }
  }
  bad = prep_wave_sum(bad);
  if (lane == 0 && bad) atomicAdd(&totals->n_asymmetric, bad);
}

}  // namespace topolow
