// topolow_amd/csrc/relax_prep_fold.h -- one cross-validation fold prepared from a resident handle: the fold mask, the
// ordering sums and degrees of the masked matrix, the held-out pairs and the scored cells (host pipeline:
// topolow_layout_prep_fold / _cv_sweep in topolow_prep_fold.hip; the host twin on the cell list: relax_fold.h, fold_pairs).
//
// A fold is its picks -- linear column-major indices r + c * n -- and their mirrors (fold_dropped).  The kernels work
// on a FOLD MASK, one bit per cell of the handle's buffer, bit a * n + b for the cell B[a * n + b]; it lives in the
// handle and is cleared at the end of every fold.
//
// Folds are held out of SYMMETRIC matrices only (fold_symmetry_kernel decides it once per handle: the condition of
// fold_cells_symmetric).  A symmetric matrix reads the same row- or column-major, so every kernel here treats the
// handle's buffer as COLUMN-major whatever `transposed` says: the slow index a is the column, the contiguous index b
// the row, and a pick IS its bit index.  Nothing here writes vals or codes.
//
// The masked sums are prep_tile_sums of relax_prep_device.h with this file's policy, the compaction prep_column_counts and
// prep_rank_trip of relax_prep_rank.h with this file's cell test: only what a fold adds to them is written here.
#pragma once

#include "relax_prep_device.h"

namespace topolow {

// (fold_bit, the mask's bit test, is in relax_prep_device.h: the fit kernels of other sources read the mask too.)

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

// The masked matrix's cells for prep_tile_sums: a masked cell is NA.  Of the totals the fold needs the maximum
// (-> numeric_max) and the kept upper-triangle count (-> n_edges); the code is read where the cell is kept.
struct FoldSumsCells {
  const int8_t* __restrict__ codes;
  const uint32_t* __restrict__ mask;
  FoldTotals* __restrict__ totals;
  unsigned long long upper = 0, max_key = 0;
  __device__ bool kept(size_t cell, double v) const { return !__builtin_isnan(v) && !fold_bit(mask, cell); }
  __device__ void count(int a, int b, size_t cell, double v) {
    if (b < a) ++upper;
    if (codes == nullptr || codes[cell] == 0) max_key = max(max_key, prep_order_key(v));
  }
  __device__ void flush() {
    prep_flush(&totals->n_upper, upper);
    prep_flush<true>(&totals->max_key, max_key);
  }
};

// The first pass on the masked matrix; prep_finish_sums_kernel adds the partials as it does for the full matrix.
// Grid: (blocks of b, blocks of a).
__global__ __launch_bounds__(kPrepThreads) void fold_sums_kernel(
    const double* __restrict__ vals, const int8_t* __restrict__ codes, const uint32_t* __restrict__ mask, int n,
    double* __restrict__ part_slow_sum, int32_t* __restrict__ part_slow_cnt, double* __restrict__ part_fast_sum,
    int32_t* __restrict__ part_fast_cnt, uint8_t* __restrict__ diag_counts, FoldTotals* __restrict__ totals) {
  prep_tile_sums(vals, n, blockIdx.y, part_slow_sum, part_slow_cnt, part_fast_sum, part_fast_cnt, diag_counts,
                 FoldSumsCells{codes, mask, totals});
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

// Column a's held-out pairs and scored cells, counted (prep_column_counts).  One workgroup per column: line a of the
// buffer, contiguous.
__global__ __launch_bounds__(kPrepThreads) void fold_compact_count_kernel(
    const double* __restrict__ vals, const int8_t* __restrict__ codes, const uint32_t* __restrict__ mask, int n,
    int32_t* __restrict__ col_pairs, int32_t* __restrict__ col_scored) {
  const int a = blockIdx.x;
  const size_t line = (size_t)a * (size_t)n;
  int32_t k[2] = {0, 0};
  for (int b = threadIdx.x; b < n; b += kPrepThreads) {
    bool pair, scored;
    double v;
    fold_cell_kind(vals, codes, mask, line + b, a, b, &pair, &scored, &v);
    k[0] += pair ? 1 : 0;
    k[1] += scored ? 1 : 0;
  }
  prep_column_counts(k);
  if (threadIdx.x == 0) {
    col_pairs[a] = k[0];
    col_scored[a] = k[1];
  }
}

// The stable compaction (prep_rank_trip, both lists at once): column a's pairs go to [pair_off[a], pair_off[a + 1]) and
// its scored cells to [score_off[a], score_off[a + 1]), both in ascending row -- the pairs sorted by (j, i), the scored
// cells in ascending column-major index with their truth from vals.
__global__ __launch_bounds__(kPrepThreads) void fold_compact_write_kernel(
    const double* __restrict__ vals, const int8_t* __restrict__ codes, const uint32_t* __restrict__ mask, int n,
    const int64_t* __restrict__ pair_off, const int64_t* __restrict__ score_off, int32_t* __restrict__ pair_i,
    int32_t* __restrict__ pair_j, int32_t* __restrict__ score_r, int32_t* __restrict__ score_c,
    double* __restrict__ score_truth) {
  const int a = blockIdx.x;
  const size_t line = (size_t)a * (size_t)n;
  int64_t base[2] = {pair_off[a], score_off[a]}, e[2];
  if (pair_off[a + 1] == base[0] && score_off[a + 1] == base[1]) return;   // uniform: nothing of this column is listed
  for (int b0 = 0; b0 < n; b0 += kPrepThreads) {   // uniform over the workgroup
    const int b = b0 + threadIdx.x;
    bool in[2] = {false, false};   // a held-out pair, a scored cell
    double v = 0.0;
    if (b < n) fold_cell_kind(vals, codes, mask, line + b, a, b, &in[0], &in[1], &v);
    prep_rank_trip(in, base, e);
    if (in[0]) {
      pair_i[e[0]] = b;
      pair_j[e[0]] = a;
    }
    if (in[1]) {
      score_r[e[1]] = b;
      score_c[e[1]] = a;
      score_truth[e[1]] = v;
    }
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
