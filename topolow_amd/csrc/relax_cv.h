// topolow_amd/csrc/relax_cv.h -- device side of holding a cross-validation fold out of a resident session
// (topolow_session_hold_out / _restore_held_out / _score_pairs, include/topolow_relax.h).
//
// A fold differs from the full matrix in its held-out pairs only, so the session's encoded block -- and what was
// derived from it: the symmetric sweep's tile-major copy, the f64 delta tiles, the device edge list of the
// convergence MAE -- is patched at those pairs and put back afterwards; nothing of size n x n crosses PCIe.  All
// kernels here are plain scatter / gather over the pairs (session labels, lo < hi, every pair once: the host sorts
// and de-duplicates the caller's list, so no two threads touch the same word).
#pragma once

#include "relax_common.h"
#include "relax_device.h"
#include "relax_symm_plan.h"

namespace topolow {

// What a held-out cell carries between the two passes of a hold-out on a session that gathers its edge list: the
// edges whose cell holds this word are the ones to leave out (an edge whose pair was unmeasured in the block all
// along is not).  +Inf with code 3; no run ever sees it.
constexpr uint32_t kHeldMark = 0x7f800003u;

// Both mirrors of every pair <- word.  saved (nullable): 2 words per pair, what the mirrors (lo, hi) and (hi, lo) held.
__global__ __launch_bounds__(kThreads) void cv_mask_kernel(const int* __restrict__ lo, const int* __restrict__ hi,
                                                           long long n_pairs, uint32_t* __restrict__ enc, int ld,
                                                           uint32_t* __restrict__ saved, uint32_t word) {
  const long long q = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (q >= n_pairs) return;
  const size_t a = enc_index(lo[q], hi[q], ld), b = enc_index(hi[q], lo[q], ld);
  if (saved != nullptr) { saved[2 * q] = enc[a]; saved[2 * q + 1] = enc[b]; }
  enc[a] = word;
  enc[b] = word;
}

// Both mirrors of every pair <- the words cv_mask_kernel saved.
__global__ __launch_bounds__(kThreads) void cv_unmask_kernel(const int* __restrict__ lo, const int* __restrict__ hi,
                                                             long long n_pairs, uint32_t* __restrict__ enc, int ld,
                                                             const uint32_t* __restrict__ saved) {
  const long long q = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (q >= n_pairs) return;
  enc[enc_index(lo[q], hi[q], ld)] = saved[2 * q];
  enc[enc_index(hi[q], lo[q], ld)] = saved[2 * q + 1];
}

// The same patch on the tile-major copy of the whole upper triangle (the index map of symm_tiles_kernel /
// symm64_delta_kernel: cell (lo, hi) lies in tile (lo / 64, hi / 32); its mirror is in the copy too when both points
// share a diagonal square).  saved == nullptr: hold out (the unmeasured word; tdelta, when given, is saved into
// saved_delta and zeroed); otherwise put the saved words and deltas back.
__global__ __launch_bounds__(kThreads) void cv_tiles_kernel(const int* __restrict__ lo, const int* __restrict__ hi,
                                                            long long n_pairs, uint32_t* __restrict__ tenc,
                                                            float* __restrict__ tdelta, int TC,
                                                            const uint32_t* __restrict__ saved,
                                                            float* __restrict__ saved_delta) {
  const long long q = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (q >= n_pairs) return;
  const int l = lo[q], h = hi[q];
  const int R = l / kSymRows;
  const size_t up = (size_t)sym_tile_index(R, h / kSymCols, TC) * kSymTileWords + sym_word_in_tile(l % kSymRows, h % kSymCols);
  const bool mirrored = h / kSymRows == R;
  const size_t dn = mirrored ? (size_t)sym_tile_index(R, l / kSymCols, TC) * kSymTileWords + sym_word_in_tile(h % kSymRows, l % kSymCols) : 0;
  if (saved == nullptr) {
    tenc[up] = kInfWord;
    if (mirrored) tenc[dn] = kInfWord;
    if (tdelta != nullptr) {
      saved_delta[q] = tdelta[up];   // (the delta kernel writes one value to both cells)
      tdelta[up] = 0.0f;
      if (mirrored) tdelta[dn] = 0.0f;
    }
  } else {
    tenc[up] = saved[2 * q];
    if (mirrored) tenc[dn] = saved[2 * q + 1];
    if (tdelta != nullptr) {
      tdelta[up] = saved_delta[q];
      if (mirrored) tdelta[dn] = saved_delta[q];
    }
  }
}

// ---- the device edge list without the held-out edges: a stable compaction, so that the list -- and with it the
// summation order of the edge MAE -- is the one a fresh session loaded with the fold's list would hold ----
__device__ __forceinline__ bool cv_edge_kept(const int* ei, const int* ej, long long e, const uint32_t* enc, int ld, int n) {
  const int a = ei[e], b = ej[e];
  if (a < 0 || b < 0 || a >= n || b >= n) return true;   // (not a cell of the block: left as the caller listed it)
  return enc[enc_index(a, b, ld)] != kHeldMark;
}

// count[b] = kept edges among the kThreads edges of workgroup b
__global__ __launch_bounds__(kThreads) void cv_edges_count_kernel(const int* __restrict__ ei, const int* __restrict__ ej,
                                                                  long long n_edges, const uint32_t* __restrict__ enc,
                                                                  int ld, int n, int* __restrict__ count) {
  const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
  const bool keep = e < n_edges && cv_edge_kept(ei, ej, e, enc, ld, n);
  const int c = __syncthreads_count(keep ? 1 : 0);
  if (threadIdx.x == 0) count[blockIdx.x] = c;
}

// offset[b] = count[0] + ... + count[b - 1]; offset[n_blocks] = the total.  One workgroup, chunks of 1024 with a carry.
__global__ __launch_bounds__(1024) void cv_scan_kernel(const int* __restrict__ count, int n_blocks,
                                                       long long* __restrict__ offset) {
  __shared__ long long sh[1024];
  __shared__ long long carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < n_blocks; base += 1024) {
    const int b = base + (int)threadIdx.x;
    const long long own = b < n_blocks ? (long long)count[b] : 0;
    sh[threadIdx.x] = own;
    __syncthreads();
    for (int step = 1; step < 1024; step <<= 1) {   // inclusive scan
      const long long add = (int)threadIdx.x >= step ? sh[threadIdx.x - step] : 0;
      __syncthreads();
      sh[threadIdx.x] += add;
      __syncthreads();
    }
    if (b < n_blocks) offset[b] = carry + sh[threadIdx.x] - own;
    __syncthreads();
    if (threadIdx.x == 0) carry += sh[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) offset[n_blocks] = carry;
}

template <typename tgt_t>
__global__ __launch_bounds__(kThreads) void cv_edges_compact_kernel(
    const int* __restrict__ ei, const int* __restrict__ ej, const tgt_t* __restrict__ et, const int8_t* __restrict__ ec,
    long long n_edges, const uint32_t* __restrict__ enc, int ld, int n, const long long* __restrict__ offset,
    int* __restrict__ oi, int* __restrict__ oj, tgt_t* __restrict__ ot, int8_t* __restrict__ oc) {
  __shared__ int wave_total[kWaves];
  const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
  const bool keep = e < n_edges && cv_edge_kept(ei, ej, e, enc, ld, n);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long votes = __ballot(keep ? 1 : 0);
  const int before = __popcll(votes & ((1ull << lane) - 1ull));
  if (lane == 0) wave_total[wave] = __popcll(votes);
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += wave_total[w];
  if (!keep) return;
  const long long to = offset[blockIdx.x] + base + before;
  oi[to] = ei[e]; oj[to] = ej[e]; ot[to] = et[e]; oc[to] = ec[e];
}

// ---- out-of-sample score: sum |truth - ||p_i - p_j||| over the pairs (session labels), distances and sums in f64
// whatever the positions' precision; one partial per workgroup, summed by the host in index order ----
template <typename real>
__global__ __launch_bounds__(kThreads) void cv_score_kernel(const real* __restrict__ pos, int dim,
                                                            const int* __restrict__ pi, const int* __restrict__ pj,
                                                            const double* __restrict__ truth, long long n_pairs,
                                                            double* __restrict__ part_sum) {
  double s = 0.0;
  for (long long q = (long long)blockIdx.x * kThreads + threadIdx.x; q < n_pairs; q += (long long)gridDim.x * kThreads) {
    const real* a = pos + (size_t)pi[q] * dim;
    const real* b = pos + (size_t)pj[q] * dim;
    double d2 = 0.0;
    for (int d = 0; d < dim; ++d) {
      const double diff = (double)a[d] - (double)b[d];
      d2 = fma(diff, diff, d2);
    }
    s += fabs(truth[q] - ::sqrt(d2));
  }
  __shared__ double sh[kWaves];
  s = wave_sum<double>(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < kWaves; ++w) t += sh[w];
    part_sum[blockIdx.x] = t;
  }
}

}  // namespace topolow
