// topolow_amd/csrc/relax_prep_rank.h -- the ranked compaction of K lists of one column's cells, one workgroup of
// kPrepThreads per column: K = 1 the edge list of relax_prep.h, K = 2 a fold's held-out pairs and scored cells
// (relax_prep_fold.h).  A kernel classifies its cells; these two helpers count them and rank them.
#pragma once

#include "relax_prep_types.h"

namespace topolow {

// Counting: every thread brings how many cells it found for each list; thread 0 leaves with the column's totals.
template <int K>
__device__ inline void prep_column_counts(int32_t (&k)[K]) {
  __shared__ int32_t wave_cnt[K][kPrepWaves];
  for (int off = 32; off > 0; off >>= 1)
    for (int q = 0; q < K; ++q) k[q] += __shfl_down(k[q], off, 64);
  for (int q = 0; q < K; ++q)
    if ((threadIdx.x & 63) == 0) wave_cnt[q][threadIdx.x >> 6] = k[q];
  __syncthreads();
  for (int q = 0; q < K && threadIdx.x == 0; ++q)
    for (int w = 1; w < kPrepWaves; ++w) k[q] += wave_cnt[q][w];
}

// Ranking, 256 cells per trip of the whole workgroup: in[q] -- is this thread's cell in list q?; base[q] -- the slot of
// list q's first cell of this trip, moved on by the trip's count.  slot[q] = base[q] + the waves before this one + the
// set bits below the lane in its wave's ballot: a rank, never what an atomic returned, so no list depends on timing.
template <int K>
__device__ inline void prep_rank_trip(const bool (&in)[K], int64_t (&base)[K], int64_t (&slot)[K]) {
  __shared__ int32_t wave_cnt[K][kPrepWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long m[K];
  for (int q = 0; q < K; ++q) {
    m[q] = __ballot(in[q]);
    if (lane == 0) wave_cnt[q][wave] = __popcll(m[q]);
  }
  __syncthreads();   // one pair of barriers for all K lists
  for (int q = 0; q < K; ++q) {
    int32_t before = 0, all = 0;
    for (int w = 0; w < kPrepWaves; ++w) { before += w < wave ? wave_cnt[q][w] : 0; all += wave_cnt[q][w]; }
    slot[q] = base[q] + before + __popcll(m[q] & ((1ull << lane) - 1ull));
    base[q] += all;
  }
  __syncthreads();
}

}  // namespace topolow
