// topolow_amd/csrc/relax_prep_prune.h -- degrees of a resident matrix and the pruning of its poorly connected points
// (reference R/diagnostics.R:434-475 analyze_network_structure, R/data_preprocessing.R:1225-1503 prune_sparse_matrix;
// host pipeline: topolow_layout_prep_degrees / _prune in topolow_prep_graph.hip).
//
// Everything here works on the packed bits graph_bits_kernel (relax_prep_graph.h) leaves: the n x n doubles are read
// once per call.  The counts are along MATRIX ROWS and the matrix need not be symmetric, so the bits must be
// row-oriented: bit (r, c) = cell (r, c) is measured.  graph_bits_kernel gives bits in buffer coordinates; where a buffer
// line is a matrix column, prune_bits_transpose_kernel turns them round, 64 x 64 bits per wave -- the doubles are not
// read again and no transposed n x n copy of them is made.
//
// A round of the pruning is two launches on one stream; what one writes the next reads across the launch boundary, and
// no kernel waits on another thread:
//   prune_count_kernel    for every line l alive: count[l] = sum over words of popcount(bits[l][w] & alive[w]), one wave
//                         per line, lanes over words; flag[l] = count[l] < min_connections; the round's n_remove and
//                         sum of counts (the cell count of the kept submatrix) go to the state, one integer atomic of
//                         each per workgroup;
//   prune_decide_kernel   one workgroup: nothing flagged -> converged; size - n_remove < min_points -> stop, the mask as
//                         it is; otherwise the flagged lines leave `alive` and the size drops.
// Both test st->stopped first, so the host launches rounds in batches and reads one PruneState per batch: the rounds
// behind a stop change nothing.  Every loop is bounded by `words`; integer atomics only, so any order gives the same
// result.  The same count kernel with every line alive and min_connections = 0 gives the degrees.
//
// gfx950 code object (make resource): prune_bits_transpose_kernel 42 VGPRs / 60 SGPRs (the 64 ballots unrolled),
// prune_count_kernel 14 / 26 and 16 bytes of LDS, prune_decide_kernel 6 / 19 and 4 bytes of LDS; 8 waves per SIMD, no
// scratch and no spill in any of them.
#pragma once

#include "relax_prep_graph.h"

namespace topolow {

// stop_reason of a pruning attempt (topolow_prune_info); 0 while the rounds go on
constexpr int kPruneConverged = 1, kPruneMinPoints = 2, kPruneMaxIterations = 3, kPruneAllRemoved = 4;

struct PruneState {
  int32_t size;                     // points alive
  int32_t iteration;                // rounds decided: counted before the test, as the reference counts
  int32_t stopped;                  // 0, or the reason the rounds ended on the device
  int32_t n_remove;                 // this round's flagged lines; zero between rounds
  unsigned long long cells;         // this round's sum of counts; zero between rounds
  unsigned long long final_cells;   // the sum of counts of the round that stopped
  int32_t last_remove;              // n_remove of the last round decided
  int32_t reserved;
};

// out (m x words) = the transpose of bits (m x words) as an m x m bit matrix.  One wave per 64 x 64 tile (tr, tc): lane k
// holds word tc of line tr * 64 + k; bit j of every lane, gathered by a ballot, is word tr of line tc * 64 + j.  Lines
// and bits past m are 0 in the input (graph_bits_kernel) and are neither read nor written as lines here.
__global__ __launch_bounds__(kGraphThreads) void prune_bits_transpose_kernel(
    const unsigned long long* __restrict__ bits, int m, int words, unsigned long long* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long tile = (long long)blockIdx.x * kGraphWaves + (threadIdx.x >> 6);
  if (tile >= (long long)words * (long long)words) return;   // uniform over the wave
  const int tr = (int)(tile / words), tc = (int)(tile % words);
  const int src_line = tr * 64 + lane;
  const unsigned long long word = src_line < m ? bits[(size_t)src_line * (size_t)words + (size_t)tc] : 0ull;
  unsigned long long mine = 0ull;
  for (int j = 0; j < 64; ++j) {
    const unsigned long long column = __ballot((word >> j) & 1ull);
    if (lane == j) mine = column;
  }
  const int dst_line = tc * 64 + lane;
  if (dst_line < m) out[(size_t)dst_line * (size_t)words + (size_t)tr] = mine;
}

// One wave per line l < m.  alive: `words` words, bit c set while point c is kept (no bit past m).  A line that is not
// alive counts nothing and is not flagged.  counts: m entries or nullptr.
__global__ __launch_bounds__(kGraphThreads) void prune_count_kernel(
    const unsigned long long* __restrict__ bits, int m, int words, const unsigned long long* __restrict__ alive,
    int min_connections, uint8_t* __restrict__ flag, int32_t* __restrict__ counts, PruneState* st) {
  __shared__ unsigned int block_remove;
  __shared__ unsigned long long block_cells;
  if (st->stopped != 0) return;                             // uniform over the grid: nobody writes it in this launch
  const int lane = threadIdx.x & 63;
  const int l = blockIdx.x * kGraphWaves + (threadIdx.x >> 6);
  if (threadIdx.x == 0) { block_remove = 0u; block_cells = 0ull; }
  __syncthreads();
  const bool live = l < m && ((alive[l >> 6] >> (l & 63)) & 1ull) != 0ull;   // uniform over the wave
  int count = 0;
  if (live) {
    for (int w0 = 0; w0 < words; w0 += 64) {
      const int wd = w0 + lane;
      if (wd < words) count += __popcll(bits[(size_t)l * (size_t)words + (size_t)wd] & alive[wd]);
    }
  }
  for (int off = 32; off > 0; off >>= 1) count += __shfl_down(count, off, 64);
  if (lane == 0 && l < m) {
    const bool poor = live && count < min_connections;
    flag[l] = poor ? 1 : 0;
    if (counts != nullptr) counts[l] = count;
    if (poor) atomicAdd(&block_remove, 1u);
    if (count > 0) atomicAdd(&block_cells, (unsigned long long)count);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (block_remove) atomicAdd(&st->n_remove, (int32_t)block_remove);
    if (block_cells) atomicAdd(&st->cells, block_cells);
  }
}

// One workgroup.  The reference's three-way test of a round (R/data_preprocessing.R:1384-1409), then -- only when points
// leave -- wave w clears the flagged lines of the words w, w + 4, ... of `alive`: a ballot of the 64 flags is the word
// to clear, and each word is written by one lane only.
__global__ __launch_bounds__(kGraphThreads) void prune_decide_kernel(
    int m, int words, int min_points, const uint8_t* __restrict__ flag, unsigned long long* __restrict__ alive,
    PruneState* st) {
  __shared__ int remove_now;
  if (threadIdx.x == 0) {
    remove_now = 0;
    if (st->stopped == 0) {
      const int32_t r = st->n_remove;
      st->iteration += 1;
      st->last_remove = r;
      if (r == 0) {
        st->stopped = kPruneConverged;
        st->final_cells = st->cells;
      } else if (st->size - r < min_points) {
        st->stopped = kPruneMinPoints;
        st->final_cells = st->cells;
      } else {
        remove_now = 1;
        st->size -= r;
        if (st->size == 0) { st->stopped = kPruneAllRemoved; st->final_cells = 0ull; }
      }
      st->n_remove = 0;
      st->cells = 0ull;
    }
  }
  __syncthreads();
  if (!remove_now) return;
  const int lane = threadIdx.x & 63;
  for (int wd = threadIdx.x >> 6; wd < words; wd += kGraphWaves) {   // uniform over the wave
    const int l = wd * 64 + lane;
    const unsigned long long leaving = __ballot(l < m && flag[l] != 0);
    if (lane == 0 && leaving != 0ull) alive[wd] &= ~leaving;
  }
}

}  // namespace topolow
