// topolow_amd/csrc/relax_prep_graph.h -- the measurement graph of a resident matrix and its sub-handles
// (reference R/utils.R:199-253 check_matrix_connectivity over R/diagnostics.R:442-468, R/utils.R:321-463
// subsample_dissimilarity_matrix; host pipeline: topolow_layout_prep_connectivity / _subsample in topolow_prep_graph.hip).
//
// Two kernel groups.  Both work in BUFFER coordinates, as relax_prep.h does: B[a * n + b], a the slow index.  The graph
// takes either cell of a pair, so it is the same graph in either layout and no transposed read is made.
//
// (1) Components.  Vertices are the positions 0..m-1 of `sub` (nullptr: the identity, m = n).  graph_bits_kernel reads
// the matrix once and leaves one bit per cell of the induced submatrix; the rounds then read m^2 / 8 bytes, not 8 m^2.
// parent[] is a forest with parent[q] <= q throughout: a value is only ever replaced by a smaller position of the same
// component, so there is no cycle and a walk towards a root takes fewer than m steps.  A round is
//   graph_jump_kernel   every parent[q] becomes the root of q's tree (pointer jumping, to the end of the path);
//   graph_hook_kernel   every set bit (l, c) whose ends have different roots hooks the larger root to the smaller
//                       (atomicMin on the larger root's entry) and raises `changed`.
// The host launches rounds until one raises nothing; the trees are then flat, every edge lies inside one tree, and a
// root, being <= every member, is the smallest position of its component: the canonical label.  No kernel waits for
// another thread: every loop is bounded by m and makes progress on its own.
//
// (2) graph_gather_kernel: lines [a0, a0 + lines) of child = parent[sub, sub], values and codes, device to device.
#pragma once

#include "relax_common.h"

namespace topolow {

constexpr int kGraphThreads = 256;
constexpr int kGraphWaves = kGraphThreads / 64;

// One workgroup per line l of the submatrix; wave w takes the 64-bit words w, w + 4, ... of the line.  Lane k of word
// wd reads cell (sub[l], sub[wd * 64 + k]); the wave's ballot is the word.  Cells past m are 0, the diagonal is 0.
//   bits     m x words
//   first    m: min(l, the smallest c with bit (l, c)) -- the forest the rounds start from
//   n_cells  += the set bits (non-NaN off-diagonal cells, both triangles)
__global__ __launch_bounds__(kGraphThreads) void graph_bits_kernel(
    const double* __restrict__ vals, int n, const int32_t* __restrict__ sub, int m, int words,
    unsigned long long* __restrict__ bits, int32_t* __restrict__ first, unsigned long long* __restrict__ n_cells) {
  __shared__ int32_t line_first;
  __shared__ unsigned int line_cells;
  const int l = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) { line_first = l; line_cells = 0u; }
  __syncthreads();
  const size_t src = (size_t)(sub != nullptr ? sub[l] : l) * (size_t)n;
  int32_t lowest = l;
  unsigned int cells = 0;
  for (int wd = wave; wd < words; wd += kGraphWaves) {   // uniform over the wave
    const int c = wd * 64 + lane;
    bool measured = false;
    if (c < m && c != l) measured = !__builtin_isnan(vals[src + (size_t)(sub != nullptr ? sub[c] : c)]);
    const unsigned long long word = __ballot(measured);
    if (lane == 0) {
      bits[(size_t)l * (size_t)words + (size_t)wd] = word;
      if (word != 0ull) {
        const int32_t c0 = wd * 64 + (__ffsll((long long)word) - 1);
        lowest = c0 < lowest ? c0 : lowest;
        cells += (unsigned int)__popcll(word);
      }
    }
  }
  if (lane == 0) {
    if (lowest < l) atomicMin(&line_first, lowest);
    if (cells) atomicAdd(&line_cells, cells);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    first[l] = line_first;
    if (line_cells) atomicAdd(n_cells, (unsigned long long)line_cells);
  }
}

// parent[q] <- the root of q's tree.  parent[x] < x for every x that is no root, so the walk ends within m steps;
// a root is written by nobody during this kernel, so what the walk ends on is still a root when the kernel ends.
__global__ __launch_bounds__(kGraphThreads) void graph_jump_kernel(int32_t* parent, int m) {
  const int q = blockIdx.x * kGraphThreads + threadIdx.x;
  if (q >= m) return;
  int32_t r = parent[q];
  for (int step = 0; step < m; ++step) {
    const int32_t up = parent[r];
    if (up == r) break;
    r = up;
  }
  parent[q] = r;
}

// One wave per line l, lanes over its words, a lane over the set bits of its word.  For the bit (l, c) with roots
// pl = parent[l] and pc = parent[c]: pc > pl hooks pc under pl at once; the smallest pc < pl of the line hooks pl.
// A bit found in line l links l and c whichever triangle its cell came from, so line c need not hold the mirror.
// Early rounds have a handful of large trees, so most bits of a line name the same few roots: a lane hooks a root it
// hooked last only once, and asks the entry itself (a load that L2 answers, not this CU's cache) before it sends an
// atomic that would change nothing -- otherwise millions of atomics queue on two or three addresses.  Any bit whose
// ends differ raises `changed`, whoever does the hooking.
__device__ inline void graph_hook(int32_t* parent, int32_t hi, int32_t lo) {
  if (__hip_atomic_load(&parent[hi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > lo) atomicMin(&parent[hi], lo);
}

__global__ __launch_bounds__(kGraphThreads) void graph_hook_kernel(
    const unsigned long long* __restrict__ bits, int m, int words, int32_t* parent, int32_t* __restrict__ changed) {
  const int lane = threadIdx.x & 63;
  const int l = blockIdx.x * kGraphWaves + (threadIdx.x >> 6);
  if (l >= m) return;                                     // uniform over the wave
  const int32_t pl = parent[l];
  int32_t lowest = pl, last = pl;
  bool differ = false;
  for (int w0 = 0; w0 < words; w0 += 64) {
    const int wd = w0 + lane;
    unsigned long long word = wd < words ? bits[(size_t)l * (size_t)words + (size_t)wd] : 0ull;
    while (word != 0ull) {
      const int c = wd * 64 + (__ffsll((long long)word) - 1);   // < m: graph_bits_kernel set no bit past m
      word &= word - 1ull;
      const int32_t pc = parent[c];
      if (pc == pl) continue;
      differ = true;
      if (pc < pl) {
        lowest = pc < lowest ? pc : lowest;
      } else if (pc != last) {
        graph_hook(parent, pc, pl);
        last = pc;
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const int32_t other = __shfl_down(lowest, off, 64);
    lowest = other < lowest ? other : lowest;
  }
  if (lane == 0 && lowest < pl) graph_hook(parent, pl, lowest);
  if (differ) *changed = 1;
}

// child[a][b] = parent[sub[a]][sub[b]] for the lines a0 <= a < a0 + gridDim.x of the child's buffer (m x m), in the
// parent's own layout; sub == nullptr: the identity.  One workgroup per line: the source line sub[a] is contiguous,
// the lanes gather within it and store to consecutive addresses.
__global__ __launch_bounds__(kGraphThreads) void graph_gather_kernel(
    const double* __restrict__ vals, const int8_t* __restrict__ codes, int n, const int32_t* __restrict__ sub, int m,
    int a0, double* __restrict__ out_vals, int8_t* __restrict__ out_codes) {
  const int a = a0 + blockIdx.x;
  if (a >= m) return;
  const size_t src = (size_t)(sub != nullptr ? sub[a] : a) * (size_t)n, dst = (size_t)a * (size_t)m;
  for (int b = threadIdx.x; b < m; b += kGraphThreads) {
    const size_t cell = src + (size_t)(sub != nullptr ? sub[b] : b);
    out_vals[dst + b] = vals[cell];
    if (codes != nullptr) out_codes[dst + b] = codes[cell];
  }
}

}  // namespace topolow
