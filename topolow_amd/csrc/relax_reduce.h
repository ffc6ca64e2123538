// topolow_amd/csrc/relax_reduce.h -- the objective of the reference's scale_to_original_distances
// (R/visualization.R:624-640) as one pairwise pass over the coordinates (host side: topolow_reduce.hip).
//
// For positions X (n x ndim), reduced coordinates Y (n x k) and scales s_0 .. s_{m-1}, with d_ij = ||x_i - x_j|| and
// r_ij = ||y_i - y_j||:
//   F(s) = sum_{i != j} |d_ij - s r_ij|        G = sum_{i != j} d_ij        H = sum_{i != j} r_ij
// The reference forms both n x n distance matrices and sums over them; here no matrix exists.  Only the pairs j < i
// are visited and the sums are doubled at the end, which is exact.  Everything is f64: two square roots per pair,
// shared by all m scales, and per scale one fused multiply-add and one addition -- |fma(-s, r, d)|, written as an
// fma so that every instance of the kernel rounds a pair's term the same way.
//
// The triangle is cut into UNITS: unit (b, c) adds the columns [c * chunk_cols, (c + 1) * chunk_cols) to the rows
// [b * kRedThreads, ...), and only the units that hold a pair j < i exist -- the host lists them (reduce_units) and
// the grid is that list, so no workgroup is launched over the empty half.  A unit on the diagonal stops at its last
// row's column; among the units of a launch only those (one per row block) do less than a full unit's work.
//
// The reduction has no floating-point atomic and one fixed order.  A lane owns a row and walks its unit's columns in
// ascending order; the 256 lanes of the workgroup are added by a fixed tree in LDS; the unit's m + 2 sums go to
// part[unit]; scale_objective_combine_kernel adds the units' partials in list order (lane t the units t, t + 256,
// ..., then the same tree).  The order so depends on n and chunk_cols alone and every call returns the same bits.
// Two chunk widths group the additions differently and may differ in the last bits.
#pragma once

#include "relax_common.h"

namespace topolow {

constexpr int kRedThreads = 256;   // rows of a workgroup: one per lane
constexpr int kRedTile = 64;       // columns staged in LDS at a time
constexpr int kRedMaxScales = 8;

struct ReduceScales {
  double s[kRedMaxScales];
};

// One pair.  col points at the pair's column in the staged tile: coordinate d of X at col[d * kRedTile], coordinate d
// of Y at col[(DIM + d) * kRedTile] -- every lane of a wave reads the same address, an LDS broadcast.
template <int DIM, int KDIM, int M>
__device__ __forceinline__ void red_pair(const double* __restrict__ col, const double (&xi)[DIM], const double (&yi)[KDIM],
                                         const double (&s)[M], double (&F)[M], double& G, double& H) {
  double d2 = 0.0, r2 = 0.0;
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    const double dx = xi[d] - col[d * kRedTile];
    d2 += dx * dx;
  }
#pragma unroll
  for (int d = 0; d < KDIM; ++d) {
    const double dy = yi[d] - col[(DIM + d) * kRedTile];
    r2 += dy * dy;
  }
  const double dist = ::sqrt(d2), red = ::sqrt(r2);
  G += dist;
  H += red;
#pragma unroll
  for (int q = 0; q < M; ++q) F[q] += ::fabs(::fma(-s[q], red, dist));
}

// The 256 lanes' NV values, each added over the lanes in one fixed tree; the sums stand in v of lane 0 (other
// lanes: partials of no use).  scratch holds NV x kRedThreads doubles.
template <int NV>
__device__ __forceinline__ void red_block_sums(double (&v)[NV], double* __restrict__ scratch) {
#pragma unroll
  for (int q = 0; q < NV; ++q) scratch[q * kRedThreads + threadIdx.x] = v[q];
  __syncthreads();
  for (int w = kRedThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
#pragma unroll
      for (int q = 0; q < NV; ++q) scratch[q * kRedThreads + threadIdx.x] += scratch[q * kRedThreads + threadIdx.x + w];
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < NV; ++q) v[q] = scratch[q * kRedThreads];
}

// Grid (units): workgroup u takes units[u] = (b, c).
//   pos    DIM x n f64, coordinate d of point j at pos[d * n + j] (coordinates beyond the caller's ndim are 0)
//   red    KDIM x n f64, likewise (coordinates beyond the caller's k are 0: they add exactly 0 to r^2)
//   units  the list of reduce_units (topolow_reduce.hip): every (b, c) with c * chunk_cols < the last row of block b
//   part   units x (M + 2) f64 out: F_0 .. F_{M-1}, G, H of the unit, over its pairs j < i, not doubled
// Row i takes the columns j < i.  A tile that lies wholly below all 64 rows of a wave runs without a per-pair test.
template <int DIM, int KDIM, int M>
__global__ __launch_bounds__(kRedThreads) void scale_objective_partial_kernel(
    const double* __restrict__ pos, const double* __restrict__ red, const int2* __restrict__ units, int n,
    int chunk_cols, ReduceScales scales, double* __restrict__ part) {
  __shared__ double tile[(DIM + KDIM) * kRedTile];
  __shared__ double scratch[(M + 2) * kRedThreads];
  const int2 unit = units[blockIdx.x];
  const int i = unit.x * kRedThreads + threadIdx.x;
  const int c0 = unit.y * chunk_cols;
  const int last_row = min((unit.x + 1) * kRedThreads, n) - 1;   // the same in every lane of the workgroup
  const int c1 = min(c0 + chunk_cols, last_row);                 // columns j < last_row: c1 <= n - 1
  const int my_cols = i < n ? i : 0;                             // row i takes the columns [0, i)

  double xi[DIM], yi[KDIM], s[M], F[M];
#pragma unroll
  for (int d = 0; d < DIM; ++d) xi[d] = i < n ? pos[(size_t)d * n + i] : 0.0;
#pragma unroll
  for (int d = 0; d < KDIM; ++d) yi[d] = i < n ? red[(size_t)d * n + i] : 0.0;
#pragma unroll
  for (int q = 0; q < M; ++q) {
    s[q] = scales.s[q];
    F[q] = 0.0;
  }
  double G = 0.0, H = 0.0;

  for (int j0 = c0; j0 < c1; j0 += kRedTile) {
    __syncthreads();   // every lane has finished with the tile before
    for (int idx = threadIdx.x; idx < (DIM + KDIM) * kRedTile; idx += kRedThreads) {
      const int k = idx / kRedTile, j = j0 + idx % kRedTile;
      tile[idx] = j < n ? (k < DIM ? pos[(size_t)k * n + j] : red[(size_t)(k - DIM) * n + j]) : 0.0;
    }
    __syncthreads();
    const int cols = min(kRedTile, c1 - j0);
    const int mine = my_cols - j0;   // this row reaches `mine` columns into the tile (<= 0: none)
    if (__all(mine >= cols)) {
      for (int jj = 0; jj < cols; ++jj) red_pair<DIM, KDIM, M>(tile + jj, xi, yi, s, F, G, H);
    } else {
      for (int jj = 0; jj < cols; ++jj)
        if (jj < mine) red_pair<DIM, KDIM, M>(tile + jj, xi, yi, s, F, G, H);
    }
  }

  double sums[M + 2];
#pragma unroll
  for (int q = 0; q < M; ++q) sums[q] = F[q];
  sums[M] = G;
  sums[M + 1] = H;
  red_block_sums<M + 2>(sums, scratch);
  if (threadIdx.x == 0) {
    double* out = part + (size_t)blockIdx.x * (M + 2);
#pragma unroll
    for (int q = 0; q < M + 2; ++q) out[q] = sums[q];
  }
}

// One workgroup: the units' partials added in list order, doubled (pairs j < i stand for both orders).
//   stride  M + 2 of the partial kernel;  m  the caller's scales (<= M)
//   out     m + 2 f64: F_0 .. F_{m-1}, G, H
__global__ __launch_bounds__(kRedThreads) void scale_objective_combine_kernel(const double* __restrict__ part, int units,
                                                                              int stride, int m,
                                                                              double* __restrict__ out) {
  __shared__ double scratch[kRedThreads];
  for (int q = 0; q < m + 2; ++q) {
    const int src = q < m ? q : stride - 2 + (q - m);
    double v[1] = {0.0};
    for (int u = threadIdx.x; u < units; u += kRedThreads) v[0] += part[(size_t)u * stride + src];
    __syncthreads();   // the scratch of the sum before has been read
    red_block_sums<1>(v, scratch);
    if (threadIdx.x == 0) out[q] = 2.0 * v[0];
  }
}

}  // namespace topolow
