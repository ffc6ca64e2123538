// topolow_amd/csrc/relax_velocity.h -- kernel-weighted antigenic velocities of a finished map: the reference's
// compute_kernel_velocity (R/visualization.R:802-843) as one pairwise pass (host side: topolow_velocity.hip).
//
// For every row i, over the columns j of its PAST (t_j < t_i, strictly) that its exclusion bits leave eligible:
//   w_ij = exp(-(||x_i - x_j||^2 / (2 sx^2) + (t_i - t_j)^2 / (2 st^2)))
//   W_i  = sum_j w_ij        S_id = sum_j w_ij (x_id - x_jd) / (t_i - t_j)        V_id = S_id / W_i,  NaN when W_i is not > 0
// Everything is f64.
//
// The host sorts the points by time (stable, NaN last; equal times by coordinates, so that the order does not depend
// on the caller's; points equal in time and in every coordinate keep the caller's), so the past of row i is the
// column prefix [0, past[i]): past[i] = the number of points with a smaller time, 0 for a NaN time.  A tie is in no prefix and a NaN time is in
// none either, so the kernel compares no times at all: a pair counts iff j < past[i] and its exclusion bit is clear.
//
// ONE exp per pair, of the summed exponent, where the reference multiplies two.  The two forms agree to a few ulp
// of the weight (the bands are derived in tests/test_gpu_velocity.py) and can differ on whether a weight is EXACTLY
// 0 only where the summed exponent lies between about 700 and 760: there a product of two exps may still be a
// subnormal (or one factor may already have flushed) while the single exp has gone to 0, or the other way round.
// Below 700 both are normal numbers, above 760 both are 0.
//
// The reduction has no floating-point atomic and one fixed order.  A lane owns a row and walks the columns of one
// CHUNK (chunk_cols columns, a multiple of kVelTile) in ascending order, adding every pair's terms to its own
// registers; the chunk's W and S go to part[chunk][k][row]; velocity_combine_kernel adds a row's partials in chunk
// order.  The order of a row's additions so depends on n and chunk_cols alone -- not on the launch geometry, not on
// which rows share a workgroup -- and every call returns the same bits.  Two chunk widths group the additions
// differently and may differ in the last bits; the library's width is a function of n alone (topolow_velocity.hip).
#pragma once

#include "relax_common.h"

namespace topolow {

constexpr int kVelThreads = 256;   // rows of a workgroup: one per lane
constexpr int kVelTile = 64;       // columns staged in LDS at a time = the columns of one exclusion word

// One eligible pair.  col points at the pair's column in the staged tile: coordinate d at col[d * kVelTile], the time
// at col[DIM * kVelTile] -- every lane of a wave reads the same address, an LDS broadcast.  dt > 0 for every pair that
// gets here.  (w / dt) * dx is the reference's w * (dx / dt) with one division per pair in place of DIM.
template <int DIM>
__device__ __forceinline__ void vel_pair(const double* __restrict__ col, const double (&xi)[DIM], double ti, double hx,
                                         double ht, double& W, double (&S)[DIM]) {
  double dx[DIM];
  double d2 = 0.0;
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    dx[d] = xi[d] - col[d * kVelTile];
    d2 += dx[d] * dx[d];
  }
  const double dt = ti - col[DIM * kVelTile];
  const double w = ::exp(-(d2 * hx + dt * dt * ht));
  const double q = w / dt;
  W += w;
#pragma unroll
  for (int d = 0; d < DIM; ++d) S[d] += q * dx[d];
}

// Grid (ceil(n / kVelThreads), chunks): workgroup (b, c) adds columns [c * chunk_cols, (c + 1) * chunk_cols) to rows
// [b * kVelThreads, ...).  All arrays are in sorted order.
//   pos    DIM x n f64, coordinate d of point j at pos[d * n + j] (coordinates beyond the caller's ndim are 0)
//   times  n f64;  past  n i32, see above
//   bits   n x words u64 or nullptr (only when BITS): bit j of row i set = column j is excluded for row i
//   part   chunks x (DIM + 1) x n f64 out: part[(c * (DIM + 1) + d) * n + i] = S_id of chunk c, ... + DIM ... = W_i.
//          Workgroup (b, c) writes its rows' partials iff c * chunk_cols < past[i] for at least one of its rows --
//          exactly the partials velocity_combine_kernel reads.
// A tile that lies wholly inside the past of all 64 rows of a wave and has no exclusion bit set runs without a
// per-pair test; a tile beyond every row's past is not visited.
template <int DIM, bool BITS>
__global__ __launch_bounds__(kVelThreads) void velocity_partial_kernel(
    const double* __restrict__ pos, const double* __restrict__ times, const int32_t* __restrict__ past,
    const uint64_t* __restrict__ bits, int n, int words, int chunk_cols, double hx, double ht,
    double* __restrict__ part) {
  __shared__ double tile[(DIM + 1) * kVelTile];
  __shared__ int block_past;
  const int i = blockIdx.x * kVelThreads + threadIdx.x;
  const int c = blockIdx.y;
  const int c0 = c * chunk_cols;
  if (threadIdx.x == 0) block_past = 0;
  __syncthreads();
  const int my_past = i < n ? past[i] : 0;
  atomicMax(&block_past, my_past);
  __syncthreads();
  const int c1 = min(c0 + chunk_cols, block_past);   // the same in every lane of the workgroup
  if (c1 <= c0) return;

  double xi[DIM], S[DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    xi[d] = i < n ? pos[(size_t)d * n + i] : 0.0;
    S[d] = 0.0;
  }
  const double ti = i < n ? times[i] : 0.0;
  double W = 0.0;

  for (int j0 = c0; j0 < c1; j0 += kVelTile) {
    __syncthreads();   // every lane has finished with the tile before
    for (int idx = threadIdx.x; idx < (DIM + 1) * kVelTile; idx += kVelThreads) {
      const int k = idx / kVelTile, j = j0 + idx % kVelTile;
      tile[idx] = j < n ? (k < DIM ? pos[(size_t)k * n + j] : times[j]) : 0.0;
    }
    __syncthreads();
    const int cols = min(kVelTile, c1 - j0);
    const int mine = my_past - j0;   // this row's past reaches `mine` columns into the tile (<= 0: none)
    uint64_t excl = 0;
    if (BITS && mine > 0) excl = bits[(size_t)i * words + (j0 >> 6)];   // j0 is a multiple of 64
    if (__all(mine >= cols && excl == 0)) {
      for (int jj = 0; jj < cols; ++jj) vel_pair<DIM>(tile + jj, xi, ti, hx, ht, W, S);
    } else {
      for (int jj = 0; jj < cols; ++jj)
        if (jj < mine && ((excl >> jj) & 1) == 0) vel_pair<DIM>(tile + jj, xi, ti, hx, ht, W, S);
    }
  }
  if (i < n) {
    double* out = part + (size_t)c * (DIM + 1) * n + i;
#pragma unroll
    for (int d = 0; d < DIM; ++d) out[(size_t)d * n] = S[d];
    out[(size_t)DIM * n] = W;
  }
}

// One lane per sorted row: its partials added in chunk order -- chunks [0, ceil(past[i] / chunk_cols)), the ones that
// were written -- then the quotient, scattered to the caller's order (row i is the caller's row perm[i]).
//   stride  DIM + 1 of the partial kernel;  velocity  n x ndim out, column-major;  weight_sum  n out
__global__ __launch_bounds__(kVelThreads) void velocity_combine_kernel(
    const double* __restrict__ part, const int32_t* __restrict__ past, const int32_t* __restrict__ perm, int n, int ndim,
    int stride, int chunk_cols, double* __restrict__ velocity, double* __restrict__ weight_sum) {
  const int i = blockIdx.x * kVelThreads + threadIdx.x;
  if (i >= n) return;
  const int chunks = (past[i] + chunk_cols - 1) / chunk_cols;
  const size_t plane = (size_t)stride * n;
  double W = 0.0;
  for (int c = 0; c < chunks; ++c) W += part[(size_t)c * plane + (size_t)(stride - 1) * n + i];
  const size_t o = (size_t)perm[i];
  weight_sum[o] = W;
  for (int d = 0; d < ndim; ++d) {
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += part[(size_t)c * plane + (size_t)d * n + i];
    velocity[(size_t)d * n + o] = W > 0.0 ? s / W : __builtin_nan("");
  }
}

}  // namespace topolow
