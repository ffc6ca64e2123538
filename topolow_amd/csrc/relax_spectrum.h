// topolow_amd/csrc/relax_spectrum.h -- the data assessment of the reference's Euclidify() (R/core.R:983-1007) on the
// device: the median of the numeric cells, the double-centred matrix B = -0.5 J D^2 J of the median-filled matrix, and
// all eigenvalues of a symmetric f64 matrix by Householder tridiagonalisation and Sturm bisection
// (host pipeline: topolow_layout_prep_spectrum / topolow_symmetric_eigenvalues / topolow_tridiagonal_eigenvalues in
// topolow_spectrum.hip; NumPy model of the same algorithm: tests/models/spectrum_model.py).
//
// As relax_prep.h, every matrix kernel works in BUFFER coordinates, B[a * n + b] with b the contiguous index.
// Nothing here adds floating-point numbers in an order that depends on the grid or on timing: histograms are integer
// atomics, every floating-point reduction has fixed partitions added in a fixed order.
#pragma once

#include "relax_prep_device.h"

namespace topolow {

constexpr int kSpecThreads = 256;          // the streaming kernels: one column per thread
constexpr int kSpecStepThreads = 1024;     // the one-workgroup step kernel
constexpr int kSpecLineBlock = 64;         // lines of the trailing matrix per workgroup of the streaming kernel
constexpr int kSpecSumThreads = 64;        // the kernel that adds a column's partials
constexpr int kSpecBisectThreads = 64;

// ---- 1. median of the numeric cells: radix select over prep_order_key ---------------------------------------------
struct SpecSelect {
  unsigned long long hist[2][256];   // [r]: digit counts of the keys that share rank r's prefix
  unsigned long long n_infinite;     // first pass: numeric cells that are +-Inf
};

// A numeric cell (as.numeric form): code 0 and not NaN.
__device__ inline bool spec_numeric(const double* __restrict__ vals, const int8_t* __restrict__ codes, size_t cell,
                                    double& v) {
  v = vals[cell];
  return !__builtin_isnan(v) && (codes == nullptr || codes[cell] == 0);
}

// One pass of the select: the digit (key >> shift) & 255 of every numeric cell whose key agrees with prefix0 (hist[0])
// / prefix1 (hist[1]) in the bits above the digit; shift = 56 (no bits above: every numeric cell counts), 48, ..., 0.
// Counts go to LDS first, one global integer add per (workgroup, digit) that is not 0.
__global__ __launch_bounds__(kSpecThreads) void spec_select_kernel(
    const double* __restrict__ vals, const int8_t* __restrict__ codes, size_t cells, int shift,
    unsigned long long prefix0, unsigned long long prefix1, SpecSelect* __restrict__ out) {
  __shared__ unsigned int h[2][256];
  h[0][threadIdx.x] = 0;
  h[1][threadIdx.x] = 0;
  __syncthreads();
  const bool first = shift == 56;
  const unsigned long long p0 = first ? 0ull : prefix0 >> (shift + 8), p1 = first ? 0ull : prefix1 >> (shift + 8);
  unsigned long long n_inf = 0;
  for (size_t c = (size_t)blockIdx.x * kSpecThreads + threadIdx.x; c < cells; c += (size_t)gridDim.x * kSpecThreads) {
    double v;
    if (!spec_numeric(vals, codes, c, v)) continue;
    if (first && __builtin_isinf(v)) ++n_inf;
    const unsigned long long key = prep_order_key(v);
    const unsigned int digit = (unsigned int)(key >> shift) & 255u;
    const unsigned long long above = first ? 0ull : key >> (shift + 8);
    if (above == p0) atomicAdd(&h[0][digit], 1u);
    if (above == p1) atomicAdd(&h[1][digit], 1u);
  }
  __syncthreads();
  if (h[0][threadIdx.x]) atomicAdd(&out->hist[0][threadIdx.x], (unsigned long long)h[0][threadIdx.x]);
  if (h[1][threadIdx.x]) atomicAdd(&out->hist[1][threadIdx.x], (unsigned long long)h[1][threadIdx.x]);
  if (first) prep_flush(&out->n_infinite, n_inf);
}

// ---- 2. the centred matrix -----------------------------------------------------------------------------------------
// x = the cell where it is numeric, otherwise the median; D2 = x * x.  The sums of D2 along both directions by the
// first pass's rule (relax_prep_device.h: prep_tile_sums): one partial per (point, block of 64 cells), the cells added in
// index order from 0.0 -- here every cell counts, the diagonal too.
__global__ __launch_bounds__(kPrepThreads) void spec_square_sums_kernel(
    const double* __restrict__ vals, const int8_t* __restrict__ codes, int n, double median,
    double* __restrict__ part_slow, double* __restrict__ part_fast) {
  __shared__ double tile[kPrepTile][kPrepTile + 1];
  const int tb = blockIdx.x, ta = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = tb * kPrepTile + lane;
  for (int r = wave; r < kPrepTile; r += kPrepWaves) {
    const int a = ta * kPrepTile + r;
    double x = 0.0;
    if (a < n && b < n) {
      double v;
      x = spec_numeric(vals, codes, (size_t)a * (size_t)n + (size_t)b, v) ? v : median;
      x = __dmul_rn(x, x);
    }
    tile[r][lane] = x;
  }
  __syncthreads();
  if (wave == 0) {
    const int p = ta * kPrepTile + lane;
    if (p < n) {
      double s = 0.0;
      for (int q = 0; q < kPrepTile; ++q) s += tile[lane][q];
      part_slow[(size_t)tb * n + p] = s;
    }
  } else if (wave == 1) {
    if (b < n) {
      double s = 0.0;
      for (int q = 0; q < kPrepTile; ++q) s += tile[q][lane];
      part_fast[(size_t)ta * n + b] = s;
    }
  }
}

// One thread per point: its partials added in block order.  out is 2 x n: slow lines, then fast lines.
__global__ __launch_bounds__(kPrepThreads) void spec_finish_sums_kernel(
    int n, int n_blocks, const double* __restrict__ part_slow, const double* __restrict__ part_fast,
    double* __restrict__ out) {
  const int q = blockIdx.x * kPrepThreads + threadIdx.x;
  if (q >= n) return;
  double ss = 0.0, fs = 0.0;
  for (int blk = 0; blk < n_blocks; ++blk) {
    ss += part_slow[(size_t)blk * n + q];
    fs += part_fast[(size_t)blk * n + q];
  }
  out[q] = ss;
  out[(size_t)n + q] = fs;
}

// B = -0.5 (D2 - r_i - c_j + g), evaluated as ((D2 - r_i) - c_j) + g with the ROW mean first in either layout, so a
// matrix handed over row-major and the same matrix handed over column-major give the same bits.  means: 2 x n, slow
// lines then fast lines.  Grid: (n lines, column chunks of kSpecThreads).
__global__ __launch_bounds__(kSpecThreads) void spec_center_kernel(
    const double* __restrict__ vals, const int8_t* __restrict__ codes, int n, double median,
    const double* __restrict__ means, double grand, int row_is_slow, double* __restrict__ B) {
  const int a = blockIdx.x, b = blockIdx.y * kSpecThreads + threadIdx.x;
  if (a >= n || b >= n) return;
  const size_t cell = (size_t)a * (size_t)n + (size_t)b;
  double v;
  const double x = spec_numeric(vals, codes, cell, v) ? v : median;
  const double sm = means[a], fm = means[(size_t)n + b];
  const double r = row_is_slow ? sm : fm, c = row_is_slow ? fm : sm;
  B[cell] = -0.5 * (((__dmul_rn(x, x) - r) - c) + grand);
}

// The diagonal of B, for the trace.
__global__ __launch_bounds__(kSpecThreads) void spec_diagonal_kernel(const double* __restrict__ B, int n,
                                                                     double* __restrict__ diag) {
  const int q = blockIdx.x * kSpecThreads + threadIdx.x;
  if (q < n) diag[q] = B[(size_t)q * n + q];
}

// The eigenvalue solve reads the matrix's lower triangle only: every cell of the upper triangle takes its mirror's
// bits.  upper_a_lt_b as prep_dense_kernel: != 0 for a row-major buffer.  Cells that are read are never written.
__global__ __launch_bounds__(kSpecThreads) void spec_mirror_kernel(double* __restrict__ B, int n, int upper_a_lt_b) {
  const int a = blockIdx.x, b = blockIdx.y * kSpecThreads + threadIdx.x;
  if (a >= n || b >= n) return;
  if (upper_a_lt_b ? a < b : b < a) B[(size_t)a * n + b] = B[(size_t)b * n + a];
}

// ---- 3. Householder tridiagonalisation of a symmetric matrix held in full ----------------------------------------------
// Unblocked, one reflection per column, three launches per step k = 0 .. n - 2 on one stream:
//   spec_step_kernel(k)    one workgroup: finishes w of reflection k - 1 from y, brings line k (= column k: the matrix
//                          stays symmetric bit for bit) up to date, leaves d[k], forms reflection k and e[k]
//   spec_stream_kernel(k)  the trailing matrix [k + 1, n)^2, once: applies the pending rank-2 update of reflection k - 1
//                          and, in the same read, accumulates y = A v of reflection k into one partial per column and
//                          block of kSpecLineBlock lines
//   spec_sum_kernel(k)     y = a column's partials added in block order
// Short blocks of lines keep a workgroup's chain of dependent round trips short and the grid wider than the chip until
// the trailing matrix is a few hundred lines; the price is the third launch, which moves 1/64 of the step's bytes.
// With H = I - beta v v^T:  p = beta A v,  K = beta (p . v) / 2,  w = p - K v,  A <- A - v w^T - w v^T.
// v and w are indexed by the absolute point; reflection k lives on [k + 1, n).  A zero sub-column takes no reflection:
// beta = 0 and v = 0, so the update it leaves pending changes nothing.

// Sum of red[0 .. kSpecStepThreads) in a fixed tree; every thread returns with the total.
__device__ inline double spec_block_sum(double* red, double x) {
  __syncthreads();   // whoever still reads the last total
  red[threadIdx.x] = x;
  __syncthreads();
  for (int s = kSpecStepThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// scal[0]: beta of the reflection in v_prev on entry, of the one in v_new on return.  y = A v_prev on [k, n).
__global__ __launch_bounds__(kSpecStepThreads) void spec_step_kernel(
    const double* __restrict__ A, int n, int k, const double* __restrict__ v_prev, double* __restrict__ v_new,
    double* __restrict__ w, const double* __restrict__ y, double* __restrict__ scal, double* __restrict__ d,
    double* __restrict__ e) {
  __shared__ double red[kSpecStepThreads];
  __shared__ double s_wk, s_vk, s_x0;
  const int tid = threadIdx.x;
  const double beta = scal[0];
  // w of reflection k - 1 on [k, n): p into w first, then K, then w = p - K v.  Thread t owns points k + t, k + t + 1024, ..
  double pv = 0.0;
  for (int i = k + tid; i < n; i += kSpecStepThreads) {
    const double p = beta * y[i];
    w[i] = p;
    pv += p * v_prev[i];
  }
  const double K = 0.5 * beta * spec_block_sum(red, pv);
  for (int i = k + tid; i < n; i += kSpecStepThreads) {
    const double vi = v_prev[i], wi = w[i] - K * vi;
    w[i] = wi;
    if (i == k) { s_wk = wi; s_vk = vi; }
  }
  __syncthreads();
  // line k of the matrix with reflection k - 1 applied: d[k], and x = its part on [k + 1, n), kept in v_new
  const double wk = s_wk, vk = s_vk;
  double tail = 0.0;
  for (int i = k + tid; i < n; i += kSpecStepThreads) {
    const double x = A[(size_t)k * n + i] - __dadd_rn(__dmul_rn(vk, w[i]), __dmul_rn(wk, v_prev[i]));
    if (i == k) { d[k] = x; continue; }
    v_new[i] = x;
    if (i == k + 1) s_x0 = x;
    else tail += x * x;
  }
  if (k + 1 >= n) {   // n == 1
    if (tid == 0) scal[0] = 0.0;
    return;
  }
  const double tail2 = spec_block_sum(red, tail);   // its barriers publish s_x0 too
  const double x0 = s_x0;
  if (k == n - 2 || tail2 == 0.0) {
    // nothing below the sub-diagonal: no reflection
    for (int i = k + 1 + tid; i < n; i += kSpecStepThreads) v_new[i] = 0.0;
    if (tid == 0) {
      e[k] = x0;
      scal[0] = 0.0;
      if (k == n - 2) {
        const double t = __dmul_rn(v_prev[n - 1], w[n - 1]);
        d[n - 1] = A[(size_t)(n - 1) * n + (n - 1)] - __dadd_rn(t, t);
      }
    }
    return;
  }
  if (tid == 0) {
    const double alpha = -copysign(sqrt(x0 * x0 + tail2), x0);
    const double v0 = x0 - alpha;
    e[k] = alpha;
    v_new[k + 1] = v0;
    scal[0] = 2.0 / (v0 * v0 + tail2);
  }
}

// Grid: (column chunks that reach into [k + 1, n), line blocks that do).  Thread = one column b; the lines of its block
// in index order.  part[block * n + b] = sum over the block's lines a of A_new[a][b] v_new[a].
__global__ __launch_bounds__(kSpecThreads) void spec_stream_kernel(
    double* __restrict__ A, int n, int k, const double* __restrict__ v_prev, const double* __restrict__ w,
    const double* __restrict__ v_new, double* __restrict__ part) {
  const int first = k + 1;
  const int b = (first / kSpecThreads + (int)blockIdx.x) * kSpecThreads + (int)threadIdx.x;
  const int blk = first / kSpecLineBlock + (int)blockIdx.y;
  const int a_lo = max(first, blk * kSpecLineBlock), a_hi = min(n, (blk + 1) * kSpecLineBlock);
  if (b < first || b >= n) return;
  const double vb = v_prev[b], wb = w[b];
  double acc = 0.0;
#pragma unroll 8
  for (int a = a_lo; a < a_hi; ++a) {
    const size_t cell = (size_t)a * (size_t)n + (size_t)b;
    const double x = A[cell] - __dadd_rn(__dmul_rn(v_prev[a], wb), __dmul_rn(w[a], vb));
    A[cell] = x;
    acc += x * v_new[a];
  }
  part[(size_t)blk * n + b] = acc;
}

// y[b] on [k + 1, n): the partials of column b over the line blocks that reach into [k + 1, n), in block order.
__global__ __launch_bounds__(kSpecSumThreads) void spec_sum_kernel(int n, int k, const double* __restrict__ part,
                                                                   double* __restrict__ y) {
  const int first = k + 1;
  const int b = first + (int)blockIdx.x * kSpecSumThreads + (int)threadIdx.x;
  if (b >= n) return;
  double s = 0.0;
  for (int blk = first / kSpecLineBlock; blk <= (n - 1) / kSpecLineBlock; ++blk) s += part[(size_t)blk * n + b];
  y[b] = s;
}

// ---- 4. eigenvalues of a symmetric tridiagonal matrix by bisection -------------------------------------------------
// count(x) = the number of eigenvalues below x, by the Sturm sequence with LAPACK dstebz's pivmin guard.  Thread j
// bisects [lo, hi] (the widened Gershgorin interval) for the j-th smallest eigenvalue until the interval is no wider
// than 2 u max(|lo|, |hi|) + pivmin, and writes it at out[n - 1 - j]: descending order.  e2[i] = e[i]^2.  An interval
// that ends within the guard's own resolution of zero is reported as 0.
__global__ __launch_bounds__(kSpecBisectThreads) void spec_bisect_kernel(
    const double* __restrict__ d, const double* __restrict__ e2, int n, double lo0, double hi0, double pivmin,
    double* __restrict__ out) {
  const int j = blockIdx.x * kSpecBisectThreads + threadIdx.x;
  if (j >= n) return;
  double lo = lo0, hi = hi0;
  for (int it = 0; it < 2200; ++it) {   // an f64 interval halves at most ~2100 times before mid meets an end
    const double width = hi - lo;
    if (width <= 0x1p-51 * fmax(fabs(lo), fabs(hi)) + pivmin) break;
    const double mid = 0.5 * lo + 0.5 * hi;
    if (!(mid > lo && mid < hi)) break;
    double q = d[0] - mid;
    if (fabs(q) < pivmin) q = -pivmin;
    int count = q < 0.0 ? 1 : 0;
    for (int i = 1; i < n; ++i) {
      q = d[i] - mid - e2[i - 1] / q;
      if (fabs(q) < pivmin) q = -pivmin;
      count += q < 0.0 ? 1 : 0;
    }
    if (count > j) hi = mid;
    else lo = mid;
  }
  double lam = 0.5 * lo + 0.5 * hi;
  if (fmax(fabs(lo), fabs(hi)) <= 8.0 * pivmin) lam = 0.0;
  out[n - 1 - j] = lam;
}

}  // namespace topolow
