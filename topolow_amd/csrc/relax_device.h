// topolow_amd/csrc/relax_device.h -- the device functions and constants the relaxation kernel families share: the
// block size of the auxiliary kernels, Math<>, the wave reductions, the controller step of one workgroup and the
// fingerprint of a measured cell.  Included by relax_kernels.h (the stage, check and loader kernels), relax_symm.h
// (the symmetric sweeps) and relax_cv.h (the hold-out kernels).  No kernels here: any source may include it.
#pragma once

#include <hip/hip_runtime.h>
#include <type_traits>
#include "relax_common.h"

namespace topolow {

constexpr int kThreads = 256;       // block size of the auxiliary kernels
constexpr int kWaves = kThreads / 64;

template <typename real> struct Math;
template <> struct Math<float> {
  static __device__ __forceinline__ float sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
  static __device__ __forceinline__ float rcp(float x) { return __builtin_amdgcn_rcpf(x); }
  static constexpr float far() { return kFarF32; }
};
template <> struct Math<double> {
  // The hardware estimates (v_rsq_f64, v_rcp_f64: ~2^-26) and two Newton steps: within 1 ulp of the correctly rounded
  // result, 15 instructions for the pair where the IEEE expansions (scaling for denormals, division fix-ups) take 25.
  // The arguments here are sums of squares of coordinate differences -- exactly 0 for a point with itself, never
  // denormal otherwise -- and r + 0.01 in [0.01, 1e150].  (-DTOPOLOW_F64_IEEE: the library calls.)  The exact GS
  // kernels (relax_gs.h, relax_tilegs.h), which are held to the CPU oracle pair by pair, do not come through here.
#ifdef TOPOLOW_F64_IEEE
  static __device__ __forceinline__ double sqrt(double x) { return ::sqrt(x); }
  static __device__ __forceinline__ double rcp(double x) { return 1.0 / x; }
#else
  static __device__ __forceinline__ double sqrt(double x) {
    const double y0 = __builtin_amdgcn_rsq(x);
    double g = x * y0, h = 0.5 * y0;
    const double e1 = fma(-h, g, 0.5);
    g = fma(g, e1, g);
    h = fma(h, e1, h);
    g = fma(fma(-g, g, x), h, g);
    return x > 0.0 ? g : 0.0;
  }
  static __device__ __forceinline__ double rcp(double x) {
    double y = __builtin_amdgcn_rcp(x);
    y = fma(fma(-x, y, 1.0), y, y);
    return fma(fma(-x, y, 1.0), y, y);
  }
#endif
  static constexpr double far() { return kFarF64; }
};

// Marks a wave-uniform value so the compiler keeps it in scalar registers.
__device__ __forceinline__ float uniform(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
__device__ __forceinline__ double uniform(double v) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_readfirstlane((int)(b & 0xffffffffll));
  const int hi = __builtin_amdgcn_readfirstlane((int)(b >> 32));
  return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}

template <typename real>
__device__ __forceinline__ real wave_sum(real v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// fp32 wave sum on the vector pipe alone (DPP lane permutations; __shfl_xor goes through LDS
// hardware, ds_bpermute, with a round trip per step): quads, half rows, rows, then the row sums are
// passed down the rows; the total is read from lane 63.  Fixed order, so deterministic; the value is
// valid in every lane.
__device__ __forceinline__ float wave_sum_dpp(float v) {
  auto dpp = [](float x, auto ctrl, auto row_mask) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), decltype(ctrl)::value,
                                                                 decltype(row_mask)::value, 0xf, true));
  };
  using std::integral_constant;
  v += dpp(v, integral_constant<int, 0xB1>{}, integral_constant<int, 0xf>{});    // quad_perm [1,0,3,2]
  v += dpp(v, integral_constant<int, 0x4E>{}, integral_constant<int, 0xf>{});    // quad_perm [2,3,0,1]
  v += dpp(v, integral_constant<int, 0x141>{}, integral_constant<int, 0xf>{});   // row_half_mirror
  v += dpp(v, integral_constant<int, 0x140>{}, integral_constant<int, 0xf>{});   // row_mirror
  v += dpp(v, integral_constant<int, 0x142>{}, integral_constant<int, 0xa>{});   // row_bcast:15 -> rows 1, 3
  v += dpp(v, integral_constant<int, 0x143>{}, integral_constant<int, 0xc>{});   // row_bcast:31 -> rows 2, 3
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// Controller step of one workgroup: reduces the partials in a fixed order, runs the reference's
// three-way classification, snapshots positions when the error improved, advances the run
// state and mirrors it to the pinned host mailbox.
//
// The order of the reduction is part of the result: kCtlThreads strided partial sums (virtual
// thread v sums the partials v, v + 1024, ...) followed by a halving tree over them.  A workgroup
// of THREADS < kCtlThreads threads gives thread t the virtual threads t, t + THREADS, ... and
// folds them exactly as the tree's first levels do (v with v + 512, then with v + 256, ...)
// before it runs the remaining levels: the same additions on the same operands.
//
// The snapshot (RunState::best_buf).  check_no < 0, a launch of its own: the step copies the positions by itself into
// the buffer the current entry names, kCtlCopyBatch 16-byte loads of a thread in flight together, and leaves both
// entries equal.  check_no >= 0, check number check_no riding in an apply's launch: the launch's column blocks have
// copied the positions into the buffer entry check_no & 1 does NOT name (relax_symm.h); the step copies nothing and
// writes entry (check_no + 1) & 1 -- that other buffer when the error improved, the same buffer otherwise.
constexpr int kCtlThreads = 1024;
constexpr int kCtlCopyBatch = 4;

template <int THREADS, typename real>
__device__ __forceinline__ void controller_step(
    RunState* st, RunState* mailbox, const double* __restrict__ part_sum,
    const unsigned long long* __restrict__ part_cnt, int n_parts, const real* __restrict__ pos,
    real* __restrict__ best0, real* __restrict__ best1, long long n_values, int iter1, double k_after,
    double* __restrict__ trace, int trace_cap, const double* __restrict__ total2, int check_no) {
  static_assert(THREADS >= 64 && THREADS <= kCtlThreads && kCtlThreads % THREADS == 0 && (THREADS & (THREADS - 1)) == 0,
                "controller_step: a power-of-two workgroup of at most kCtlThreads threads");
  constexpr int V = kCtlThreads / THREADS;   // virtual threads per thread
  // total2 != nullptr: the error sum and count arrive already reduced (two doubles: the row-sharded
  // multi-process driver all-reduces them over RCCL); the partial arrays are ignored
  if (st->stopped) return;
  __shared__ double sh_s[THREADS];
  __shared__ unsigned long long sh_c[THREADS];
  __shared__ int sh_action, sh_cur;
  double s[V];
  unsigned long long c[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    s[j] = 0.0;
    c[j] = 0;
    if (total2 == nullptr)
      for (int p = threadIdx.x + j * THREADS; p < n_parts; p += kCtlThreads) { s[j] += part_sum[p]; c[j] += part_cnt[p]; }
  }
  if (total2 != nullptr && threadIdx.x == 0) { s[0] = total2[0]; c[0] = (unsigned long long)total2[1]; }
#pragma unroll
  for (int h = V / 2; h >= 1; h >>= 1) {   // the tree's levels above THREADS
#pragma unroll
    for (int j = 0; j < h; ++j) { s[j] += s[j + h]; c[j] += c[j + h]; }
  }
  sh_s[threadIdx.x] = s[0];
  sh_c[threadIdx.x] = c[0];
  __syncthreads();
  for (int half = THREADS / 2; half >= 1; half >>= 1) {
    if (threadIdx.x < half) {
      sh_s[threadIdx.x] += sh_s[threadIdx.x + half];
      sh_c[threadIdx.x] += sh_c[threadIdx.x + half];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double err = sh_c[0] > 0 ? sh_s[0] / (double)sh_c[0] : 0.0;  // reference :296
    const int action = st->ctl.observe(err, iter1, k_after);
    st->last_mae = err;
    if (trace != nullptr && st->n_checks < trace_cap) {   // (iteration, MAE, k) of every check
      trace[3 * st->n_checks + 0] = (double)iter1;
      trace[3 * st->n_checks + 1] = err;
      trace[3 * st->n_checks + 2] = k_after;
    }
    st->n_checks += 1;
    st->iter_base = iter1;
    st->k_base = k_after;
    if (check_no >= 0) {
      const int cur = st->best_buf[check_no & 1];
      st->best_buf[(check_no + 1) & 1] = (action & 2) ? cur ^ 1 : cur;
      st->best_entry = (check_no + 1) & 1;
      sh_cur = -1;                                   // (nothing to copy here)
    } else {
      const int cur = st->best_buf[st->best_entry & 1];
      st->best_buf[0] = cur;
      st->best_buf[1] = cur;
      sh_cur = cur;
    }
    if (action & 1) { st->stop_mark = check_no >= 0 ? check_no + 1 : -1; st->stopped = 1; st->converged = 1; }
    sh_action = action;
  }
  __syncthreads();
  if ((sh_action & 2) && sh_cur >= 0) {
    // snapshot: 16-byte copies (both buffers come from hipMalloc, so they are 256-B aligned), a thread's kCtlCopyBatch
    // loads issued before its first store (a chunk past the end repeats the last one: the same bytes to the same place)
    real* __restrict__ best_pos = sh_cur ? best1 : best0;
    const long long bytes = n_values * (long long)sizeof(real);
    const long long n16 = bytes / 16;
    const uint4* src = reinterpret_cast<const uint4*>(pos);
    uint4* dst = reinterpret_cast<uint4*>(best_pos);
    for (long long q = threadIdx.x; q < n16; q += (long long)THREADS * kCtlCopyBatch) {
      uint4 v[kCtlCopyBatch];
#pragma unroll
      for (int j = 0; j < kCtlCopyBatch; ++j) {
        const long long at = q + (long long)j * THREADS;
        v[j] = src[at < n16 ? at : n16 - 1];
      }
#pragma unroll
      for (int j = 0; j < kCtlCopyBatch; ++j) {
        const long long at = q + (long long)j * THREADS;
        dst[at < n16 ? at : n16 - 1] = v[j];   // (unconditional: a store under a branch pulls its load in behind it)
      }
    }
    for (long long q = n16 * 16 / (long long)sizeof(real) + threadIdx.x; q < n_values; q += THREADS)
      best_pos[q] = pos[q];
  }
  __syncthreads();
  if (threadIdx.x == 0 && mailbox != nullptr) {
    *mailbox = *st;
    __threadfence_system();
  }
}

// Order-independent fingerprint of the measured cells the dense MAE pass would reduce, used to
// verify that a caller's edge list is exactly that set (same pairs, same encoded targets).
TL_HD inline uint64_t cell_fingerprint(int lo, int hi, uint32_t word) {
  return mix64(((uint64_t)(uint32_t)lo << 32) ^ (uint64_t)(uint32_t)hi ^ ((uint64_t)word * 0x9e3779b97f4a7c15ull));
}
TL_HD inline bool dense_takes(int i, int c, bool parity) {
  if (!parity) return c > i;
  const bool even = ((i + c) & 1) == 0;
  return (even & (c > i)) | (!even & (c < i));
}

}  // namespace topolow
