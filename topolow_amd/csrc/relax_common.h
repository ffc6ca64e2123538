// topolow_amd/csrc/relax_common.h -- shared host/device definitions of libtopolow_relax.so.
#pragma once

#include <stdint.h>
#include <math.h>
#include <float.h>
#include <stdlib.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TL_HD __host__ __device__
#else
#define TL_HD
#endif

namespace topolow {

// ---------------------------------------------------------------------------------------
// fp32 target encoding.  One 4-byte word per ORDERED pair (row i, column c):
//   value  = fp32(target) rounded to a multiple of 4 ulp (relative error < 3e-7)
//   bits[1:0] = threshold code: 0 exact, 1 ">", 2 "<"
//   unmeasured pair = (+Inf, "<"): "spring if r > +Inf" never holds, so the pair always takes
//   the repulsion branch (reference src/optimization.cpp:221,269-281) without a separate test.
//   The diagonal and the padding columns [n, ld) also carry the unmeasured word: a point
//   paired with itself has delta = 0 (contributes exactly 0), and padding columns are given
//   a phantom position so far away that the repulsion coefficient underflows to exactly 0.
// ---------------------------------------------------------------------------------------
constexpr uint32_t kCodeMask = 3u;
constexpr uint32_t kInfWord = 0x7f800002u;   // +Inf | "<"  == unmeasured
constexpr float kFarF32 = 1.0e18f;           // phantom coordinate of padding columns (f32)
constexpr double kFarF64 = 1.0e150;          // ... (f64)

TL_HD inline uint32_t f32_bits(float f) {
  union { float f; uint32_t u; } v; v.f = f; return v.u;
}
TL_HD inline float bits_f32(uint32_t u) {
  union { float f; uint32_t u; } v; v.u = u; return v.f;
}

// threshold_code as the reference passes it: 0 exact, 1 ">", anything else "<" (the
// reference's else-branch, src/optimization.cpp:236-242).
TL_HD inline uint32_t encode_target(double t, int code) {
  if (!__builtin_isfinite(t)) return kInfWord;  // NaN, +-Inf: not finite -> unmeasured (:221)
  float f = (float)t;
  uint32_t u = f32_bits(f);
  uint32_t mag = u & 0x7fffffffu;
  if (mag >= 0x7f7ffffcu) mag = 0x7f7ffffcu;  // keep huge finite targets finite
  else mag = (mag + 2u) & ~kCodeMask;
  if (mag >= 0x7f800000u) mag = 0x7f7ffffcu;
  const uint32_t c = code == 0 ? 0u : (code == 1 ? 1u : 2u);
  return (u & 0x80000000u) | mag | c;
}

TL_HD inline double decode_target(uint32_t w, int* code) {
  const uint32_t c = w & kCodeMask;
  if (code) *code = c == 0 ? 0 : (c == 1 ? 1 : -1);
  return (double)bits_f32(w & ~kCodeMask);
}

// What the word's rounding took from a measured target, as fp32: target = decode(word) + delta to 2e-14 relative (the
// word is within 3e-7 of the target, the fp32 delta within 6e-8 of that).  0 for an unmeasured cell, and for a target so
// large that its word was clamped.  Sessions of precision f64_exact keep one per cell beside the words (the "delta block").
TL_HD inline float encode_delta(double t, uint32_t w) {
  if (w == kInfWord) return 0.0f;
  const float d = (float)(t - (double)bits_f32(w & ~kCodeMask));
  return __builtin_isfinite(d) ? d : 0.0f;
}

// ---------------------------------------------------------------------------------------
// Layout of an encoded block in HBM.  Production: row-major, rows x ld words, ld % 64 == 0.
// Every kernel addresses the block through enc_index / enc_col_offset_bytes, so a layout is one
// definition.  Tried on MI355X and NOT kept (-DTOPOLOW_ENC_TILED=1 builds it): "row-group tiles" -- the
// 8 x 256 words of a (workgroup's rows, 256-column group) tile contiguous, a workgroup's tiles one
// after another, so that a workgroup streams ONE contiguous region instead of eight rows ld * 4 bytes
// apart.  Bit-identical results; config 3 (one 400-MB sweep per iteration) 66.6 instead of 64.6 us per
// launch, config 4 on one GPU 513 instead of 500 iterations/s: within the box-to-box spread either way.
// ---------------------------------------------------------------------------------------
#ifndef TOPOLOW_ENC_TILED
#define TOPOLOW_ENC_TILED 0
#endif
#if TOPOLOW_ENC_TILED
constexpr int kEncLdAlign = 256;
constexpr int kEncRowAlign = 8;
TL_HD inline size_t enc_index(int row_in_block, int c, int ld) {
  return (size_t)(row_in_block >> 3) * ((size_t)8 * (size_t)ld) + (size_t)(c >> 8) * 2048 +
         (size_t)(row_in_block & 7) * 256 + (size_t)(c & 255);
}
// byte offset of column c from the first word of its row (enc_index(row, 0, ld))
TL_HD inline int enc_col_offset_bytes(int c) { return ((c >> 8) << 13) | ((c & 255) << 2); }
TL_HD inline int enc_row_span_bytes(int row_in_block, int ld) { return (8 * ld - (row_in_block & 7) * 256) * 4; }
#else
constexpr int kEncLdAlign = 64;
constexpr int kEncRowAlign = 1;
TL_HD inline size_t enc_index(int row_in_block, int c, int ld) { return (size_t)row_in_block * (size_t)ld + (size_t)c; }
TL_HD inline int enc_col_offset_bytes(int c) { return c * 4; }
TL_HD inline int enc_row_span_bytes(int, int ld) { return ld * 4; }
#endif

// ---------------------------------------------------------------------------------------
// Counter-based random numbers for schedules (same stream on host and device).
// ---------------------------------------------------------------------------------------
TL_HD inline uint64_t mix64(uint64_t z) {  // splitmix64 finaliser
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
TL_HD inline uint64_t rnd64(uint64_t seed, uint64_t stream, uint64_t ctr) {
  return mix64(mix64(seed ^ (stream * 0xd1342543de82ef95ull)) + ctr * 0x9e3779b97f4a7c15ull);
}
// Unbiased-enough bounded integer (multiply-shift on the high 32 bits).
TL_HD inline uint32_t rnd_below(uint64_t r, uint32_t bound) {
  return (uint32_t)(((r >> 32) * (uint64_t)bound) >> 32);
}

// ---------------------------------------------------------------------------------------
// Slab plan.  Columns live in the padded index space [0, n4), n4 = roundup(n, 4) (padding
// columns carry the skip code).  An iteration is cut into S' = ceil(n4 / w) slabs of width
// w = roundup(ceil(n4 / S), 4) placed cyclically from a random offset (multiple of 4), and
// executed in a random order.  A slab that wraps is two ranges.
// ---------------------------------------------------------------------------------------
constexpr int kMaxStages = 64;

struct SlabGeom {
  int n4;
  int w;
  int n_stages;
};

TL_HD inline SlabGeom slab_geom(int n, int stages) {
  SlabGeom g;
  g.n4 = (n + 3) & ~3;
  if (stages < 1) stages = 1;
  if (stages > kMaxStages) stages = kMaxStages;
  int w = (g.n4 + stages - 1) / stages;
  w = (w + 3) & ~3;
  if (w < 4) w = 4;
  g.w = w;
  g.n_stages = (g.n4 + w - 1) / w;
  return g;
}

struct SlabRanges {
  int b0, e0, b1, e1;  // [b0,e0) and [b1,e1) (second empty unless wrapped)
};

// Range(s) of the slab executed at position `slot` of iteration `iter`.
TL_HD inline SlabRanges slab_ranges(const SlabGeom& g, uint64_t seed, int iter, int slot) {
  // random order: Fisher-Yates over stage ids, recomputed by every caller (<= 64 steps)
  int perm[kMaxStages];
  for (int q = 0; q < g.n_stages; ++q) perm[q] = q;
  for (int q = g.n_stages - 1; q > 0; --q) {
    const uint32_t r = rnd_below(rnd64(seed, 0x51ab5ull, ((uint64_t)iter << 8) | (uint64_t)q),
                                 (uint32_t)(q + 1));
    const int tmp = perm[q]; perm[q] = perm[r]; perm[r] = tmp;
  }
  const int j = perm[slot];
  const uint32_t groups = (uint32_t)(g.n4 / 4);
  const int off = 4 * (int)rnd_below(rnd64(seed, 0x0ff5e7ull, (uint64_t)iter), groups);
  const int len = (j == g.n_stages - 1) ? (g.n4 - j * g.w) : g.w;
  int start = off + j * g.w;
  if (start >= g.n4) start -= g.n4;
  SlabRanges r;
  r.b0 = start;
  if (start + len <= g.n4) { r.e0 = start + len; r.b1 = 0; r.e1 = 0; }
  else { r.e0 = g.n4; r.b1 = 0; r.e1 = start + len - g.n4; }
  return r;
}

// Adaptive stage count.  Within a stage the updates are Jacobi: every point sums its own halves over the
// slab from frozen positions.  Linearised around a fit, a stage multiplies the position error by
// I - a L, L the (direction-weighted) Laplacian of the measured pairs; with per-pair gain
// a = 2k / (4 g + k) and about g partners per point its largest eigenvalue is about (k / S) / d in d
// dimensions (2 G / d with G = k / (2 S), both endpoints move), so a stage is stable for k / S < 2 d.  In the
// schedule study (tests/study) the slab schedule was stable for k / S <~ 5 at d = 3 and 5.  The policy keeps
// k / S <= min(3, d): a factor 2 inside the first bound, 0.6 of the measured one (round 2 shipped 2.5; with 3.0 and
// 3.5 every statistic of the ten pinned problems -- two of them at 7 168 points -- stays where it is to 1e-4,
// 64 seeds each: profiles/r03_schedule_study.txt).  No other floor: once k <= 3 (d >= 3) an iteration is
// ONE sweep -- what decides the result happens in the first iterations, see below.
#if defined(TOPOLOW_TUNING) && !defined(__HIP_DEVICE_COMPILE__)
// study builds (make tuning): the schedule's constants from the environment (tests/study/schedule_study.py)
inline double tl_env_num(const char* name, double dflt) { const char* e = getenv(name); return e ? atof(e) : dflt; }
#define TL_STAGE_K tl_env_num("TL_STAGE_K", 3.0)
#define TL_EARLY_ITERS ((int)tl_env_num("TL_EARLY_ITERS", 8))
#define TL_EARLY_STAGES ((int)tl_env_num("TL_EARLY_STAGES", 16))
#else
#define TL_STAGE_K 3.0
#define TL_EARLY_ITERS kEarlyIters
#define TL_EARLY_STAGES kEarlyStages
#endif
constexpr int kEarlyIters = 8;
constexpr int kEarlyStages = 16;
TL_HD inline int slab_stages_for_k(double k, int ndim) {
  const double per_stage = ndim < 3 ? (double)(ndim < 1 ? 1 : ndim) : TL_STAGE_K;
  int s = 1;
  while ((double)s * per_stage < k && s < kMaxStages) s <<= 1;
  return s;
}

// While the layout unfolds from the reference's random-walk start (R/core.R:407-415) the moves are
// large and which basin the embedding settles in is decided: the first kEarlyIters iterations run
// at least kEarlyStages stages.  Measured on MI355X (tests/study/gpu_contract_study.py, 32 seeds per
// problem): with this floor and random labels the final-MAE distribution of the slab schedule sits
// inside the reference-order oracle's  mean +- max(3 sd, 1 %)  on every pinned problem; what runs
// afterwards no longer moves the result: 16, 12 and 8 unfolding iterations give the same statistics to 1e-4 on
// every pinned problem (profiles/r02_schedule_study.txt, r03_schedule_study.txt: 64 seeds each) -- 8 it is; 8 unfolding
// STAGES instead of 16 let 2-D runs diverge.
TL_HD inline int slab_stages_at(int iter, double k, int ndim) {
  const int s = slab_stages_for_k(k, ndim);
  return (iter < TL_EARLY_ITERS && s < TL_EARLY_STAGES) ? TL_EARLY_STAGES : s;
}

// ---------------------------------------------------------------------------------------
// Convergence controller (reference src/optimization.cpp:168-179 state, :303-357 logic).
// ---------------------------------------------------------------------------------------
struct Controller {
  double best_mae;
  double best_k;
  double eps;
  int best_iter;
  int worsening;
  int plateau;
  int window;

  TL_HD void init(double k0, int window_, double eps_) {
    best_mae = DBL_MAX; best_k = k0; eps = eps_; best_iter = 0; worsening = 0; plateau = 0;
    window = window_;
  }
  // Returns bit0 = stop, bit1 = snapshot positions now.
  TL_HD int observe(double err, int iter1, double k) {
    int snap = 0;
    if (err < best_mae * (1.0 - eps)) {
      best_mae = err; best_k = k; best_iter = iter1; worsening = 0; plateau = 0;
      return 2;
    }
    if (err <= best_mae * (1.0 + eps)) {
      if (err < best_mae) { best_mae = err; best_k = k; best_iter = iter1; snap = 2; }
      worsening = 0;
      ++plateau;
      return snap | (plateau >= window ? 1 : 0);
    }
    plateau = 0;  // also the NaN path: every comparison above is false
    ++worsening;
    return worsening >= window ? 1 : 0;
  }
};

// Device-resident run state of one embedding (slab path).
struct RunState {
  Controller ctl;
  double k_base;        // spring constant at iteration iter_base
  double cooling;
  double last_mae;
  int iter_base;        // iterations completed
  int n_iter;
  int stopped;          // 1 after the controller said stop (kernels become no-ops)
  int converged;
  int n_checks;
  int first_nonfinite;  // first iteration (1-based) that produced a non-finite position
  int pad0, pad1;
  // The best snapshot lives in one of the session's two snapshot buffers (0, 1).  best_buf[best_entry] names it.  Two
  // entries, so that a check that rides in an apply's launch never reads what its own launch writes: the launch of
  // check number c reads entry c & 1 (every column block copies its points into the OTHER buffer) and its controller
  // writes entry (c + 1) & 1 and best_entry; controller_kernel copies by itself and leaves both entries equal.
  int best_buf[2];
  int best_entry;
  // 0 while the run goes on; after a stop, check number + 1 of the in-apply check that stopped it, or -1 (a stop by
  // controller_kernel).  One word, so the apply kernel learns from one load whether the stop is its own launch's.
  int stop_mark;
};

#if defined(__HIPCC__)
// ||pj - pi||: pdist_kernel's own arithmetic -- a sequential s += dev * dev over the coordinates, then ::sqrt -- so the
// result is bit-identical to topolow_est_distances.  The one copy every kernel that scores a cell calls (relax_post.h,
// relax_fit.h).
__device__ inline double post_distance(const double* __restrict__ pj, const double* __restrict__ pi, int dim) {
  double s = 0.0;
  for (int d = 0; d < dim; ++d) {
    const double dev = pj[d] - pi[d];
    s += dev * dev;
  }
  return ::sqrt(s);
}
#endif

}  // namespace topolow
