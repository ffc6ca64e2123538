// topolow_amd/csrc/topolow_relax.hip -- the session of libtopolow_relax.so: everything that touches a session's
// buffers or launches a relaxation kernel (relax_kernels.h, relax_exact.h, relax_tilegs.h, relax_symm*.h, relax_cv.h)
// -- the launch helpers, the symmetric sweep's host code, the row-sharded engine and the topolow_session_* C ABI of
// include/topolow_relax.h.  The drivers that run whole embeddings on sessions are topolow_drivers.hip, the
// one-workgroup Gauss-Seidel entries topolow_gs.hip, the post-metrics topolow_post.hip, the prepared handle
// topolow_prep.hip with topolow_prep_graph.hip, topolow_spectrum.hip and topolow_prep_fold.hip.
//
// There is no CPU fallback in this library: without a HIP device every entry point that
// computes returns TOPOLOW_ERR_NO_DEVICE.

#include "topolow_session.h"
#include "topolow_prep.h"
#include "relax_kernels.h"
#include "relax_exact.h"
#include "relax_tilegs.h"
#include "relax_symm.h"
#include "relax_symm64.h"
#include "relax_symm_wide.h"
#include "relax_cv.h"

// =========================================================================================
// Session (slab path)
// =========================================================================================
namespace {

// ---- kernel dispatch over (DIM, real) ----------------------------------------------------
#define TL_DISPATCH_DIM(dim, FN, ...)                 \
  switch (dim) {                                      \
    case 1: FN<1>(__VA_ARGS__); break;                \
    case 2: FN<2>(__VA_ARGS__); break;                \
    case 3: FN<3>(__VA_ARGS__); break;                \
    case 4: FN<4>(__VA_ARGS__); break;                \
    case 5: FN<5>(__VA_ARGS__); break;                \
    case 6: FN<6>(__VA_ARGS__); break;                \
    case 7: FN<7>(__VA_ARGS__); break;                \
    case 8: FN<8>(__VA_ARGS__); break;                \
    case 9: FN<9>(__VA_ARGS__); break;                \
    case 10: FN<10>(__VA_ARGS__); break;              \
    case 12: FN<12>(__VA_ARGS__); break;              \
    case 16: FN<16>(__VA_ARGS__); break;              \
    case 32: FN<32>(__VA_ARGS__); break;              \
    case 64: FN<64>(__VA_ARGS__); break;              \
    default: throw HipError{TOPOLOW_ERR_UNSUPPORTED, "ndim must be between 1 and 64"}; \
  }

struct ProfScope {
  topolow_session* s;
  std::vector<std::pair<hipEvent_t, hipEvent_t>>* dst;
  hipEvent_t a = nullptr, b = nullptr;
  ProfScope(topolow_session* s_, std::vector<std::pair<hipEvent_t, hipEvent_t>>* d) : s(s_), dst(d) {
    if (!s->profiling) return;
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    HIP_TRY(hipEventRecord(a, s->stream));
  }
  ~ProfScope() {
    if (!a) return;
    (void)hipEventRecord(b, s->stream);
    dst->emplace_back(a, b);
  }
};

// Stage-kernel geometry.  Production: 256 threads, 2 rows per wave (8 rows per workgroup), chunk
// size picked per ndim (PipeGeom), falling issue priority, register budget for 5 waves per SIMD --
// the fastest of the variants measured on MI355X.  A build with
// -DTOPOLOW_TUNING also instantiates other chunk sizes / budgets (TOPOLOW_SLAB_VARIANT=<n>) and
// the per-workgroup time stamps (TOPOLOW_WG_STAMPS=<file>).
using CfgProd = StageCfg<256, 2, 0, 1, 5>;
#ifdef TOPOLOW_TUNING
// TOPOLOW_WG_STAMPS=<file>: the stage kernel's workgroups stamp their start/end times; the last
// launch's stamps are written to <file> as text when the session is destroyed.
struct WgStamps {
  unsigned long long* dev = nullptr;
  int blocks = 0;
  void arm(int nblocks) {
    if (dev != nullptr || getenv("TOPOLOW_WG_STAMPS") == nullptr) return;
    blocks = nblocks;
    if (hipMalloc(&dev, sizeof(unsigned long long) * 2 * nblocks) != hipSuccess) { dev = nullptr; return; }
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_wg_stamps), &dev, sizeof(dev));
  }
  void dump() {
    if (dev == nullptr) return;
    std::vector<unsigned long long> h(2 * (size_t)blocks);
    (void)hipDeviceSynchronize();
    (void)hipMemcpy(h.data(), dev, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    if (FILE* f = fopen(getenv("TOPOLOW_WG_STAMPS"), "w")) {
      for (int b = 0; b < blocks; ++b) fprintf(f, "%llu %llu\n", h[2 * b], h[2 * b + 1]);
      fclose(f);
    }
    unsigned long long* none = nullptr;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_wg_stamps), &none, sizeof(none));
    (void)hipFree(dev);
    dev = nullptr;
  }
};
WgStamps g_stamps;

int slab_variant() {
  static int v = [] {
    const char* e = getenv("TOPOLOW_SLAB_VARIANT");
    return e ? atoi(e) : -1;
  }();
  return v;
}
#endif

template <int DIM, typename real, typename CFG>
void launch_stage_pipe(topolow_session* s, const void* pin, void* pout, RunState* st,
                       SlabRanges rg, int iter1, double k, const void* push, int n_push, bool err) {
  const int blocks = (s->rows() + CFG::ROWS - 1) / CFG::ROWS;
#ifdef TOPOLOW_TUNING
  g_stamps.arm(blocks);
#endif
  auto launch = [&](auto kern, int which) {
    // falling issue priority only when every workgroup of the grid is resident at once
    static int resident[2] = {0, 0};     // workgroups of this (ndim, precision) kernel a device holds
    if (resident[which] == 0) {          // [0] threshold-free instance, [1] threshold-carrying one
      hipDeviceProp_t prop;
      HIP_TRY(hipGetDeviceProperties(&prop, s->device));
      int per_cu = 0;
      HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, CFG::THREADS, 0));
      resident[which] = std::max(1, per_cu) * prop.multiProcessorCount;
    }
    const int falling = blocks <= resident[which] ? 1 : 0;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(CFG::THREADS), 0, s->stream, s->enc.p, s->ld,
                       s->row_begin, s->row_end, s->n, (const real*)pin, (real*)pout, s->gplus.p,
                       s->rowflags.p, st, rg, iter1, k, s->c_rep, falling, (real* const*)push, n_push,
                       s->part_sum.p, s->part_cnt.p, s->block_cells);
  };
  if constexpr (sizeof(real) == 4) {
    if (err) {   // the launch also reduces the convergence MAE of the positions it reads (one-stage iterations)
      if (s->any_threshold) {
        constexpr int kThrWavesE = DIM >= 16 ? 1 : (DIM >= 12 ? 2 : (DIM >= 9 ? 3 : (DIM >= 5 ? 4 : 5)));   // the error sums cost registers: 4 waves from ndim 5
        using CfgThrE = StageCfg<CFG::THREADS, CFG::RPW, CFG::CHUNK, CFG::PRIO,
                                 CFG::MINWAVES < kThrWavesE ? CFG::MINWAVES : kThrWavesE>;
        launch(&slab_stage_pipe_kernel<DIM, real, CfgThrE, true, true>, 1);
      } else {
        launch(&slab_stage_pipe_kernel<DIM, real, CFG, false, true>, 0);
      }
      return;
    }
  }
  if (s->any_threshold) {
    // The instance that also carries the ">" / "<" classification needs more registers: from
    // ndim 7 on it would spill inside the pair loop at a 5-wave budget (9x slower at ndim 10), so
    // it is built for 4 waves per SIMD there and for 3 from ndim 9 (tests/test_capi.py checks that no
    // instantiation uses scratch).
    constexpr int kThrWaves = sizeof(real) == 4 ? (DIM >= 16 ? 1 : (DIM >= 12 ? 2 : (DIM >= 9 ? 3 : (DIM >= 7 ? 4 : 5)))) : 1;
    using CfgThr = StageCfg<CFG::THREADS, CFG::RPW, CFG::CHUNK, CFG::PRIO,
                            CFG::MINWAVES < kThrWaves ? CFG::MINWAVES : kThrWaves>;
    launch(&slab_stage_pipe_kernel<DIM, real, CfgThr, true>, 1);
  } else {
    launch(&slab_stage_pipe_kernel<DIM, real, CFG, false>, 0);
  }
}

// The row-owner stage of an f64_exact session (relax_exact.h): the f64 pipe kernel's geometry, targets = word + delta.
template <int DIM>
void launch_stage_exact(topolow_session* s, const void* pin, void* pout, RunState* st, SlabRanges rg, int iter1, double k,
                        int n_push) {
  using CFG = StageCfg<256, 2, 0, 1>;
  if (n_push > 0) throw HipError{TOPOLOW_ERR_UNSUPPORTED, "precision f64_exact: no row blocks (the stage kernel pushes to no peer)"};
  const int blocks = (s->rows() + CFG::ROWS - 1) / CFG::ROWS;
  auto launch = [&](auto kern, int which) {
    static int resident[2] = {0, 0};     // as launch_stage_pipe: falling priority only when the whole grid is resident
    if (resident[which] == 0) {
      hipDeviceProp_t prop;
      HIP_TRY(hipGetDeviceProperties(&prop, s->device));
      int per_cu = 0;
      HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, CFG::THREADS, 0));
      resident[which] = std::max(1, per_cu) * prop.multiProcessorCount;
    }
    const int falling = blocks <= resident[which] ? 1 : 0;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(CFG::THREADS), 0, s->stream, s->enc.p, s->denc.p, s->ld, s->row_begin,
                       s->row_end, s->n, (const double*)pin, (double*)pout, s->gplus.p, s->rowflags.p, st, rg, iter1, k,
                       s->c_rep, falling);
  };
  if (s->any_threshold) launch(&slab_stage_exact_kernel<DIM, CFG, true>, 1);
  else launch(&slab_stage_exact_kernel<DIM, CFG, false>, 0);
}

template <int DIM>
void launch_stage(topolow_session* s, const void* pin, void* pout, RunState* st, SlabRanges rg,
                  int iter1, double k, const void* push = nullptr, int n_push = 0, bool err = false) {
  if (s->rows() <= 0) return;
  ProfScope prof(s, err ? &s->prof_stage_err : &s->prof_stage);
  if constexpr (DIM > kMaxTunedDim) {      // wide embeddings: the plain stage kernel (never an ERR launch: no dense MAE there)
    const int blocks = (s->rows() + kWaves - 1) / kWaves;
    if (s->exact) throw HipError{TOPOLOW_ERR_UNSUPPORTED, "precision f64_exact: ndim must be between 1 and 16"};   // (refused at creation)
    if (s->precision == TOPOLOW_PRECISION_F64)
      hipLaunchKernelGGL((slab_stage_wide_kernel<DIM, double>), dim3(blocks), dim3(kThreads), 0, s->stream, s->enc.p, s->ld,
                         s->row_begin, s->row_end, s->n, (const double*)pin, (double*)pout, s->gplus.p, st, rg, iter1, k,
                         s->c_rep, (double* const*)push, n_push);
    else
      hipLaunchKernelGGL((slab_stage_wide_kernel<DIM, float>), dim3(blocks), dim3(kThreads), 0, s->stream, s->enc.p, s->ld,
                         s->row_begin, s->row_end, s->n, (const float*)pin, (float*)pout, s->gplus.p, st, rg, iter1, k,
                         s->c_rep, (float* const*)push, n_push);
    HIP_TRY(hipGetLastError());
    s->stage_launches += 1;
    return;
  } else
  if (s->exact) {
    launch_stage_exact<DIM>(s, pin, pout, st, rg, iter1, k, n_push);
  } else if (s->precision == TOPOLOW_PRECISION_F64) {
    launch_stage_pipe<DIM, double, StageCfg<256, 2, 0, 1>>(s, pin, pout, st, rg, iter1, k, push, n_push, false);
  } else {
#ifdef TOPOLOW_TUNING
    switch (slab_variant()) {
      case 20: launch_stage_pipe<DIM, float, StageCfg<256, 2, 512, 0, 5>>(s, pin, pout, st, rg, iter1, k, push, n_push, err); break;
      case 21: launch_stage_pipe<DIM, float, StageCfg<256, 2, 768, 1, 5>>(s, pin, pout, st, rg, iter1, k, push, n_push, err); break;
      case 22: launch_stage_pipe<DIM, float, StageCfg<256, 2, 512, 1, 4>>(s, pin, pout, st, rg, iter1, k, push, n_push, err); break;
      case 23: launch_stage_pipe<DIM, float, StageCfg<256, 2, 256, 1, 5>>(s, pin, pout, st, rg, iter1, k, push, n_push, err); break;
      case 24: launch_stage_pipe<DIM, float, StageCfg<256, 2, 512, 1, 7>>(s, pin, pout, st, rg, iter1, k, push, n_push, err); break;
      case 25: launch_stage_pipe<DIM, float, StageCfg<512, 2, 768, 0, 4>>(s, pin, pout, st, rg, iter1, k, push, n_push, err); break;
      case 27: launch_stage_pipe<DIM, float, StageCfg<256, 2, 1024, 1, 4>>(s, pin, pout, st, rg, iter1, k, push, n_push, err); break;
      case 28: launch_stage_pipe<DIM, float, StageCfg<512, 2, 512, 0, 4>>(s, pin, pout, st, rg, iter1, k, push, n_push, err); break;
      default: launch_stage_pipe<DIM, float, CfgProd>(s, pin, pout, st, rg, iter1, k, push, n_push, err); break;
    }
#else
    // register budget: 5 waves per SIMD up to ndim 10 (CfgProd), 3 at 12 coordinates, 2 at 16
    using CfgDim = StageCfg<CfgProd::THREADS, CfgProd::RPW, CfgProd::CHUNK, CfgProd::PRIO,
                            DIM <= 10 ? CfgProd::MINWAVES : (DIM <= 12 ? 3 : 2)>;
    launch_stage_pipe<DIM, float, CfgDim>(s, pin, pout, st, rg, iter1, k, push, n_push, err);
#endif
  }
  HIP_TRY(hipGetLastError());
  s->stage_launches += 1;
}

using ErrCfg = StageCfg<256, 2, 1024>;

template <int DIM, typename real>
void launch_dense_error(topolow_session* s, const void* pos, const RunState* st) {
  const size_t lds = sizeof(real) * DIM * ErrCfg::CHUNK;
  const dim3 grid(s->dense_grid_x, s->dense_grid_y);
  if (s->dense_parity) {
    hipLaunchKernelGGL((dense_error_kernel<DIM, real, ErrCfg, true>), grid, dim3(ErrCfg::THREADS), lds,
                       s->stream, s->enc.p, s->ld, s->row_begin, s->row_end, s->n, (const real*)pos,
                       s->rowflags.p, s->part_sum.p, s->part_cnt.p, st);
  } else {
    hipLaunchKernelGGL((dense_error_kernel<DIM, real, ErrCfg, false>), grid, dim3(ErrCfg::THREADS), lds,
                       s->stream, s->enc.p, s->ld, s->row_begin, s->row_end, s->n, (const real*)pos,
                       s->rowflags.p, s->part_sum.p, s->part_cnt.p, st);
  }
}

// Workgroups (= partial sums) of the edge-list MAE pass over n_edges edges.
int edge_error_blocks(long long n_edges) {
  long long blocks = (n_edges + (long long)kThreads * 8 - 1) / ((long long)kThreads * 8);
  if (blocks < 1) blocks = 1;
  if (blocks > 2048) blocks = 2048;
  return (int)blocks;
}

// Number of partial sums the last launched error kernel produced.
int error_parts(const topolow_session* s) { return s->dense_mae ? s->dense_blocks : s->n_parts; }

template <int DIM>
void launch_edge_error(topolow_session* s, const void* pos, const RunState* st) {
  if (s->dense_mae) {
    if constexpr (DIM > kMaxTunedDim) {
      throw HipError{TOPOLOW_ERR_UNSUPPORTED, "dense MAE pass: ndim"};   // (wide sessions never set dense_mae)
    } else {
      if (s->precision == TOPOLOW_PRECISION_F64) launch_dense_error<DIM, double>(s, pos, st);
      else launch_dense_error<DIM, float>(s, pos, st);
    }
  } else if (s->precision == TOPOLOW_PRECISION_F64) {
    hipLaunchKernelGGL((edge_error_kernel<DIM, double, double>), dim3(s->n_parts),
                       dim3(kThreads), 0, s->stream, (const double*)pos, s->ei.p, s->ej.p,
                       (const double*)s->et.p, s->ec.p, s->n_edges, s->part_sum.p,
                       s->part_cnt.p, st);
  } else {
    hipLaunchKernelGGL((edge_error_kernel<DIM, float, float>), dim3(s->n_parts), dim3(kThreads),
                       0, s->stream, (const float*)pos, s->ei.p, s->ej.p, (const float*)s->et.p,
                       s->ec.p, s->n_edges, s->part_sum.p, s->part_cnt.p, st);
  }
  HIP_TRY(hipGetLastError());
}

// psum / pcnt / nparts: the partials to reduce (default: the block's own error-kernel partials)
void launch_controller(topolow_session* s, const void* pos, int iter1, double k_after,
                       const double* psum = nullptr, const unsigned long long* pcnt = nullptr, int nparts = 0,
                       const double* total2 = nullptr) {
  const long long nv = (long long)s->n * s->dim;
  if (psum == nullptr && total2 == nullptr) { psum = s->part_sum.p; pcnt = s->part_cnt.p; nparts = error_parts(s); }
  if (s->precision == TOPOLOW_PRECISION_F64) {
    hipLaunchKernelGGL((controller_kernel<double>), dim3(1), dim3(kCtlThreads), 0, s->stream,
                       s->state.p, s->mailbox_dev, psum, pcnt, nparts,
                       (const double*)pos, (double*)s->best[0].p, (double*)s->best[1].p, nv, iter1, k_after, s->trace_dev, s->trace_cap, total2);
  } else {
    hipLaunchKernelGGL((controller_kernel<float>), dim3(1), dim3(kCtlThreads), 0, s->stream,
                       s->state.p, s->mailbox_dev, psum, pcnt, nparts,
                       (const float*)pos, (float*)s->best[0].p, (float*)s->best[1].p, nv, iter1, k_after, s->trace_dev, s->trace_cap, total2);
  }
  HIP_TRY(hipGetLastError());
}

// positions host (n x dim f64 column-major) <-> device (n x dim row-major, session precision)
void upload_positions(topolow_session* s, const double* host_colmajor, void* dst) {
  // rows [n, roundup4(n)) are the phantom points of the padding columns (relax_common.h)
  const size_t nv = (size_t)s->pos_rows() * s->dim;
  if (s->precision == TOPOLOW_PRECISION_F64) {
    std::vector<double> tmp(nv, 0.0);
    for (int i = 0; i < s->n; ++i) {
      const int o = s->perm.empty() ? i : s->perm[i];
      for (int d = 0; d < s->udim; ++d) tmp[(size_t)i * s->dim + d] = host_colmajor[o + (size_t)d * s->n];
    }
    for (int i = s->n; i < s->pos_rows(); ++i) tmp[(size_t)i * s->dim] = kFarF64;
    HIP_TRY(hipMemcpyAsync(dst, tmp.data(), nv * 8, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
  } else {
    std::vector<float> tmp(nv, 0.0f);
    for (int i = 0; i < s->n; ++i) {
      const int o = s->perm.empty() ? i : s->perm[i];
      for (int d = 0; d < s->udim; ++d)
        tmp[(size_t)i * s->dim + d] = (float)host_colmajor[o + (size_t)d * s->n];
    }
    for (int i = s->n; i < s->pos_rows(); ++i) tmp[(size_t)i * s->dim] = kFarF32;
    HIP_TRY(hipMemcpyAsync(dst, tmp.data(), nv * 4, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
}

void download_positions(topolow_session* s, const void* src, double* host_colmajor) {
  const size_t nv = (size_t)s->n * s->dim;
  if (s->precision == TOPOLOW_PRECISION_F64) {
    std::vector<double> tmp(nv);
    HIP_TRY(hipMemcpyAsync(tmp.data(), src, nv * 8, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    for (int i = 0; i < s->n; ++i) {
      const int o = s->perm.empty() ? i : s->perm[i];
      for (int d = 0; d < s->udim; ++d) host_colmajor[o + (size_t)d * s->n] = tmp[(size_t)i * s->dim + d];
    }
  } else {
    std::vector<float> tmp(nv);
    HIP_TRY(hipMemcpyAsync(tmp.data(), src, nv * 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    for (int i = 0; i < s->n; ++i) {
      const int o = s->perm.empty() ? i : s->perm[i];
      for (int d = 0; d < s->udim; ++d)
        host_colmajor[o + (size_t)d * s->n] = (double)tmp[(size_t)i * s->dim + d];
    }
  }
}

// rowflags, any_threshold and block_cells of the block as it is now, into the buffers the session has.
void scan_row_flags(topolow_session* s) {
  DevBuf<unsigned long long> measured;
  measured.alloc(1);
  HIP_TRY(hipMemsetAsync(measured.p, 0, sizeof(unsigned long long), s->stream));
  hipLaunchKernelGGL(row_flags_kernel, dim3(s->rows()), dim3(kThreads), 0, s->stream, s->enc.p,
                     s->rows(), s->ld, s->rowflags.p, measured.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipMemcpy(&s->block_cells, measured.p, sizeof(unsigned long long), hipMemcpyDeviceToHost));
  std::vector<unsigned char> h(s->rows());
  HIP_TRY(hipMemcpy(h.data(), s->rowflags.p, h.size(), hipMemcpyDeviceToHost));
  s->any_threshold = false;
  for (unsigned char f : h) s->any_threshold = s->any_threshold || f != 0;
}

void compute_row_flags(topolow_session* s) {
  s->cv.active = false;   // a new block: whatever was held out of the old one is gone with it
  s->block_gen += 1;
  s->sym.invalidate();    // a new block invalidates whatever the sweep holds: rebuilt on first use
  s->rowflags.alloc(s->rows());
  scan_row_flags(s);
}

void upload_degrees(topolow_session* s, const int32_t* degrees) {
  std::vector<float> g(s->n);
  for (int i = 0; i < s->n; ++i) g[i] = (float)degrees[s->perm.empty() ? i : s->perm[i]] + 1.0f;  // reference :137-140
  if (s->gplus.p == nullptr || s->gplus.n != (size_t)s->n) s->gplus.alloc(s->n);
  HIP_TRY(hipMemcpy(s->gplus.p, g.data(), (size_t)s->n * 4, hipMemcpyHostToDevice));
}

hipEvent_t take_event(topolow_session* s) {
  if (!s->event_pool.empty()) {
    hipEvent_t e = s->event_pool.back();
    s->event_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return e;
}

void poll_checks(topolow_session* s, size_t keep_in_flight) {
  while (s->pending.size() > keep_in_flight) {
    hipEvent_t e = s->pending.front();
    HIP_TRY(hipEventSynchronize(e));
    s->pending.pop_front();
    s->event_pool.push_back(e);
    if (s->mailbox->stopped) s->host_seen_stop = true;
  }
  // opportunistic: anything already finished
  while (!s->pending.empty() && hipEventQuery(s->pending.front()) == hipSuccess) {
    s->event_pool.push_back(s->pending.front());
    s->pending.pop_front();
    if (s->mailbox->stopped) s->host_seen_stop = true;
  }
}

// Launch helpers take the stream from the session: run a few of them on another one.
struct StreamScope {
  topolow_session* s;
  hipStream_t saved;
  StreamScope(topolow_session* s_, hipStream_t on) : s(s_), saved(s_->stream) { s->stream = on; }
  ~StreamScope() { s->stream = saved; }
};

// ---- exact tile Gauss-Seidel iteration (relax_tilegs.h): in place on `pos` -------------------
template <int DIM>
void launch_tilegs_iteration(topolow_session* s, void* pos, int iter, double k) {
  if constexpr (DIM > kMaxTunedDim) {
    throw HipError{TOPOLOW_ERR_UNSUPPORTED, "schedule gs: ndim must be between 1 and 16 (wider embeddings run the slab schedule)"};
  } else {
  const int nb = (s->n + kTile - 1) / kTile;
  if ((int)s->bperm.n < nb) s->bperm.alloc(nb);
  hipLaunchKernelGGL(tilegs_perm_kernel, dim3(1), dim3(256), 0, s->stream, s->seed, iter, nb, s->bperm.p,
                     s->state.p);
  const int M = nb + (nb & 1), m1 = M - 1;
  const float* no_delta = nullptr;
  for (int r = 0; r < m1 && nb >= 2; ++r) {
    if (s->exact)
      hipLaunchKernelGGL((tilegs_pair_kernel<DIM, double, true>), dim3(M / 2), dim3(kTile), 0, s->stream, s->enc.p,
                         s->denc.p, s->ld, s->n, (double*)pos, s->gplus.p, s->bperm.p, nb, r, s->state.p, s->seed, iter, k,
                         s->c_rep);
    else if (s->precision == TOPOLOW_PRECISION_F64)
      hipLaunchKernelGGL((tilegs_pair_kernel<DIM, double>), dim3(M / 2), dim3(kTile), 0, s->stream, s->enc.p,
                         no_delta, s->ld, s->n, (double*)pos, s->gplus.p, s->bperm.p, nb, r, s->state.p, s->seed, iter, k,
                         s->c_rep);
    else
      hipLaunchKernelGGL((tilegs_pair_kernel<DIM, float>), dim3(M / 2), dim3(kTile), 0, s->stream, s->enc.p,
                         no_delta, s->ld, s->n, (float*)pos, s->gplus.p, s->bperm.p, nb, r, s->state.p, s->seed, iter, k,
                         s->c_rep);
    s->stage_launches += 1;
  }
  if (s->exact)
    hipLaunchKernelGGL((tilegs_intra_kernel<DIM, double, true>), dim3(nb), dim3(kTile), 0, s->stream, s->enc.p, s->denc.p,
                       s->ld, s->n, (double*)pos, s->gplus.p, s->state.p, s->seed, iter, k, s->c_rep);
  else if (s->precision == TOPOLOW_PRECISION_F64)
    hipLaunchKernelGGL((tilegs_intra_kernel<DIM, double>), dim3(nb), dim3(kTile), 0, s->stream, s->enc.p, no_delta, s->ld,
                       s->n, (double*)pos, s->gplus.p, s->state.p, s->seed, iter, k, s->c_rep);
  else
    hipLaunchKernelGGL((tilegs_intra_kernel<DIM, float>), dim3(nb), dim3(kTile), 0, s->stream, s->enc.p, no_delta, s->ld,
                       s->n, (float*)pos, s->gplus.p, s->state.p, s->seed, iter, k, s->c_rep);
  s->stage_launches += 1;
  HIP_TRY(hipGetLastError());
  }
}

void launch_tilegs_finite(topolow_session* s, const void* pos, int iter1) {
  const long long nv = (long long)s->n * s->dim;
  if (s->precision == TOPOLOW_PRECISION_F64)
    hipLaunchKernelGGL((tilegs_finite_kernel<double>), dim3(64), dim3(256), 0, s->stream, (const double*)pos, nv,
                       s->state.p, iter1);
  else
    hipLaunchKernelGGL((tilegs_finite_kernel<float>), dim3(64), dim3(256), 0, s->stream, (const float*)pos, nv,
                       s->state.p, iter1);
  HIP_TRY(hipGetLastError());
}

// ---- symmetric sweep (relax_symm.h, relax_symm_wide.h, relax_symm64.h) -------------------------------------
// Which sessions take it: the whole matrix on one GPU (no row block, nothing to push), slab schedule, ndim 2..10 in
// fp32 and 2..6 in f64, at least kSymMinPoints points.  Up to ndim 6 the register-tiled kernel keeps eight rows'
// coordinates, constants and sums in VGPRs (20 x ndim + 16 of them); fp32 sessions of ndim 7..10 run
// symm_sweep_wide_kernel, which keeps the rows in LDS and only their sums in VGPRs (relax_symm_wide.h); f64 sessions of
// ndim 7..10 stay on the row-owner kernel.  Row-sharded runs shard it over their sessions (sym_sharded_*, below).
// Everything else stays on the row-owner stage kernel.
constexpr int kSymMinPoints = 7168;   // below ~7000 points a resident wave gets fewer than 8 tiles and the row-owner sweep is faster (tests/study/symm_crossover.py; at ndim 10 the two meet near 4 100 points and the sweep leads by 1.11 at 6 144, 1.27 at 7 168: the gate stays, profiles/r05_symm_wide.txt)

// The sweep's host functions exist for ndim 2..10 only, the dims its kernels are instantiated for (f64: 2..6).
constexpr int kSymMaxDimF32 = kSymWideMaxDim, kSymMaxDimF64 = 6;
// Whether the sweep is on by default at this ndim: where its iteration measured faster than the row-owner kernel's by
// more than the spread of repeated runs.  ndim 2..6: profiles/r03_symm_crossover.txt; ndim 7..10: at N = 10 000 the
// parent's row-owner iteration takes 1.40 .. 1.75 times the sweep's, 27 .. 58 us more at spreads of 5 .. 12 us
// (profiles/r05_symm_wide.txt) -- all on.  A dimension that is off would stay reachable with TOPOLOW_SYMMETRIC=1.
constexpr bool sym_dim_default(int dim) { return dim >= 2 && dim <= kSymMaxDimF32; }
#define TL_DISPATCH_SYM(dim, FN, ...)                                                 \
  switch (dim) {                                                                      \
    case 2: FN<2>(__VA_ARGS__); break;                                                \
    case 3: FN<3>(__VA_ARGS__); break;                                                \
    case 4: FN<4>(__VA_ARGS__); break;                                                \
    case 5: FN<5>(__VA_ARGS__); break;                                                \
    case 6: FN<6>(__VA_ARGS__); break;                                                \
    case 7: FN<7>(__VA_ARGS__); break;                                                \
    case 8: FN<8>(__VA_ARGS__); break;                                                \
    case 9: FN<9>(__VA_ARGS__); break;                                                \
    case 10: FN<10>(__VA_ARGS__); break;                                              \
    default: throw HipError{TOPOLOW_ERR_UNSUPPORTED, "symmetric sweep: ndim"};        \
  }

using SymPlanDev = topolow_session::SymState::Plan;
using SymHolds = topolow_session::SymState::Holds;

// The shape every form of the sweep needs; the eligibility of each form adds its own terms.
// The precision term is part of the shape: the largest ndim differs (fp32: 10, f64: 6).
bool sym_shape_ok(const topolow_session* s) {
  const int max_dim = s->precision == TOPOLOW_PRECISION_F32 ? kSymMaxDimF32
                      : s->precision == TOPOLOW_PRECISION_F64 ? kSymMaxDimF64 : 0;
  return s->sym.allowed && s->schedule == TOPOLOW_SCHEDULE_SLAB && s->dim >= 2 && s->dim <= max_dim &&
         (sym_dim_default(s->dim) || s->sym.forced) && s->dim == s->udim && s->n >= s->sym.min_n;
}

bool sym_eligible(const topolow_session* s) {
  return sym_shape_ok(s) && s->row_begin == 0 && s->row_end == s->n && s->n_push == 0;
}

// f(real{}) in the session's precision; from ndim 7 there is fp32 only (sym_shape_ok keeps f64 sessions away).
template <int DIM, typename F>
void sym_real(const topolow_session* s, F&& f) {
  if constexpr (DIM <= kSymMaxDimF64) {
    if (s->precision == TOPOLOW_PRECISION_F64) { f(double{}); return; }
  } else if (s->precision != TOPOLOW_PRECISION_F32) {
    throw HipError{TOPOLOW_ERR_UNSUPPORTED, "symmetric sweep: ndim 7..10 in fp32 only"};
  }
  f(float{});
}

// f(kernel) with the sweep instance for (real, thresholds, err): the one list of instances, for the launches and the
// occupancy probe alike.
template <int DIM, typename real, typename F>
void sym_sweep_instance(bool thr, bool err, bool exact, F&& f) {
  if constexpr (std::is_same<real, double>::value) {
    if (exact) {   // f64_exact sessions: targets = word + delta in every instance (relax_symm64.h: symm64x_sweep_kernel)
      if (thr) { if (err) f(&symm64x_sweep_kernel<DIM, true, true>); else f(&symm64x_sweep_kernel<DIM, true, false>); }
      else { if (err) f(&symm64x_sweep_kernel<DIM, false, true>); else f(&symm64x_sweep_kernel<DIM, false, false>); }
    } else
    if (thr) { if (err) f(&symm64_sweep_kernel<DIM, true, true>); else f(&symm64_sweep_kernel<DIM, true, false>); }
    else { if (err) f(&symm64_sweep_kernel<DIM, false, true>); else f(&symm64_sweep_kernel<DIM, false, false>); }
  } else if constexpr (DIM >= kSymWideMinDim) {   // same arguments, rows in LDS (relax_symm_wide.h)
    if (thr) { if (err) f(&symm_sweep_wide_kernel<DIM, true, true>); else f(&symm_sweep_wide_kernel<DIM, true, false>); }
    else { if (err) f(&symm_sweep_wide_kernel<DIM, false, true>); else f(&symm_sweep_wide_kernel<DIM, false, false>); }
  } else {
    if (thr) { if (err) f(&symm_sweep_kernel<DIM, true, true>); else f(&symm_sweep_kernel<DIM, true, false>); }
    else { if (err) f(&symm_sweep_kernel<DIM, false, true>); else f(&symm_sweep_kernel<DIM, false, false>); }
  }
}

// Builds the plan, the tile-major copy and the partial buffers of tiles [t0, t1) of the upper triangle (t1 < 0: all of
// it) from the row blocks `src` (device pointers of their encoded blocks, first rows in row0[0..n_src]).
template <int DIM>
void sym_build(topolow_session* s, const std::vector<const uint32_t*>& src, const std::vector<int>& row0, bool any_thr,
               long long t0, long long t1) {
  auto& y = s->sym;
  y.invalidate();   // until the caller's hold(): a build that throws half-way leaves nothing that reads as built
  y.npad = (s->n + kSymRows - 1) & ~(kSymRows - 1);
  const int TR = y.npad / kSymRows, TC = y.npad / kSymCols;
  if (t1 < 0) t1 = (long long)TR * (TR + 1);
  y.tiles = (int)(t1 - t0);
  const bool whole = t0 == 0 && t1 == (long long)TR * (TR + 1);
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, s->device));
  int occ = 1 << 30;   // the session's two instances (plain, ERR) share one plan: the smaller occupancy decides the grid
  auto probe = [&](auto kern) {
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 64 * kSymWaves, 0));
    occ = std::min(occ, std::max(1, per_cu));
  };
  const bool f64 = s->precision == TOPOLOW_PRECISION_F64;
  sym_real<DIM>(s, [&](auto r) {
    sym_sweep_instance<DIM, decltype(r)>(any_thr, false, s->exact, probe);
    sym_sweep_instance<DIM, decltype(r)>(any_thr, true, s->exact, probe);
  });
  y.grid = occ * prop.multiProcessorCount;
  if (y.grid_cap > 0) y.grid = std::min(y.grid, y.grid_cap);
  y.plan.load(relax_symm_plan(y.npad, y.grid * kSymWaves, t0, t1, &y.seg_first, &y.seg_last));
  for (auto& v : y.rr) v.clear();
  // a stage plan has at most one unit per wave and one more per tile-row and interval end
  const int max_units = std::max(y.plan.n_units, y.grid * kSymWaves + 2 * TR + 8);
  y.src_tab.alloc(src.size());
  y.src_row0.alloc(row0.size());
  HIP_TRY(hipMemcpy(y.src_tab.p, src.data(), src.size() * sizeof(const uint32_t*), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(y.src_row0.p, row0.data(), row0.size() * sizeof(int), hipMemcpyHostToDevice));
  y.tenc.alloc((size_t)std::max(y.tiles, 1) * kSymTileWords);
  if (y.tiles > 0)
    hipLaunchKernelGGL(symm_tiles_kernel, dim3(y.tiles), dim3(256), 0, s->stream, y.src_tab.p, y.src_row0.p, (int)src.size(),
                       s->ld, y.tenc.p, TC, t0, kInfWord);
  HIP_TRY(hipGetLastError());
  const int seg_rows = y.seg_last >= y.seg_first ? y.seg_last - y.seg_first + 1 : 1;
  const size_t rs = s->real_size();
  size_t rec_w = SymRec<DIM>::W;
  if constexpr (DIM <= kSymMaxDimF64) { if (f64) rec_w = SymRec64<DIM>::W; }
  for (auto& r : y.rec) r.alloc((size_t)y.npad * rec_w * rs);
  y.rowpart.alloc((size_t)std::max(max_units, 1) * kSymRows * DIM * rs);
  y.colpart.alloc((size_t)seg_rows * y.npad * DIM * rs);
  // (a segment's first and last tile-row are partial: the columns its tiles never reach must read as zero)
  HIP_TRY(hipMemsetAsync(y.colpart.p, 0, (size_t)seg_rows * y.npad * DIM * rs, s->stream));
  if (s->exact) {
    // the delta tiles come from the session's delta block, permuted like the words (4-byte cells either way); every
    // instance reads them.  (A fused check also needs the edge list to be the block's measured cells: sym_fused_ok.)
    if (!(src.size() == 1 && src[0] == s->enc.p))
      throw HipError{TOPOLOW_ERR_UNSUPPORTED, "precision f64_exact: the sweep is built from the session's own block only"};
    y.tdelta.alloc((size_t)std::max(y.tiles, 1) * kSymTileWords);
    DevBuf<const uint32_t*> dsrc;
    dsrc.alloc(1);
    const uint32_t* dp = reinterpret_cast<const uint32_t*>(s->denc.p);
    HIP_TRY(hipMemcpy(dsrc.p, &dp, sizeof dp, hipMemcpyHostToDevice));
    if (y.tiles > 0)
      hipLaunchKernelGGL(symm_tiles_kernel, dim3(y.tiles), dim3(256), 0, s->stream, dsrc.p, y.src_row0.p, 1, s->ld,
                         reinterpret_cast<uint32_t*>(y.tdelta.p), TC, t0, 0u);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->stream));   // (dsrc goes out of scope)
    y.delta_ready = true;
  } else if (f64) {
    // the fused check needs the edge list to BE the block's measured cells and to be on the device in f64
    if (s->list_is_block && !s->dense_mae && s->n_edges > 0 && whole) {
      y.tdelta.alloc((size_t)y.tiles * kSymTileWords);
      HIP_TRY(hipMemsetAsync(y.tdelta.p, 0, (size_t)y.tiles * kSymTileWords * sizeof(float), s->stream));
      hipLaunchKernelGGL(symm64_delta_kernel, dim3(2048), dim3(256), 0, s->stream, s->ei.p, s->ej.p, (const double*)s->et.p,
                         s->ec.p, (long long)s->n_edges, y.tdelta.p, TC, s->n);
      HIP_TRY(hipGetLastError());
      y.delta_ready = true;
    }
  }
  if ((size_t)y.plan.n_units > s->part_sum.n) {   // error partials: one per unit
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipStreamSynchronize(s->check_stream));
    s->part_sum.alloc(y.plan.n_units);
    s->part_cnt.alloc(y.plan.n_units);
  }
  y.generation += 1;
}

template <int DIM>
void sym_prepare(topolow_session* s) {
  sym_build<DIM>(s, {s->enc.p}, {0, s->rows()}, s->any_threshold, 0, -1);
  s->sym.hold(SymHolds::kTriangle);
}

// Builds the sweep's buffers on first use.  They cost device memory (half the encoded block again, plus the
// partials): if the device cannot give it, the session simply keeps the row-owner sweep.
bool sym_available(topolow_session* s) {
  if (s->sym.holds == SymHolds::kTriangle) return true;
  try {
    TL_DISPATCH_SYM(s->dim, sym_prepare, s);
  } catch (const HipError&) {
    (void)hipGetLastError();
    s->sym.release();
    s->sym.allowed = false;
  }
  return s->sym.holds == SymHolds::kTriangle;
}

// ---- launches: records, sweep, apply ----
// The records of iteration `k` from plain positions (all npad of them: the phantom ones too).
template <int DIM>
void sym_records(topolow_session* s, const void* pin, void* rec, double k) {
  sym_real<DIM>(s, [&](auto r) {
    using real = decltype(r);
    hipLaunchKernelGGL((symm_records_kernel<DIM, real>), dim3((s->sym.npad + 255) / 256), dim3(256), 0, s->stream,
                       (const real*)pin, s->gplus.p, (real*)rec, s->n, s->sym.npad, k, s->c_rep);
  });
}

// The sweep of `plan` over the records `rec` into the partials.  err: it also reduces the pending check's MAE into
// part_sum / part_cnt (one partial per unit); block_cells: the count of a threshold-free block (0: none reduced);
// col_row0: the first tile-row of the column partials (a segment's; 0 for the whole triangle); prio: the fp32 sweep's
// issue priority follows the work a wave has left (relax_symm.h) -- for a launch that has the GPU to itself.
template <int DIM>
void sym_sweep(topolow_session* s, const SymPlanDev& plan, const void* rec, bool thr, bool err,
               unsigned long long block_cells, int col_row0, bool prio) {
  auto& y = s->sym;
  if (err && ((size_t)plan.n_units > s->part_sum.n || (size_t)plan.n_units > s->part_cnt.n))
    throw HipError{TOPOLOW_ERR_HIP, "symmetric sweep: the error partials are smaller than the plan's unit count"};
  sym_real<DIM>(s, [&](auto r) {
    using real = decltype(r);
    sym_sweep_instance<DIM, real>(thr, err, s->exact, [&](auto kern) {
      if constexpr (std::is_same<real, double>::value)
        hipLaunchKernelGGL(kern, dim3(y.grid), dim3(64 * kSymWaves), 0, s->stream, y.tenc.p, (const double*)rec,
                           plan.units.p, plan.runs.p, (double*)y.rowpart.p, (double*)y.colpart.p, y.npad, s->state.p,
                           col_row0, y.tdelta.p, s->part_sum.p, s->part_cnt.p, block_cells);
      else
        hipLaunchKernelGGL(kern, dim3(y.grid), dim3(64 * kSymWaves), 0, s->stream, y.tenc.p, (const float*)rec,
                           plan.units.p, plan.runs.p, (float*)y.rowpart.p, (float*)y.colpart.p, y.npad, s->state.p,
                           s->part_sum.p, s->part_cnt.p, block_cells, col_row0, prio && y.prio ? 1 : 0);
    });
  });
}

// f64: whether a sweep may reduce a check's MAE.  Plain f64 sessions: the delta tiles exist (they are made from the edge
// list when it is the block's measured cells).  Exact sessions always have delta tiles, from the matrix; the fused
// check's sum and count run over the block's measured cells, so the list must still be exactly those.
bool sym_fused_ok(const topolow_session* s) {
  if (!s->sym.delta_ready) return false;
  return !s->exact || (s->list_is_block && s->n_edges > 0 && s->sym.holds == SymHolds::kTriangle);
}

// The apply of the whole triangle (rr_stages = 0) or of stage rr_stage of an rr_stages-stage iteration: positions into
// `pout`, the records of k_next into `rec_next`.  chk (nullable): the check whose MAE partials the sweep in front of
// this apply wrote (n_parts of them, of the positions `pin`): one more workgroup runs its controller step.
template <int DIM>
void sym_apply(topolow_session* s, const SymPlanDev& plan, const void* rec, void* rec_next, void* pout, double k_next,
               int iter, int rr_stages, int rr_stage, const PendingCheck* chk = nullptr, const void* pin = nullptr,
               int n_parts = 0) {
  auto& y = s->sym;
  SymApplyCheck ac;
  if (chk != nullptr) {
    ac.part_sum = s->part_sum.p;
    ac.part_cnt = s->part_cnt.p;
    ac.n_parts = n_parts;
    ac.pos = pin;
    ac.best0 = s->best[0].p;
    ac.best1 = s->best[1].p;
    ac.check_no = s->checks_launched;   // (check_went_in_apply counts this one afterwards)
    ac.n_values = (long long)s->n * s->dim;
    ac.iter1 = chk->iter1;
    ac.k_after = chk->k_after;
    ac.trace = s->trace_dev;
    ac.trace_cap = s->trace_cap;
    ac.mailbox = s->mailbox_dev;
  }
  sym_real<DIM>(s, [&](auto r) {
    using real = decltype(r);
    hipLaunchKernelGGL((symm_apply_kernel<DIM, real>), dim3(y.npad / kSymCols + (chk != nullptr ? 1 : 0)),
                       dim3(32 * kSymApplyParts), 0, s->stream,
                       (const real*)rec, (real*)rec_next, (real*)pout, s->gplus.p, (const real*)y.rowpart.p,
                       (const real*)y.colpart.p, plan.row_units.p, s->n, y.npad, k_next, s->c_rep, iter + 1, s->state.p,
                       rr_stages, rr_stage, ac);
  });
}

// Multi-stage iterations on the symmetric sweep (relax_symm.h: sym_rr_*).  The row-owner form of an S-stage iteration gives
// every point its halves of the pairs with one slab of the points per stage, the same slab for everybody; this form
// splits the PAIRS: in stage st every slab a meets its partner slab (st - a) mod S -- every point still meets one slab
// of partners per stage (the stability argument, k / S, is the same), both ends of a pair move in the same stage as in
// the reference (src/optimization.cpp:245-281), and every pair is evaluated once per iteration instead of twice.  The
// order of the stages is drawn per iteration.  S = 2, 4, 8; sixteen stages (the unfolding phase, k > 24) stay row-owner.
bool sym_rr_stages_ok(int S) { return S == 2 || S == 4 || S == 8; }
int sym_rr_log2(int S) { return S == 2 ? 1 : (S == 4 ? 2 : 3); }

// The plan of stage st of an S-stage iteration over npad points for n_waves waves (sym_rr_row: one interval per tile-row).
SymPlan sym_rr_plan(int npad, int n_waves, int S, int st) {
  const int TR = npad / kSymRows;
  return relax_symm_plan_rows(npad, n_waves, [&](int R, int& j0, int& j1) { sym_rr_row(TR, S, st, R, j0, j1); });
}

bool sym_rr_available(topolow_session* s, int S) {
  auto& y = s->sym;
  if (!sym_rr_stages_ok(S) || y.holds != SymHolds::kTriangle) return false;
  const int TR = y.npad / kSymRows;
  if (TR < 2 * S) return false;
  // a stage must give a resident wave about five tiles: below that a wave's prologue and epilogue and the apply kernel
  // cost what the halved pair count saves, or more (config 3, tests/study/two_stage_ab.py: two stages, 6 tiles per wave:
  // a run with k0 = 6 26.1 against 27.6 ms on the row-owner stages; four stages, 3 tiles: +25 us per iteration; eight
  // stages, 1.5 tiles: 16.0 against 13.0 ms per run with k0 = 20)
  if ((long long)TR * (TR + 1) / S < (long long)y.rr_min_tiles * y.grid * kSymWaves) return false;
  const int lg = sym_rr_log2(S);
  if (!y.rr[lg].empty()) return true;
  std::vector<SymPlanDev> plans(S);
  for (int st = 0; st < S; ++st) {
    const SymPlan hp = sym_rr_plan(y.npad, y.grid * kSymWaves, S, st);
    if (hp.units.size() * kSymRows * s->dim * s->real_size() > y.rowpart.n) return false;   // (never: sym_build sizes for it)
    plans[st].load(hp);
  }
  y.rr[lg] = std::move(plans);
  return true;
}

// One symmetric sweep + apply from `pin` into `pout`: a whole one-stage iteration (S = 0), or stage st of an S-stage
// iteration (the tiles of rr[log2 S][st]).  The records of this iteration are built from `pin` unless the previous apply
// left them; the apply leaves the next sweep's: this iteration's, or after the iteration's last sweep (`last`) the next
// one's.  err: the sweep also reduces the pending check's MAE (positions read = that check's positions).  in_apply
// (nullable, with err on a whole sweep only): that check, whose controller step then runs in the apply's launch.
template <int DIM>
void sym_iteration(topolow_session* s, const void* pin, void* pout, int iter, double k, bool err, int S = 0, int st = 0,
                   bool last = true, const PendingCheck* in_apply = nullptr) {
  auto& y = s->sym;
  const SymPlanDev& plan = S == 0 ? y.plan : y.rr[sym_rr_log2(S)][st];
  ProfScope prof(s, S > 0 ? &s->prof_stage : err ? &s->prof_sym_err : &s->prof_sym);
  if (err && s->precision == TOPOLOW_PRECISION_F64 && !sym_fused_ok(s))
    throw HipError{TOPOLOW_ERR_UNSUPPORTED, "symmetric sweep (f64): no delta tiles for a fused check"};
  if (y.rec_iter != iter) {
    for (int b = 0; b < 2; ++b)   // both buffers need the phantom records; the second one's points are overwritten by the apply
      sym_records<DIM>(s, pin, y.rec[b].p, k);
    y.rec_cur = 0;
  }
  sym_sweep<DIM>(s, plan, y.rec[y.rec_cur].p, s->any_threshold, err, S == 0 ? s->block_cells : 0ull, 0, true);
  if (in_apply != nullptr && !(err && S == 0))
    throw HipError{TOPOLOW_ERR_BAD_ARGUMENT, "symmetric sweep: a check in the apply needs the ERR sweep of a one-stage iteration"};
  sym_apply<DIM>(s, plan, y.rec[y.rec_cur].p, y.rec[y.rec_cur ^ 1].p, pout, last ? k * (1.0 - s->cooling) : k, iter, S, st,
                 in_apply, pin, plan.n_units);
  HIP_TRY(hipGetLastError());
  y.rec_cur ^= 1;
  y.rec_iter = last ? iter + 1 : iter;
  if (err) s->fused_parts = plan.n_units;
  s->stage_launches += 1;
}

// How an iteration of n_stages stages runs on a whole-matrix session: one symmetric sweep (one stage), S sweeps over the
// tiles of one stage each (S = 2, 4, 8), or the row-owner stage kernel.  Builds the sweep on first use.
enum class SymForm { kRowOwner, kSweep, kStages };
SymForm sym_form(topolow_session* s, int n_stages) {
  if (n_stages == 1) return sym_eligible(s) && sym_available(s) ? SymForm::kSweep : SymForm::kRowOwner;
  return s->sym.two_stage && sym_rr_stages_ok(n_stages) && sym_eligible(s) && sym_available(s) &&
                 sym_rr_available(s, n_stages)
             ? SymForm::kStages
             : SymForm::kRowOwner;
}

// The stages of iteration `iter` at k: the run's fixed count or the schedule's, as the slab geometry of n points has them.
int iteration_stages(const topolow_session* s, int iter, double k) {
  return slab_geom(s->n, s->fixed_stages > 0 ? s->fixed_stages : slab_stages_at(iter, k, s->dim)).n_stages;
}

// Whether a convergence check follows iteration `iter` (reference :294).
bool check_after(const topolow_session* s, int iter) { return (iter + 1) % s->check_freq == 0 || iter == s->n_iter - 1; }

// How iteration `iter` runs at k: its stages, their form (a row block of several has n_push > 0: always row-owner), and
// for SymForm::kStages the order of the stages (drawn per iteration).
struct IterPlan {
  SlabGeom geo;
  SymForm form;
  int order[8];
};
IterPlan plan_iteration(topolow_session* s, int iter, double k) {
  IterPlan p;
  p.geo = slab_geom(s->n, iteration_stages(s, iter, k));
  p.form = sym_form(s, p.geo.n_stages);
  if (p.form == SymForm::kStages) sym_rr_order(s->seed, iter, p.geo.n_stages, p.order);
  return p;
}

// Enqueues stage t of iteration `iter` in the form p names, from pin into pout: the whole sweep, stage t's sweep, or the
// row-owner slab t (push: the other blocks' copies of pout, n_push of them).  err: the launch also reduces the pending
// check's MAE of pin; in_apply (nullable, SymForm::kSweep with err only): that check, run in the sweep's apply launch.
// Returns the error partials it wrote (0 without err).
int enqueue_stage(topolow_session* s, const IterPlan& p, int t, const void* pin, void* pout, int iter, double k,
                  const void* push, int n_push, bool err, const PendingCheck* in_apply = nullptr) {
  if (in_apply != nullptr && p.form != SymForm::kSweep)
    throw HipError{TOPOLOW_ERR_BAD_ARGUMENT, "a check in the apply needs a one-stage symmetric sweep"};
  if (p.form == SymForm::kRowOwner) {
    TL_DISPATCH_DIM(s->dim, launch_stage, s, pin, pout, s->state.p, slab_ranges(p.geo, s->seed, iter, t), iter + 1, k,
                    push, n_push, err);
    if (err) s->fused_parts = (s->rows() + CfgProd::ROWS - 1) / CfgProd::ROWS;
  } else if (p.form == SymForm::kSweep) {   // one sweep over the upper triangle moves both ends of every pair
    TL_DISPATCH_SYM(s->dim, sym_iteration, s, pin, pout, iter, k, err, 0, 0, true, in_apply);
  } else {   // S symmetric sweeps over the tiles of one stage each, in random order
    const int S = p.geo.n_stages;
    TL_DISPATCH_SYM(s->dim, sym_iteration, s, pin, pout, iter, k, err, S, p.order[t], t == S - 1);
  }
  return err ? s->fused_parts : 0;
}

// Whether a check may be fused into an iteration of n_stages stages: the iteration's one sweep reduces the MAE of the
// positions it reads.  The row-owner ERR instance pairs rows two by two (an odd block keeps the separate pass), the
// symmetric sweep's has no such rule; f64 fuses into the symmetric sweep only, exact through its delta tiles (asked
// first: an f64 session builds its sweep at its first check).
bool check_fusable(topolow_session* s, int n_stages) {
  if (s->precision == TOPOLOW_PRECISION_F64)
    return sym_form(s, 1) == SymForm::kSweep && sym_fused_ok(s) && n_stages == 1;
  return n_stages == 1 && (s->rows() % 2 == 0 || sym_form(s, 1) == SymForm::kSweep);
}

// ---- the symmetric sweep sharded over the row-block sessions of one run (relax_symm.h; the engine below) ----
// Segment b of P of the sweep over n points: tiles [t0, t1), equal runs of the tile-row-major list of the upper
// triangle (`total` tiles); tile-rows [r_first, r_last] hold its tiles (-1: none).
struct SymSegment {
  long long total, t0, t1;
  int r_first = -1, r_last = -1;
};
SymSegment sym_segment(int n, int b, int P) {
  SymSegment g;
  const int npad = (n + kSymRows - 1) & ~(kSymRows - 1), TR = npad / kSymRows;
  g.total = (long long)TR * (TR + 1);
  g.t0 = g.total * b / P;
  g.t1 = g.total * (b + 1) / P;
  (void)relax_symm_plan(npad, 1, g.t0, g.t1, &g.r_first, &g.r_last);
  return g;
}

bool sym_sharded_eligible(const std::vector<topolow_session*>& ss) {
  const char* e = getenv("TOPOLOW_SHARD_SYMMETRIC");
  if (e != nullptr && e[0] == '0') return false;       // row-owner sweeps only
  const int P = (int)ss.size();
  if (P < 2) return false;
  const topolow_session* a = ss[0];
  const long long TR = ((a->n + kSymRows - 1) & ~(kSymRows - 1)) / kSymRows;
  if (TR * (TR + 1) < 8ll * P) return false;
  for (const topolow_session* s : ss)
    if (!(sym_shape_ok(s) && s->precision == TOPOLOW_PRECISION_F32 && s->rows() > 0 && s->fuse_checks == a->fuse_checks))
      return false;
  return true;
}

// The table of the inboxes a segment's folded partials go to, one per owner.  With it the segment is complete: the
// buffers hold `kind`.
void sym_wire_inboxes(topolow_session* s, const std::vector<float*>& tab, SymHolds kind) {
  s->sym.inbox_tab.alloc(tab.size());
  HIP_TRY(hipMemcpy(s->sym.inbox_tab.p, tab.data(), tab.size() * sizeof(float*), hipMemcpyHostToDevice));
  s->sym.hold(kind);
}

// What follows sym_build for a segment of either kind: its slot, its inbox (`slots` zeroed slots of npad x DIM floats for
// every session's folded partials of this session's points), own0: the first row of every owner, then n.  Returns with
// the tile-major copy complete.  A run segment's table needs every session's inbox: sym_sharded_prepare.
template <int DIM>
void sym_install_segment(topolow_session* s, SymHolds kind, bool any_thr, int slots, int slot, const std::vector<int>& own0,
                         topolow_session::SymState::Sources from = {}) {
  auto& y = s->sym;
  if (y.seg_first < 0) { y.seg_first = 0; y.seg_last = -1; }
  y.seg_thr = any_thr;
  y.seg_slots = slots;
  y.seg_slot = slot;
  y.inbox.alloc((size_t)slots * y.npad * DIM);
  HIP_TRY(hipMemsetAsync(y.inbox.p, 0, (size_t)slots * y.npad * DIM * sizeof(float), s->stream));
  y.own0.alloc(own0.size());
  HIP_TRY(hipMemcpy(y.own0.p, own0.data(), own0.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipStreamSynchronize(s->stream));
  y.seg_from = std::move(from);
  if (kind == SymHolds::kCallerSegment) sym_wire_inboxes(s, {y.inbox.p}, kind);
}

// Session b's segment: tiles [total b / P, total (b + 1) / P) of the tile-row-major list, gathered from every session's
// row block (peer reads where the sessions sit on different GPUs).  Kept while the same sessions, in the same order (so
// the same slot), run together again on the blocks it was gathered from.
template <int DIM>
void sym_sharded_build(std::vector<topolow_session*>& ss, int b) {
  const int P = (int)ss.size();
  topolow_session* s = ss[b];
  std::vector<const uint32_t*> src;
  topolow_session::SymState::Sources from;
  std::vector<int> row0;
  bool any_thr = false;
  for (topolow_session* q : ss) {
    src.push_back(q->enc.p);
    from.emplace_back(q->enc.p, q->block_gen);
    row0.push_back(q->row_begin);
    any_thr = any_thr || q->any_threshold;
  }
  row0.push_back(s->n);
  const auto& y = s->sym;
  if (y.holds == SymHolds::kRunSegment && y.seg_from == from && y.seg_thr == any_thr) return;
  HIP_TRY(hipSetDevice(s->device));
  const SymSegment g = sym_segment(s->n, b, P);
  sym_build<DIM>(s, src, row0, any_thr, g.t0, g.t1);
  sym_install_segment<DIM>(s, SymHolds::kRunSegment, any_thr, P, s->rank, row0, std::move(from));
}

void sym_sharded_prepare(std::vector<topolow_session*>& ss) {
  const int P = (int)ss.size();
  for (topolow_session* s : ss) {   // every block is loaded before anybody gathers from it
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());
  }
  for (int b = 0; b < P; ++b) TL_DISPATCH_SYM(ss[b]->dim, sym_sharded_build, ss, b);
  for (int b = 0; b < P; ++b) {
    topolow_session* s = ss[b];
    HIP_TRY(hipSetDevice(s->device));
    // a segment meets points of every row block: their degree terms come from the owners (a caller that fills a
    // block in place -- topolow_session_commit_encoded -- need only know its own rows' degrees)
    for (topolow_session* q : ss)
      if (q != s && q->rows() > 0)
        HIP_TRY(hipMemcpy(s->gplus.p + q->row_begin, q->gplus.p + q->row_begin, (size_t)q->rows() * sizeof(float),
                          hipMemcpyDeviceToDevice));
    std::vector<float*> tab;
    for (topolow_session* q : ss) tab.push_back(q->sym.inbox.p);
    sym_wire_inboxes(s, tab, SymHolds::kRunSegment);
  }
}

// First half of a one-stage iteration of session s: records of all points from `pin`, the sweep of its segment, its
// partials folded per point into slot `rank` of the owners' inboxes.  err: the sweep also reduces its pairs' share of
// the pending check's MAE (one partial per unit: s->fused_parts).
template <int DIM>
void sym_sharded_sweep(topolow_session* s, const void* pin, int iter, double k, bool err) {
  auto& y = s->sym;
  ProfScope prof(s, err ? &s->prof_sym_err : &s->prof_sym);
  sym_records<DIM>(s, pin, y.rec[0].p, k);
  if (y.tiles > 0) sym_sweep<DIM>(s, y.plan, y.rec[0].p, y.seg_thr, err, s->block_cells, y.seg_first,
                                  false);   // several sessions may share a GPU here: every wave stays at priority 0
  hipLaunchKernelGGL(symm_partial_kernel<DIM>, dim3(y.npad / kSymCols), dim3(32 * 32), 0, s->stream, (const float*)y.rowpart.p,
                     (const float*)y.colpart.p, y.plan.row_units.p, y.seg_first, y.seg_last, s->n, y.npad, y.inbox_tab.p,
                     y.own0.p, y.seg_slots, y.seg_slot, s->state.p);
  HIP_TRY(hipGetLastError());
  if (err) s->fused_parts = y.plan.n_units;
  (void)iter;
  s->stage_launches += 1;
}

// Second half, behind the run's barrier (or the caller's sum over the processes): the points [row_begin, row_end) move
// by the sum of the inbox's slots; `push`: the other sessions' copies of the output buffer (n_push of them).
template <int DIM>
void sym_owner_apply(topolow_session* s, const void* pin, void* pout, int row_begin, int row_end, const void* push,
                     int n_push, int iter) {
  auto& y = s->sym;
  hipLaunchKernelGGL(symm_owner_apply_kernel<DIM>, dim3((row_end - row_begin + 255) / 256), dim3(256), 0, s->stream,
                     (const float*)pin, (float*)pout, y.inbox.p, y.seg_slots, y.npad, row_begin, row_end,
                     (float* const*)push, n_push, iter + 1, s->state.p);
  HIP_TRY(hipGetLastError());
}

// ---- the same sweep sharded over caller-driven sessions (one process per GPU: topolow_session_symm_segment_*) ----
// The segment of this session, built from the rows the caller brought together; ONE slot and ONE owner: the folded
// partials of all n points land in the session's own inbox (the "moves buffer"), which the caller sums over the
// processes; the apply then moves ALL points from it.
template <int DIM>
void sym_segment_build(topolow_session* s, int segment, int P, const uint32_t* d_rows, int row_first, int n_rows,
                       bool any_thr) {
  const SymSegment g = sym_segment(s->n, segment, P);
  if (g.r_first >= 0 && (row_first > g.r_first * kSymRows ||
                         row_first + n_rows < std::min<long long>(s->n, (long long)(g.r_last + 1) * kSymRows)))
    throw HipError{TOPOLOW_ERR_BAD_ARGUMENT, "symm_segment_build: d_rows does not hold the rows of the segment's tiles"};
  sym_build<DIM>(s, {d_rows}, {row_first, row_first + n_rows}, any_thr, g.t0, g.t1);
  sym_install_segment<DIM>(s, SymHolds::kCallerSegment, any_thr, 1, 0, {0, s->n});   // (the caller may free d_rows now)
}

// One convergence check of the session's own loop.  error_pass = true: the separate pass over the block (or
// the edge list) + the controller; false: the partials were written by the stage kernel just launched
// (ERR launch), only the controller follows.  pc.beside: on the check stream, beside the next stages.
void launch_check(topolow_session* s, PendingCheck& pc, bool error_pass) {
  hipStream_t check_on = s->stream;
  if (pc.beside) {
    HIP_TRY(hipEventRecord(s->ev_iter_done, s->stream));
    HIP_TRY(hipStreamWaitEvent(s->check_stream, s->ev_iter_done, 0));
    check_on = s->check_stream;
  }
  {
    StreamScope on(s, check_on);
    ProfScope prof(s, &s->prof_check);
    if (error_pass) {
      TL_DISPATCH_DIM(s->dim, launch_edge_error, s, s->pos[pc.buf].p, s->state.p);
      launch_controller(s, s->pos[pc.buf].p, pc.iter1, pc.k_after);
    } else {
      launch_controller(s, s->pos[pc.buf].p, pc.iter1, pc.k_after, s->part_sum.p, s->part_cnt.p, s->fused_parts);
    }
  }
  if (pc.beside) HIP_TRY(hipEventRecord(s->ev_check_done, check_on));
  hipEvent_t e = take_event(s);
  HIP_TRY(hipEventRecord(e, check_on));
  s->pending.push_back(e);
  s->checks_launched += 1;
  poll_checks(s, 3);
  pc.active = false;
}

// The host side of a check whose controller step went out in an apply's launch (sym_apply): nothing is put on a stream
// for it.  The host still has to see a stop and to stay at most three checks ahead, and reads both from the pinned
// mailbox, which every controller step mirrors the run state to (n_checks counts the steps that ran, whichever kernel
// ran them; after a stop they no longer count, and `stopped` ends the wait).  No event is recorded behind the apply: a
// marker between an apply and the next sweep is part of what this path removes.  The wait is
// bounded: a check completes every few hundred microseconds, and once per millisecond of waiting the stream is queried --
// idle (the mailbox is final) or failed (the next HIP call reports it) ends the wait.
void check_went_in_apply(topolow_session* s, PendingCheck& pc) {
  s->checks_launched += 1;
  s->checks_in_apply += 1;
  pc.active = false;
  const volatile RunState* mb = s->mailbox;
  double asked = now_s();
  while (!mb->stopped && s->checks_launched - mb->n_checks > 3) {
    if (now_s() - asked < 1e-3) continue;
    if (hipStreamQuery(s->stream) != hipErrorNotReady) break;
    (void)hipGetLastError();   // "not ready" is no error of a launch
    asked = now_s();
  }
  if (mb->stopped) s->host_seen_stop = true;
}

// A check that was waiting for the next iteration's kernel and will not get one (the caller stopped
// enqueueing, or asks for results): run it as a separate pass now.
void flush_pending_check(topolow_session* s) {
  if (s->pcheck.active) launch_check(s, s->pcheck, /*error_pass=*/true);
}

// Reference :359-361: positions are inspected after every 10th iteration, after that iteration's convergence check
// (which may already have stopped the run).  The iteration to report for the first non-finite result (0x7fffffff:
// none) of a run that ran `ran` iterations, or 0.
int nonfinite_report(int first_nonfinite, int ran, bool stopped) {
  if (first_nonfinite == 0x7fffffff) return 0;
  const int t = ((first_nonfinite + 9) / 10) * 10;
  return t <= ran && !(stopped && t == ran) ? t : 0;
}

// ---- a cross-validation fold on a resident session (relax_cv.h) ---------------------------
// ---- the convergence edge list of a session: what topolow_session_set_edges (a host list) and
// topolow_session_load_prepared (a device list) share ----

// The sizes every check kernel reads and the partial buffers, for a list of n_edges; the flags start at "gather the list".
void edges_begin(topolow_session* s, int64_t n_edges) {
  s->n_edges = n_edges;
  s->cv.list_compacted = false;
  if (s->precision == TOPOLOW_PRECISION_F64) s->sym.invalidate();   // its delta tiles are made from this list: rebuilt on first use
  s->n_parts = edge_error_blocks(n_edges);
  // dense MAE pass: one workgroup per (column chunk, 64-row tile)
  s->dense_grid_x = (((s->n + 3) & ~3) + ErrCfg::CHUNK - 1) / ErrCfg::CHUNK;
  s->dense_grid_y = (s->rows() + kErrTileRows - 1) / kErrTileRows;
  s->dense_blocks = s->dense_grid_x * s->dense_grid_y;
  const int stage_blocks = (s->rows() + CfgProd::ROWS - 1) / CfgProd::ROWS;   // fused checks: one partial per workgroup
  // ... and one per unit of a sweep plan the session still holds: an fp32 session keeps its sweep buffers across a new
  // edge list, and sym_build sizes the partials at build time only (the edge-list bookkeeping)
  int parts = std::max({s->n_parts, s->dense_blocks, stage_blocks, s->sym.plan.n_units});
  for (const auto& plans : s->sym.rr)
    for (const auto& p : plans) parts = std::max(parts, p.n_units);
  s->part_sum.alloc(parts);
  s->part_cnt.alloc(parts);
  s->dense_mae = false;
  s->dense_parity = !(s->row_begin == 0 && s->row_end == s->n);
  s->list_is_block = false;
}

// TOPOLOW_EDGE_MAE=1: always the edge-list pass
bool edge_mae_forced() {
  const char* force = getenv("TOPOLOW_EDGE_MAE");
  return force && atoi(force) != 0;
}

// h[0]: the order-independent fingerprint, h[1]: the number of the measured cells the dense MAE pass would reduce.
void block_fingerprint(topolow_session* s, unsigned long long h[2]) {
  DevBuf<unsigned long long> d_fp;
  d_fp.alloc(2);
  // on the session's stream: it is non-blocking, a null-stream memset is not ordered with it
  HIP_TRY(hipMemsetAsync(d_fp.p, 0, 16, s->stream));
  hipLaunchKernelGGL(upper_fingerprint_kernel, dim3(s->rows()), dim3(kThreads), 0, s->stream,
                     s->enc.p, s->n, s->row_begin, s->row_end, s->ld, s->dense_parity ? 1 : 0,
                     d_fp.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipMemcpy(h, d_fp.p, 16, hipMemcpyDeviceToHost));
}

// The list is (or is not) exactly the block's measured cells.
// (f64 sessions keep the exact edge-list pass: the block holds 4-byte targets; their symmetric sweep fuses the
//  check through the delta tiles instead, relax_symm64.h)
void edges_decide(topolow_session* s, bool list_is_block) {
  s->list_is_block = list_is_block;
  s->dense_mae = list_is_block && s->dim <= kMaxTunedDim && s->precision == TOPOLOW_PRECISION_F32;
}

// dense MAE: the gather fallback is not needed, the session keeps 1-element placeholders.  true: that was done.
bool edges_placeholders(topolow_session* s) {
  if (!s->dense_mae) return false;
  s->ei.alloc(1); s->ej.alloc(1); s->ec.alloc(1); s->et.alloc(8);
  return true;
}

template <typename T>
void swap_buf(DevBuf<T>& a, DevBuf<T>& b) { std::swap(a.p, b.p); std::swap(a.n, b.n); }

unsigned pair_grid(long long n_pairs) { return (unsigned)((n_pairs + kThreads - 1) / kThreads); }

// The device edge list without the edges whose cell carries kHeldMark: written to the spare list, swapped in.
void cv_compact_edges(topolow_session* s) {
  auto& h = s->cv;
  const long long m = s->n_edges;
  const int nb = (int)std::max<long long>(1, (m + kThreads - 1) / kThreads);
  grow_buf(h.blk_count, (size_t)nb);
  grow_buf(h.blk_offset, (size_t)nb + 1);
  grow_buf(h.ei, (size_t)m); grow_buf(h.ej, (size_t)m); grow_buf(h.ec, (size_t)m);
  grow_buf(h.et, (size_t)m * s->real_size());
  hipLaunchKernelGGL(cv_edges_count_kernel, dim3(nb), dim3(kThreads), 0, s->stream, s->ei.p, s->ej.p, m, s->enc.p, s->ld,
                     s->n, h.blk_count.p);
  hipLaunchKernelGGL(cv_scan_kernel, dim3(1), dim3(1024), 0, s->stream, h.blk_count.p, nb, h.blk_offset.p);
  if (s->precision == TOPOLOW_PRECISION_F64)
    hipLaunchKernelGGL((cv_edges_compact_kernel<double>), dim3(nb), dim3(kThreads), 0, s->stream, s->ei.p, s->ej.p,
                       (const double*)s->et.p, s->ec.p, m, s->enc.p, s->ld, s->n, h.blk_offset.p, h.ei.p, h.ej.p,
                       (double*)h.et.p, h.ec.p);
  else
    hipLaunchKernelGGL((cv_edges_compact_kernel<float>), dim3(nb), dim3(kThreads), 0, s->stream, s->ei.p, s->ej.p,
                       (const float*)s->et.p, s->ec.p, m, s->enc.p, s->ld, s->n, h.blk_offset.p, h.ei.p, h.ej.p,
                       (float*)h.et.p, h.ec.p);
  HIP_TRY(hipGetLastError());
  long long kept = 0;
  HIP_TRY(hipMemcpyAsync(&kept, h.blk_offset.p + nb, sizeof kept, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  swap_buf(s->ei, h.ei); swap_buf(s->ej, h.ej); swap_buf(s->et, h.et); swap_buf(s->ec, h.ec);
  h.full_edges = m;
  h.full_parts = s->n_parts;
  s->n_edges = kept;
  s->n_parts = edge_error_blocks(kept);
  h.list_compacted = true;
}

// Flags, threshold bit and cell count of the patched block.  copy_patched: the sweep holds the triangle and its copy took
// the same patch: it stays unless the threshold bit flipped, which changes the sweep's kernel instance and with it its
// grid and plan.  Anything else the sweep holds is invalid: rebuilt, from the block as it is now, on first use.
void cv_refresh_flags(topolow_session* s, bool copy_patched) {
  const bool before = s->any_threshold;
  scan_row_flags(s);
  if (!copy_patched || s->any_threshold != before) {
    s->sym.invalidate();
    s->cv.tiles_patched = false;
  }
}

int cv_check_session(const topolow_session* s, char* errbuf, size_t errlen) {
  if (!(s->row_begin == 0 && s->row_end == s->n)) {
    set_err(errbuf, errlen, "folds are held out of whole-problem sessions only (this one holds rows [%d, %d) of %d)",
            s->row_begin, s->row_end, s->n);
    return TOPOLOW_ERR_UNSUPPORTED;
  }
  if (!s->gplus.p || !s->part_sum.p) {
    set_err(errbuf, errlen, "session needs its targets loaded and its edges set first");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (s->in_run) {
    set_err(errbuf, errlen, "not during a run: between topolow_session_finish and the next topolow_session_begin only");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  return TOPOLOW_OK;
}

}  // namespace

// ---- the three functions topolow_prep_fold.hip calls as well (declared in topolow_session.h) ----

// The device half of a hold-out, shared by topolow_session_hold_out and the folds prepared on the device
// (topolow_layout_prep_cv_sweep).  fill(lo, hi) enqueues on s->stream whatever writes the n_pairs held-out pairs into
// the two device arrays: session labels, lo < hi, every pair once, in ANY order -- the mask, tile and compaction
// kernels of relax_cv.h need the pairs unique, not sorted.  degrees: the fold's, per caller's point (host).
void cv_hold_out_pairs(topolow_session* s, long long np, const int32_t* degrees, const std::function<void(int*, int*)>& fill) {
  auto& h = s->cv;
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipStreamSynchronize(s->check_stream));
  // the sweep's copy is built from the FULL block once and patched fold after fold
  if (sym_eligible(s)) (void)sym_available(s);
  grow_buf(h.lo, (size_t)np); grow_buf(h.hi, (size_t)np); grow_buf(h.words, 2 * (size_t)np); grow_buf(h.deltas, (size_t)np);
  h.n_pairs = np;
  h.tiles_patched = false;
  h.list_compacted = false;
  const bool gathers = !s->dense_mae;
  if (np > 0) {
    fill(h.lo.p, h.hi.p);
    hipLaunchKernelGGL(cv_mask_kernel, dim3(pair_grid(np)), dim3(kThreads), 0, s->stream, h.lo.p, h.hi.p, np, s->enc.p,
                       s->ld, h.words.p, gathers ? kHeldMark : kInfWord);
    HIP_TRY(hipGetLastError());
  }
  if (gathers) {
    cv_compact_edges(s);
    if (np > 0)
      hipLaunchKernelGGL(cv_mask_kernel, dim3(pair_grid(np)), dim3(kThreads), 0, s->stream, h.lo.p, h.hi.p, np,
                         s->enc.p, s->ld, (uint32_t*)nullptr, kInfWord);
    HIP_TRY(hipGetLastError());
  }
  if (s->sym.holds == SymHolds::kTriangle) {
    if (np > 0)
      hipLaunchKernelGGL(cv_tiles_kernel, dim3(pair_grid(np)), dim3(kThreads), 0, s->stream, h.lo.p, h.hi.p, np,
                         s->sym.tenc.p, s->sym.delta_ready ? s->sym.tdelta.p : (float*)nullptr, s->sym.npad / kSymCols,
                         (const uint32_t*)nullptr, h.deltas.p);
    HIP_TRY(hipGetLastError());
    h.tiles_patched = true;
    h.generation = s->sym.generation;
  }
  cv_refresh_flags(s, h.tiles_patched);
  upload_degrees(s, degrees);
  HIP_TRY(hipStreamSynchronize(s->stream));   // (whatever fill() read from the host may go out of scope)
  h.active = true;
}

// What a session refuses a hold-out for, whoever brings the pairs.
int cv_check_hold_out(const topolow_session* s, char* errbuf, size_t errlen) {
  const int rc0 = cv_check_session(s, errbuf, errlen);
  if (rc0 != TOPOLOW_OK) return rc0;
  if (s->exact) {
    set_err(errbuf, errlen, "precision f64_exact: folds cannot be held out of the session (the patch does not cover the delta block)");
    return TOPOLOW_ERR_UNSUPPORTED;
  }
  if (s->cv.active) {
    set_err(errbuf, errlen, "a fold is held out already: topolow_session_restore_held_out first");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  return TOPOLOW_OK;
}

// The device half of topolow_session_score_pairs: n_pairs > 0 pairs in SESSION labels with their truths, all three on
// the device.  One partial per workgroup, the blocks fixed by n_pairs alone, summed by the host in index order: the
// same pairs in the same order give the same bits wherever they came from.
void cv_score_device(topolow_session* s, const int* d_i, const int* d_j, const double* d_truth, long long n_pairs,
                     double* sum_abs, int64_t* count) {
  auto& h = s->cv;
  const int blocks = (int)std::min<long long>(1024, (n_pairs + kThreads - 1) / kThreads);   // fixed by n_pairs alone
  grow_buf(h.sc_part, 1024);
  if (s->precision == TOPOLOW_PRECISION_F64)
    hipLaunchKernelGGL((cv_score_kernel<double>), dim3(blocks), dim3(kThreads), 0, s->stream, (const double*)s->best_now(),
                       s->dim, d_i, d_j, d_truth, n_pairs, h.sc_part.p);
  else
    hipLaunchKernelGGL((cv_score_kernel<float>), dim3(blocks), dim3(kThreads), 0, s->stream, (const float*)s->best_now(),
                       s->dim, d_i, d_j, d_truth, n_pairs, h.sc_part.p);
  HIP_TRY(hipGetLastError());
  std::vector<double> part((size_t)blocks);
  HIP_TRY(hipMemcpyAsync(part.data(), h.sc_part.p, (size_t)blocks * 8, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  double total = 0.0;
  for (int b = 0; b < blocks; ++b) total += part[(size_t)b];
  if (sum_abs) *sum_abs = total;
  if (count) *count = n_pairs;
}

// =========================================================================================
// Row-sharded engine: ONE embedding relaxed over several row-block sessions, driven from one process (an R session
// is one process: reference src/RcppExports.cpp:16-39)
// =========================================================================================
// Layout: block b owns rows [row_begin_b, row_end_b) of the encoded target
// matrix and moves only its own points; every block keeps ALL n positions (they are tiny).  Per slab
// stage:
//   * block b's stage kernel writes its updated rows into its own next-position buffer AND, from the
//     same epilogue, into the next-position buffer of every other block (peer stores -- over xGMI when
//     the blocks sit on different GPUs): the all-gather of the position slices is fused into the
//     kernel, there is no separate collective and no staging copy;
//   * a barrier between the GPUs out of HIP events: every GPU's thread records an event behind its
//     stage kernels and makes its stream wait for the events of the others (blocks that share a GPU share
//     a stream: stream order is their barrier).  Peer-written data is consumed only by
//     kernels that START after that wait -- kernel-boundary visibility, the guarantee HIP gives for
//     ordinary (coarse-grained) device memory; nothing spins inside a kernel on a remote flag.
// Per convergence check each block reduces its parity share of the measured pairs, folds the
// partials into one (sum, count) and peer-stores it into a slot of every block's rank table; after
// one more barrier every block runs the SAME controller on the SAME numbers in the same order, so
// the decisions (stop / snapshot) are replicated without any host round trip.
// One host thread per GPU enqueues that GPU's work (the event waits are per pair of GPUs, a single
// thread would issue G^2 of them per stage); threads meet in a spin barrier between "record" and
// "wait" so an event is always recorded before anyone waits on it.  The calling thread is the first
// GPU's thread: only it polls the caller's interrupt callback (R's API is main-thread only).
// Measured on one MI355X (tests/study/shard_exchange_latency.py): with every block forced into its own
// thread and stream the barrier costs 27 / 62 / 198 us per stage at 2 / 4 / 8 blocks -- eight threads
// issuing 72 event calls per stage into ONE device's runtime lock; that is why same-GPU blocks share a
// stream, and it is the upper bound of what 8 GPUs (one lock each, 9 calls per thread) can cost.
namespace {

struct ShardedAbortableBarrier {
  std::atomic<int> count{0};
  std::atomic<int> sense{0};
  std::atomic<bool> failed{false};
  int n;
  explicit ShardedAbortableBarrier(int n_) : n(n_) {}
  // false: some thread failed (it never arrives); the caller must unwind
  bool wait() {
    const int s = sense.load(std::memory_order_acquire);
    if (count.fetch_add(1, std::memory_order_acq_rel) == n - 1) {
      count.store(0, std::memory_order_relaxed);
      sense.store(s ^ 1, std::memory_order_release);
      return !failed.load(std::memory_order_acquire);
    }
    int spins = 0;
    while (sense.load(std::memory_order_acquire) == s) {
      if (failed.load(std::memory_order_acquire)) return false;
      if (++spins > 4000) std::this_thread::yield();
    }
    return !failed.load(std::memory_order_acquire);
  }
  void fail() { failed.store(true, std::memory_order_release); }
};

// Blocks that share a GPU form a GROUP: one host thread enqueues all of them on ONE stream, stage by
// stage, so stream order is their barrier (their kernels each fill the chip anyway).  Groups -- i.e.
// different GPUs, one block each in production -- meet at the event barrier.  TOPOLOW_SHARD_THREAD_PER_BLOCK=1
// makes every block its own group (tests drive the cross-group path on one GPU with it).
struct ShardedGroup {
  std::vector<int> blocks;     // indices into ShardedRun::ss, ascending
  hipStream_t stream = nullptr;
  int device = 0;
};

struct ShardedRun {
  std::vector<topolow_session*> ss;
  std::vector<ShardedGroup> groups;
  std::vector<std::array<hipEvent_t, 2>> ev;      // per group
  ShardedAbortableBarrier* bar = nullptr;
  std::atomic<int> flag[2];      // published by group 0's thread before barrier g (slot g & 1): bit 0 stop, bit 1 interrupt
  int32_t (*interrupt_cb)(void*) = nullptr;
  void* interrupt_user = nullptr;
  std::mutex err_mu;
  HipError first_error{TOPOLOW_OK, ""};
  int warmup_iters = 0;          // > 0: the clock of `timed_seconds` starts when these iterations have drained
  double t_timed0 = 0.0;
  bool pair_sharded = false;     // one-stage iterations run as the symmetric sweep sharded over the sessions (relax_symm.h)
  // results of the loop
  int iters_enqueued = 0;
  bool interrupted = false;
  long long exchanges = 0;
};

// One group's enqueue loop (thread r).  Throws HipError; the caller marks the barrier failed.
void sharded_worker(ShardedRun& R, int r) {
  const ShardedGroup& G = R.groups[r];
  const int n_groups = (int)R.groups.size();
  topolow_session* lead = R.ss[G.blocks[0]];
  HIP_TRY(hipSetDevice(G.device));
  long long g = 0;          // exchange counter, identical in every thread
  int seen = 0;             // flag value read at the last exchange, identical in every thread
  auto exchange = [&]() -> bool {
    int f = 0;
    if (r == 0) {
      f = R.ss[0]->mailbox->stopped ? 1 : 0;
      if (R.interrupted) f |= 2;
    }
    if (n_groups == 1) { seen = f; ++g; return true; }   // stream order is the barrier
    HIP_TRY(hipEventRecord(R.ev[r][g & 1], G.stream));
    if (r == 0) R.flag[g & 1].store(f, std::memory_order_release);
    if (!R.bar->wait()) return false;
    for (int p = 0; p < n_groups; ++p)
      if (p != r) HIP_TRY(hipStreamWaitEvent(G.stream, R.ev[p][g & 1], 0));
    seen = R.flag[g & 1].load(std::memory_order_acquire);
    ++g;
    return true;
  };
  // The run's parameters are every session's (topolow_session_begin); the schedule is the lead block's.
  const int P = (int)R.ss.size();
  int cur = 0;
  double k = lead->k0;
  int iter = 0;
  // Position buffers rotate through three: a stage reads `cur` and writes (own rows, and the other blocks' copies)
  // the next one, so the buffer a check measured is not written for two more stages.
  // A check whose error pass is deferred into the next iteration's single sweep (slab_stage_pipe_kernel<ERR>):
  // the sweep's barrier then also carries the blocks' (sum, count) slots, so the check costs no pass over the
  // block and no barrier of its own.  Its controller runs behind that barrier and snapshots the buffer the sweep
  // READ; other blocks may already be writing their next stage -- into the third buffer.  Decided from the
  // schedule alone, hence identically in every thread.
  PendingCheck pend;
  // Rank tables alternate between successive checks: with fused checks a block may already be pushing the NEXT
  // check's (sum, count) -- it rides on the sweep that follows the barrier -- while another block's controller
  // still reads this check's table behind the same barrier.  Two tables are enough: the push of check q + 2 is
  // issued behind the barrier that follows controller(q) in every stream.  (With one table and one stream per
  // block, controllers of different blocks saw different MAEs for the same check and stopped at different
  // iterations: tests/test_gpu_sharded_native.py::test_sharded_fuzz_equals_single_session.)
  long long n_check = 0;
  auto can_fuse = [&](const topolow_session* s) {
    return s->fuse_checks && s->dense_mae && s->precision == TOPOLOW_PRECISION_F32 && s->rows() % 2 == 0;
  };
  bool fusable = true;
  for (topolow_session* s : R.ss) fusable = fusable && can_fuse(s);
  // one-stage iterations as the sharded symmetric sweep: its ERR instance has no even-rows rule
  bool fusable_pair = R.pair_sharded;
  for (topolow_session* s : R.ss)
    fusable_pair = fusable_pair && s->fuse_checks && s->dense_mae && s->precision == TOPOLOW_PRECISION_F32;
  // a check's `parts` partials -> this block's slot of every rank table `tab` (inside the caller's check ProfScope)
  auto push_partials = [&](topolow_session* s, int parts, int tab) {
    hipLaunchKernelGGL(reduce_push_kernel, dim3(1), dim3(1024), 0, s->stream, s->part_sum.p, s->part_cnt.p, parts,
                       s->rsum_tab.p, s->rcnt_tab.p, s->n_ranks, tab + s->rank, s->state.p);
    HIP_TRY(hipGetLastError());
  };
  // behind the barrier: every block's controller on rank table `tab`, for check pc
  auto controllers = [&](const PendingCheck& pc, int tab) {
    for (int b : G.blocks) {
      topolow_session* s = R.ss[b];
      ProfScope prof(s, &s->prof_check);
      launch_controller(s, s->pos[pc.buf].p, pc.iter1, pc.k_after, s->rank_sum.p + tab, s->rank_cnt.p + tab, s->n_ranks);
    }
  };
  auto separate_check = [&](const PendingCheck& pc) -> bool {
    const int tab = (int)(n_check & 1) * P;
    ++n_check;
    for (int b : G.blocks) {
      topolow_session* s = R.ss[b];
      ProfScope prof(s, &s->prof_check);
      TL_DISPATCH_DIM(s->dim, launch_edge_error, s, s->pos[pc.buf].p, s->state.p);
      push_partials(s, error_parts(s), tab);
    }
    if (!exchange()) return false;
    controllers(pc, tab);
    return true;
  };
  for (; iter < lead->n_iter; ++iter) {
    if (seen != 0) break;
    if (R.warmup_iters > 0 && iter == R.warmup_iters) {   // measurement only: drain, meet, start the clock
      HIP_TRY(hipStreamSynchronize(G.stream));
      if (n_groups > 1 && !R.bar->wait()) return;
      if (r == 0) R.t_timed0 = now_s();
      if (n_groups > 1 && !R.bar->wait()) return;
    }
    if (r == 0 && R.interrupt_cb != nullptr && iter > 0 && iter % 50 == 0 && !R.interrupted)   // reference :364
      R.interrupted = R.interrupt_cb(R.interrupt_user) != 0;   // published at the next exchange
    // the session loop's plan: ONE block (the whole matrix) takes its symmetric forms, a block of several is row-owner
    const IterPlan plan = plan_iteration(lead, iter, k);
    const bool fuse_now = pend.active && plan.geo.n_stages == 1;
    if (pend.active && !fuse_now) { if (!separate_check(pend)) return; pend.active = false; }
    const int tab = (int)(n_check & 1) * P;   // the table of the check this sweep carries, if any
    if (fuse_now) ++n_check;
    if (R.pair_sharded && plan.geo.n_stages == 1) {
      // every session sweeps its segment of the tile list and folds its partials into the owners' inboxes; barrier;
      // the owners move their points and store them into every session's next buffer; barrier
      const int nxt = (cur + 1) % 3;
      for (int b : G.blocks) {
        topolow_session* s = R.ss[b];
        TL_DISPATCH_SYM(s->dim, sym_sharded_sweep, s, s->pos[cur].p, iter, k, fuse_now);
        if (fuse_now) { ProfScope prof(s, &s->prof_check); push_partials(s, s->sym.plan.n_units, tab); }
      }
      if (!exchange()) return;
      if (fuse_now) { controllers(pend, tab); pend.active = false; }
      for (int b : G.blocks) {
        topolow_session* s = R.ss[b];
        TL_DISPATCH_SYM(s->dim, sym_owner_apply, s, s->pos[cur].p, s->pos[nxt].p, s->row_begin, s->row_end, s->push_tab[nxt].p,
                        s->n_push, iter);
      }
      if (!exchange()) return;
      cur = nxt;
    } else
    for (int t = 0; t < plan.geo.n_stages; ++t) {
      const int nxt = (cur + 1) % 3;
      for (int b : G.blocks) {
        topolow_session* s = R.ss[b];
        const int parts = enqueue_stage(s, plan, t, s->pos[cur].p, s->pos[nxt].p, iter, k, s->push_tab[nxt].p, s->n_push,
                                        fuse_now);
        if (fuse_now) { ProfScope prof(s, &s->prof_check); push_partials(s, parts, tab); }
      }
      if (!exchange()) return;
      if (fuse_now) { controllers(pend, tab); pend.active = false; }
      cur = nxt;
    }
    k *= (1.0 - lead->cooling);   // reference :289
    if (check_after(lead, iter)) {
      const PendingCheck pc{true, iter + 1, k, cur};
      const bool fuse = (fusable || fusable_pair) && iter + 1 < lead->n_iter && iteration_stages(lead, iter + 1, k) == 1;
      if (fuse) pend = pc;
      else if (!separate_check(pc)) return;
    }
  }
  if (pend.active && !separate_check(pend)) return;   // the loop ended early
  for (int b : G.blocks) R.ss[b]->cur = cur;
  if (r == 0) { R.iters_enqueued = iter; R.exchanges = g; }
  HIP_TRY(hipStreamSynchronize(G.stream));
}

// Wires `count` loaded sessions (row blocks tiling [0, n) in order, same n / ndim / precision) into one
// another: peer access between their devices, push tables, rank tables.
void sharded_wire(std::vector<topolow_session*>& ss) {
  const int P = (int)ss.size();
  for (int a = 0; a < P; ++a)
    for (int b = 0; b < P; ++b) {
      if (ss[a]->device == ss[b]->device) continue;
      int can = 0;
      HIP_TRY(hipDeviceCanAccessPeer(&can, ss[a]->device, ss[b]->device));
      if (!can) throw HipError{TOPOLOW_ERR_UNSUPPORTED, "row-sharded run: the GPUs cannot access each other's memory"};
      HIP_TRY(hipSetDevice(ss[a]->device));
      const hipError_t e = hipDeviceEnablePeerAccess(ss[b]->device, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) HIP_TRY(e);
      (void)hipGetLastError();
    }
  for (int a = 0; a < P; ++a) {
    topolow_session* s = ss[a];
    HIP_TRY(hipSetDevice(s->device));
    s->n_ranks = P;
    s->rank = a;
    s->n_push = P - 1;
    for (int b2 = 0; b2 < 3; ++b2) {
      std::vector<void*> tab;
      for (int q = 0; q < P; ++q) if (q != a) tab.push_back((void*)ss[q]->pos[b2].p);
      s->push_tab[b2].alloc(tab.size());
      if (!tab.empty())
        HIP_TRY(hipMemcpy(s->push_tab[b2].p, tab.data(), tab.size() * sizeof(void*), hipMemcpyHostToDevice));
    }
    s->rank_sum.alloc(2 * P);   // two tables, alternating between successive checks (see sharded_worker)
    s->rank_cnt.alloc(2 * P);
    HIP_TRY(hipMemset(s->rank_sum.p, 0, sizeof(double) * 2 * P));
    HIP_TRY(hipMemset(s->rank_cnt.p, 0, sizeof(unsigned long long) * 2 * P));
  }
  for (int a = 0; a < P; ++a) {
    topolow_session* s = ss[a];
    HIP_TRY(hipSetDevice(s->device));
    std::vector<double*> ts;
    std::vector<unsigned long long*> tc;
    for (int q = 0; q < P; ++q) { ts.push_back(ss[q]->rank_sum.p); tc.push_back(ss[q]->rank_cnt.p); }
    s->rsum_tab.alloc(P);
    s->rcnt_tab.alloc(P);
    HIP_TRY(hipMemcpy(s->rsum_tab.p, ts.data(), P * sizeof(double*), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->rcnt_tab.p, tc.data(), P * sizeof(unsigned long long*), hipMemcpyHostToDevice));
  }
}

}  // namespace

// =========================================================================================
// C ABI
// =========================================================================================
extern "C" {

const char* topolow_relax_version(void) { return "topolow_relax 0.1 (gfx950)"; }

int64_t topolow_encoded_index(int32_t row_in_block, int32_t column, int32_t ld) {
  return (int64_t)enc_index(row_in_block, column, ld);
}

uint32_t topolow_encode_target(double dissimilarity, int32_t threshold_code) {
  return encode_target(dissimilarity, threshold_code);
}
double topolow_decode_target(uint32_t bits, int32_t* threshold_code) {
  int c = 0;
  const double v = decode_target(bits, &c);
  if (threshold_code) *threshold_code = c;
  return v;
}

int32_t topolow_slab_stages_for_k(double k, int32_t ndim) { return slab_stages_for_k(k, ndim); }
int32_t topolow_slab_stages_at(int32_t iter, double k, int32_t ndim) { return slab_stages_at(iter, k, ndim); }

int32_t topolow_slab_plan(int32_t n, int32_t slab_stages, uint64_t seed, int32_t iter,
                          int32_t* ranges_out, int32_t max_stages) {
  const SlabGeom g = slab_geom(n, slab_stages);
  if (!ranges_out) return g.n_stages;
  for (int slot = 0; slot < g.n_stages && slot < max_stages; ++slot) {
    const SlabRanges r = slab_ranges(g, seed, iter, slot);
    ranges_out[4 * slot + 0] = r.b0;
    ranges_out[4 * slot + 1] = r.e0;
    ranges_out[4 * slot + 2] = r.b1;
    ranges_out[4 * slot + 3] = r.e1;
  }
  return g.n_stages;
}

int topolow_controller_script(const double* mae_seq, const int32_t* iter_seq,
                              const double* k_seq, int32_t n_obs, double k0, int32_t window,
                              double eps, int32_t* stopped_at_obs, int32_t* snapshot_flags,
                              double* best_mae, double* best_k, int32_t* best_iter) {
  Controller c;
  c.init(k0, window, eps);
  *stopped_at_obs = -1;
  for (int o = 0; o < n_obs; ++o) {
    const int a = c.observe(mae_seq[o], iter_seq[o], k_seq[o]);
    if (snapshot_flags) snapshot_flags[o] = (a & 2) ? 1 : 0;
    if (a & 1) { *stopped_at_obs = o; break; }
  }
  *best_mae = c.best_mae;
  *best_k = c.best_k;
  *best_iter = c.best_iter;
  return TOPOLOW_OK;
}

// ---- session ---------------------------------------------------------------------------
int topolow_session_create(topolow_session** out, int32_t n, int32_t ndim, int32_t row_begin,
                           int32_t row_end, int32_t precision, int32_t device, char* errbuf,
                           size_t errlen) {
  if (!out) return TOPOLOW_ERR_BAD_ARGUMENT;
  *out = nullptr;
  if (n < 2) {
    set_err(errbuf, errlen, "Need at least 2 points for embedding");
    return TOPOLOW_ERR_TOO_FEW_POINTS;
  }
  if (ndim < 1 || ndim > kMaxDim) {
    set_err(errbuf, errlen, "ndim must be between 1 and %d in this build", kMaxDim);
    return TOPOLOW_ERR_UNSUPPORTED;
  }
  if (row_begin < 0 || row_end > n || row_begin >= row_end) {
    set_err(errbuf, errlen, "bad row block [%d,%d) for n=%d", row_begin, row_end, n);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  const bool exact = precision == TOPOLOW_PRECISION_F64_EXACT;
  if (exact && (row_begin != 0 || row_end != n)) {
    set_err(errbuf, errlen, "precision f64_exact: whole-problem sessions only (rows [%d,%d) of %d asked for): the row-sharded "
            "paths have no exact kernels", row_begin, row_end, n);
    return TOPOLOW_ERR_UNSUPPORTED;
  }
  if (exact && ndim > kMaxTunedDim) {
    set_err(errbuf, errlen, "precision f64_exact: ndim must be between 1 and %d (the plain stage kernel of wider embeddings "
            "reads the 4-byte targets only)", kMaxTunedDim);
    return TOPOLOW_ERR_UNSUPPORTED;
  }
  topolow_session* s = nullptr;
  const int rc = guarded(errbuf, errlen, [&] {
    const int dev = select_device(device);
    s = new topolow_session();
    s->device = dev;
    s->n = n;
    s->dim = kernel_dim(ndim);
    s->udim = ndim;
    s->row_begin = row_begin;
    s->row_end = row_end;
    s->ld = (n + kEncLdAlign - 1) & ~(kEncLdAlign - 1);
    s->precision = precision == TOPOLOW_PRECISION_F64 || exact ? TOPOLOW_PRECISION_F64 : TOPOLOW_PRECISION_F32;
    s->exact = exact;
    HIP_TRY(hipStreamCreateWithFlags(&s->own_stream, hipStreamNonBlocking));
    s->stream = s->own_stream;
    HIP_TRY(hipStreamCreateWithFlags(&s->check_stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&s->ev_iter_done, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&s->ev_check_done, hipEventDisableTiming));
    const char* serial = getenv("TOPOLOW_SERIAL_CHECKS");
    s->serial_checks = serial != nullptr && serial[0] == '1';
    const char* fuse = getenv("TOPOLOW_FUSE_CHECKS");
    s->fuse_checks = !(fuse != nullptr && fuse[0] == '0');
    const char* in_apply = getenv("TOPOLOW_CHECK_IN_APPLY");
    s->check_in_apply = !(in_apply != nullptr && in_apply[0] == '0');
    const char* symm = getenv("TOPOLOW_SYMMETRIC");
    s->sym.allowed = !(symm != nullptr && symm[0] == '0');   // TOPOLOW_SYMMETRIC=0: row-owner sweeps only
    s->sym.forced = symm != nullptr && symm[0] == '1';       // TOPOLOW_SYMMETRIC=1: also at an ndim that is off by default
    const char* symm_min = getenv("TOPOLOW_SYMMETRIC_MIN_N");   // tests lower the size gate to reach the sweep on small problems
    s->sym.min_n = symm_min != nullptr ? atoi(symm_min) : kSymMinPoints;
    const char* symm2 = getenv("TOPOLOW_SYMMETRIC_TWO_STAGE");
    s->sym.two_stage = !(symm2 != nullptr && symm2[0] == '0');
    const char* rr_min = getenv("TOPOLOW_SYMMETRIC_STAGE_MIN_TILES");
    if (rr_min != nullptr) s->sym.rr_min_tiles = std::max(0, atoi(rr_min));
    const char* sym_grid = getenv("TOPOLOW_SYMMETRIC_GRID");   // tests cap the grid: a small problem then gives every wave a long run
    s->sym.grid_cap = sym_grid != nullptr ? std::max(0, atoi(sym_grid)) : 0;
    const char* sym_prio = getenv("TOPOLOW_SYM_PRIO");
    s->sym.prio = !(sym_prio != nullptr && sym_prio[0] == '0');
    s->enc.alloc((size_t)((s->rows() + kEncRowAlign - 1) / kEncRowAlign * kEncRowAlign) * s->ld);
    if (s->exact) s->denc.alloc(s->enc.n);
    const size_t pos_bytes = (size_t)s->pos_rows() * s->dim * s->real_size();
    for (auto& b : s->pos) b.alloc(pos_bytes);
    for (auto& b : s->best) b.alloc(pos_bytes);
    s->state.alloc(1);
    HIP_TRY(hipHostMalloc((void**)&s->mailbox, sizeof(RunState), hipHostMallocMapped));
    std::memset(s->mailbox, 0, sizeof(RunState));
    HIP_TRY(hipHostGetDevicePointer((void**)&s->mailbox_dev, s->mailbox, 0));
  });
  if (rc != TOPOLOW_OK) { delete s; return rc; }
  *out = s;
  return TOPOLOW_OK;
}

void topolow_session_destroy(topolow_session* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  if (s->check_stream) (void)hipStreamSynchronize(s->check_stream);
#ifdef TOPOLOW_TUNING
  g_stamps.dump();
#endif
  delete s;
}

int topolow_session_set_relabel(topolow_session* s, uint64_t seed, char* errbuf, size_t errlen) {
  if (!s) return TOPOLOW_ERR_BAD_ARGUMENT;
  if (s->gplus.p || s->part_sum.p) {
    set_err(errbuf, errlen, "the relabelling must be chosen before targets, edges or positions are loaded");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    s->perm.clear();
    s->inv.clear();
    if (seed == 0) return;   // identity
    const int n = s->n;
    s->perm.resize(n);
    s->inv.resize(n);
    for (int q = 0; q < n; ++q) s->perm[q] = q;
    for (int q = n - 1; q > 0; --q) {   // Fisher-Yates on the schedule's counter-based stream
      const uint32_t r = rnd_below(rnd64(seed, 0x7e1abe1ull, (uint64_t)q), (uint32_t)(q + 1));
      std::swap(s->perm[q], s->perm[r]);
    }
    for (int q = 0; q < n; ++q) s->inv[s->perm[q]] = q;
    s->d_perm.alloc(n);
    s->d_inv.alloc(n);
    HIP_TRY(hipMemcpy(s->d_perm.p, s->perm.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->d_inv.p, s->inv.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
  });
}

int topolow_session_labels(const topolow_session* s, int32_t* session_to_caller) {
  if (!s || !session_to_caller) return TOPOLOW_ERR_BAD_ARGUMENT;
  for (int q = 0; q < s->n; ++q) session_to_caller[q] = s->perm.empty() ? q : s->perm[q];
  return TOPOLOW_OK;
}

int topolow_session_load_dense(topolow_session* s, const double* D, const int32_t* T,
                               const int32_t* degrees, char* errbuf, size_t errlen) {
  if (!s || !D || !T || !degrees) return TOPOLOW_ERR_BAD_ARGUMENT;
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    const size_t nn = (size_t)s->n * s->n;
    DevBuf<double> dD;
    DevBuf<int> dT;
    dD.alloc(nn);
    dT.alloc(nn);
    HIP_TRY(hipMemcpy(dD.p, D, nn * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dT.p, T, nn * 4, hipMemcpyHostToDevice));
    dim3 grid(s->rows(), (s->ld + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(encode_dense_kernel, grid, dim3(kThreads), 0, s->stream, dD.p, dT.p, s->n,
                       s->row_begin, s->row_end, s->ld, s->enc.p, s->perm.empty() ? nullptr : s->d_perm.p,
                       s->exact ? s->denc.p : (float*)nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->stream));
    compute_row_flags(s);
    upload_degrees(s, degrees);
  });
}

int topolow_session_load_coo(topolow_session* s, const int32_t* edge_i, const int32_t* edge_j,
                             const double* edge_dist, const int32_t* edge_thresh,
                             int64_t n_edges, const int32_t* degrees, char* errbuf,
                             size_t errlen) {
  if (!s || !degrees || n_edges < 0) return TOPOLOW_ERR_BAD_ARGUMENT;
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    dim3 grid(s->rows(), (s->ld + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(fill_unmeasured_kernel, grid, dim3(kThreads), 0, s->stream, s->n,
                       s->row_begin, s->row_end, s->ld, s->enc.p, s->exact ? s->denc.p : (float*)nullptr);
    HIP_TRY(hipGetLastError());
    const int64_t chunk = 1 << 24;
    DevBuf<int> di, dj, dc;
    DevBuf<double> dd;
    const size_t cap = (size_t)std::min<int64_t>(chunk, std::max<int64_t>(n_edges, 1));
    di.alloc(cap); dj.alloc(cap); dc.alloc(cap); dd.alloc(cap);
    for (int64_t off = 0; off < n_edges; off += chunk) {
      const int64_t m = std::min<int64_t>(chunk, n_edges - off);
      HIP_TRY(hipMemcpyAsync(di.p, edge_i + off, m * 4, hipMemcpyHostToDevice, s->stream));
      HIP_TRY(hipMemcpyAsync(dj.p, edge_j + off, m * 4, hipMemcpyHostToDevice, s->stream));
      HIP_TRY(hipMemcpyAsync(dd.p, edge_dist + off, m * 8, hipMemcpyHostToDevice, s->stream));
      HIP_TRY(hipMemcpyAsync(dc.p, edge_thresh + off, m * 4, hipMemcpyHostToDevice, s->stream));
      hipLaunchKernelGGL(scatter_edges_kernel, dim3((unsigned)((m + kThreads - 1) / kThreads)),
                         dim3(kThreads), 0, s->stream, di.p, dj.p, dd.p, dc.p, (long long)m, s->n,
                         s->row_begin, s->row_end, s->ld, s->enc.p, s->inv.empty() ? nullptr : s->d_inv.p,
                         s->exact ? s->denc.p : (float*)nullptr);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipStreamSynchronize(s->stream));
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    compute_row_flags(s);
    upload_degrees(s, degrees);
  });
}

void* topolow_session_encoded_ptr(topolow_session* s) { return s ? (void*)s->enc.p : nullptr; }
int32_t topolow_session_encoded_ld(const topolow_session* s) { return s ? s->ld : 0; }

int topolow_session_commit_encoded(topolow_session* s, const int32_t* degrees, char* errbuf,
                                   size_t errlen) {
  if (!s || !degrees) return TOPOLOW_ERR_BAD_ARGUMENT;
  if (!s->perm.empty()) {
    set_err(errbuf, errlen, "a block filled by the caller is in the caller's labels: not with a relabelled session");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (s->exact) {
    set_err(errbuf, errlen, "precision f64_exact: a block of 4-byte words filled by the caller carries no deltas; load the "
            "targets with topolow_session_load_dense or topolow_session_load_coo");
    return TOPOLOW_ERR_UNSUPPORTED;
  }
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());  // the caller filled the block on another stream
    compute_row_flags(s);
    upload_degrees(s, degrees);
  });
}

int topolow_session_set_edges(topolow_session* s, const int32_t* edge_i, const int32_t* edge_j,
                              const double* edge_dist, const int32_t* edge_thresh,
                              int64_t n_edges, char* errbuf, size_t errlen) {
  if (!s || n_edges < 0) return TOPOLOW_ERR_BAD_ARGUMENT;
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    edges_begin(s, n_edges);
    const size_t m = (size_t)n_edges;
    // Can the MAE be reduced from the encoded block instead of gathering the edge list?  Only if
    // the list is exactly the set of measured cells the dense pass would visit -- checked with an
    // order-independent fingerprint BEFORE anything is uploaded: when it holds (it does for
    // everything the R driver builds), the list itself never travels to the device.
    const int* inv = s->inv.empty() ? nullptr : s->inv.data();
    if (s->gplus.p && !edge_mae_forced()) {
      std::atomic<bool> owned{true};
      std::atomic<unsigned long long> fp_total{0};
      host_parallel(m, kEdgeGrain, [&](size_t lo_e, size_t hi_e) {
        unsigned long long fp = 0;
        for (size_t e = lo_e; e < hi_e; ++e) {
          int a = edge_i[e], b = edge_j[e];
          if (a < 0 || b < 0 || a >= s->n || b >= s->n || a == b) { owned.store(false); return; }
          if (inv) { a = inv[a]; b = inv[b]; }
          const int lo = a < b ? a : b, hi = a < b ? b : a;
          int owner = lo;
          if (s->dense_parity && (((lo + hi) & 1) != 0)) owner = hi;
          if (owner < s->row_begin || owner >= s->row_end) { owned.store(false); return; }
          const uint32_t w = encode_target(edge_dist[e], edge_thresh[e]);
          if (w == kInfWord) { owned.store(false); return; }
          fp += cell_fingerprint(lo, hi, w);
        }
        fp_total.fetch_add(fp);
      });
      if (owned.load()) {
        unsigned long long h[2];
        block_fingerprint(s, h);
        edges_decide(s, (h[0] == fp_total.load()) && (h[1] == (unsigned long long)m));
      }
    }
    if (edges_placeholders(s)) return;
    // edge-list MAE (parity sessions keep the exact f64 targets): upload the list in session labels
    s->ei.alloc(m); s->ej.alloc(m); s->ec.alloc(m);
    std::vector<int8_t> codes(m);
    std::vector<int> li, lj;
    if (inv) { li.resize(m); lj.resize(m); }
    host_parallel(m, kEdgeGrain, [&](size_t lo_e, size_t hi_e) {
      for (size_t e = lo_e; e < hi_e; ++e) {
        const int c = edge_thresh[e];
        codes[e] = (int8_t)(c == 0 ? 0 : (c == 1 ? 1 : (c == -1 ? -1 : 2)));  // others never count
        if (inv) {
          const int a = edge_i[e], b = edge_j[e];
          li[e] = (a >= 0 && a < s->n) ? inv[a] : a;
          lj[e] = (b >= 0 && b < s->n) ? inv[b] : b;
        }
      }
    });
    if (m) {
      HIP_TRY(hipMemcpy(s->ei.p, inv ? li.data() : edge_i, m * 4, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(s->ej.p, inv ? lj.data() : edge_j, m * 4, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(s->ec.p, codes.data(), m, hipMemcpyHostToDevice));
    }
    if (s->precision == TOPOLOW_PRECISION_F64) {
      s->et.alloc(m * 8);
      if (m) HIP_TRY(hipMemcpy(s->et.p, edge_dist, m * 8, hipMemcpyHostToDevice));
    } else {
      std::vector<float> t(m);
      host_parallel(m, kEdgeGrain, [&](size_t lo_e, size_t hi_e) {
        for (size_t e = lo_e; e < hi_e; ++e) t[e] = (float)edge_dist[e];
      });
      s->et.alloc(m * 4);
      if (m) HIP_TRY(hipMemcpy(s->et.p, t.data(), m * 4, hipMemcpyHostToDevice));
    }
  });
}

int topolow_session_set_positions(topolow_session* s, const double* positions, char* errbuf,
                                  size_t errlen) {
  if (!s || !positions) return TOPOLOW_ERR_BAD_ARGUMENT;
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    s->cur = 0;
    upload_positions(s, positions, s->pos[0].p);
    // the other buffers need the same padding rows
    for (int b = 1; b < 3; ++b)
      HIP_TRY(hipMemcpyAsync(s->pos[b].p, s->pos[0].p, (size_t)s->pos_rows() * s->dim * s->real_size(),
                             hipMemcpyDeviceToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->held = -1;
    s->pcheck.active = false;
  });
}

int topolow_session_get_positions(topolow_session* s, double* positions, char* errbuf,
                                  size_t errlen) {
  if (!s || !positions) return TOPOLOW_ERR_BAD_ARGUMENT;
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    download_positions(s, s->pos[s->cur].p, positions);
  });
}

int topolow_session_begin(topolow_session* s, int32_t n_iter, double k0, double cooling_rate,
                          double c_repulsion, double relative_epsilon,
                          int32_t convergence_window, int32_t convergence_check_freq,
                          uint64_t seed, int32_t slab_stages, char* errbuf, size_t errlen) {
  if (!s) return TOPOLOW_ERR_BAD_ARGUMENT;
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    if (!s->gplus.p) throw HipError{TOPOLOW_ERR_BAD_ARGUMENT, "session has no targets loaded"};
    if (!s->part_sum.p) throw HipError{TOPOLOW_ERR_BAD_ARGUMENT, "session has no edge list"};
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipStreamSynchronize(s->check_stream));
    for (hipEvent_t e : s->pending) s->event_pool.push_back(e);
    s->pending.clear();
    s->n_iter = n_iter;
    s->k0 = k0;
    s->cooling = cooling_rate;
    s->c_rep = c_repulsion;
    s->eps = relative_epsilon;
    s->window = convergence_window;
    s->check_freq = convergence_check_freq < 1 ? 10 : convergence_check_freq;  // reference :181
    {
      const int need = n_iter / s->check_freq + 2;
      if (need > s->trace_cap) {
        if (s->trace) { (void)hipHostFree(s->trace); s->trace = nullptr; s->trace_cap = 0; }
        HIP_TRY(hipHostMalloc((void**)&s->trace, sizeof(double) * 3 * (size_t)need, hipHostMallocMapped));
        HIP_TRY(hipHostGetDevicePointer((void**)&s->trace_dev, s->trace, 0));
        s->trace_cap = need;
      }
    }
    s->seed = seed;
    s->fixed_stages = slab_stages;
    s->iters_enqueued = 0;
    s->k_host = k0;
    s->host_seen_stop = false;
    s->held = -1;
    s->pcheck.active = false;
    s->checks_launched = 0;
    s->checks_in_apply = 0;
    s->sym.rec_iter = -1;
    s->began = true;
    s->in_run = true;
    RunState st;
    std::memset(&st, 0, sizeof st);
    st.ctl.init(k0, convergence_window, relative_epsilon);
    st.k_base = k0;
    st.cooling = cooling_rate;
    st.n_iter = n_iter;
    st.first_nonfinite = 0x7fffffff;
    *s->mailbox = st;
    HIP_TRY(hipMemcpyAsync(s->state.p, &st, sizeof st, hipMemcpyHostToDevice, s->stream));
    // best snapshot starts as the initial positions (reference :171): in buffer 0, which both entries of the cleared
    // state name
    HIP_TRY(hipMemcpyAsync(s->best[0].p, s->pos[s->cur].p,
                           (size_t)s->pos_rows() * s->dim * s->real_size(), hipMemcpyDeviceToDevice,
                           s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
  });
}

int topolow_session_enqueue(topolow_session* s, int32_t max_iters, int32_t* enqueued,
                            char* errbuf, size_t errlen) {
  if (!s || !s->began) return TOPOLOW_ERR_BAD_ARGUMENT;
  if (enqueued) *enqueued = 0;
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    int done = 0;
    while (done < max_iters && s->iters_enqueued < s->n_iter && !s->host_seen_stop) {
      const int iter = s->iters_enqueued;
      if (s->schedule == TOPOLOW_SCHEDULE_GS) {
        TL_DISPATCH_DIM(s->dim, launch_tilegs_iteration, s, s->pos[s->cur].p, iter, s->k_host);
      } else {
        const IterPlan plan = plan_iteration(s, iter, s->k_host);
        const bool fuse_now = s->pcheck.active && check_fusable(s, plan.geo.n_stages);
        if (s->pcheck.active && !fuse_now) flush_pending_check(s);
        // the check rides on this iteration's one sweep and its controller step goes out in the sweep's apply launch
        const bool in_apply = fuse_now && s->pcheck.in_apply && plan.form == SymForm::kSweep;
        for (int t = 0; t < plan.geo.n_stages; ++t) {
          int out = 0;   // a buffer that is neither the input nor the one a running check reads
          while (out == s->cur || out == s->held) ++out;
          enqueue_stage(s, plan, t, s->pos[s->cur].p, s->pos[out].p, iter, s->k_host, nullptr, 0, fuse_now,
                        in_apply ? &s->pcheck : nullptr);
          s->cur = out;
        }
        if (in_apply) check_went_in_apply(s, s->pcheck);
        else if (fuse_now) launch_check(s, s->pcheck, /*error_pass=*/false);
      }
      s->iters_enqueued = iter + 1;
      s->k_host *= (1.0 - s->cooling);  // reference :289
      ++done;
      if (check_after(s, iter)) {
        PendingCheck pc{true, iter + 1, s->k_host, s->cur};
        pc.beside = s->schedule == TOPOLOW_SCHEDULE_SLAB && s->stream == s->own_stream &&
                    !s->profiling && !s->serial_checks;
        // The run's last check has no next iteration to run beside.  With the fused checks in the applies the check
        // stream has by then been idle for the whole one-stage phase, and its queue would have to be woken for this one
        // check while everything waits for it: the check goes to the main stream.  (TOPOLOW_CHECK_IN_APPLY=0 keeps it
        // where it was.)
        if (s->check_in_apply && iter + 1 == s->n_iter) pc.beside = false;
        // The check reads this iteration's positions while the next iteration's stages run.  Its
        // verdict (stop / snapshot) is the same as in the serial order: the buffer it reads is
        // not written until the next check has waited for it; stage kernels that start after a
        // stop are no-ops and those already running write buffers nobody returns.
        if (s->held >= 0) HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_check_done, 0));
        // one stage next iteration: its kernel reduces this check's MAE (the positions it reads ARE this
        // check's positions) and the separate pass over the block is dropped
        // (fp32: the row-owner ERR instance or the symmetric sweep's, when the MAE comes from the block; f64: the
        //  symmetric sweep's, exact through its delta tiles)
        const bool fuse = s->fuse_checks && s->schedule == TOPOLOW_SCHEDULE_SLAB && iter + 1 < s->n_iter &&
                          (s->dense_mae || s->precision == TOPOLOW_PRECISION_F64) &&
                          check_fusable(s, iteration_stages(s, iter + 1, s->k_host));
        // ... and when that kernel is the symmetric sweep, the controller step rides in the sweep's apply launch on the
        // main stream: the check's positions are that iteration's input, read-only until the apply has finished, so
        // no buffer is held and nothing goes to the check stream.  (Should the check be flushed instead -- the caller
        // asks for results first -- it runs as a separate pass on the main stream.)
        if (pc.beside && fuse && s->check_in_apply && sym_form(s, 1) == SymForm::kSweep) {
          pc.in_apply = true;
          pc.beside = false;
        }
        s->held = pc.beside ? s->cur : -1;
        if (fuse) s->pcheck = pc;
        else launch_check(s, pc, /*error_pass=*/true);
      }
      // the slab kernels flag non-finite results themselves; the in-place schedule is inspected at
      // the reference's cadence (:359-361), after that iteration's check
      if (s->schedule == TOPOLOW_SCHEDULE_GS && (iter + 1) % 10 == 0)
        launch_tilegs_finite(s, s->pos[s->cur].p, iter + 1);
    }
    if (enqueued) *enqueued = done;
  });
}

int topolow_session_wait(topolow_session* s, char* errbuf, size_t errlen) {
  if (!s) return TOPOLOW_ERR_BAD_ARGUMENT;
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipStreamSynchronize(s->check_stream));
  });
}

int topolow_session_sync(topolow_session* s, int32_t* iterations_run, int32_t* stopped,
                         double* last_mae, char* errbuf, size_t errlen) {
  if (!s) return TOPOLOW_ERR_BAD_ARGUMENT;
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    flush_pending_check(s);
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipStreamSynchronize(s->check_stream));
    poll_checks(s, 0);
    RunState st;
    HIP_TRY(hipMemcpy(&st, s->state.p, sizeof st, hipMemcpyDeviceToHost));
    if (st.stopped) s->host_seen_stop = true;
    if (iterations_run) *iterations_run = st.stopped ? st.iter_base : s->iters_enqueued;
    if (stopped) *stopped = st.stopped;
    if (last_mae) *last_mae = st.last_mae;
  });
}

int topolow_session_finish(topolow_session* s, double* positions_out, int32_t* converged,
                           int32_t* iterations, double* final_mae, double* final_k,
                           char* errbuf, size_t errlen) {
  if (!s) return TOPOLOW_ERR_BAD_ARGUMENT;
  int rc_nonfinite = TOPOLOW_OK;
  s->in_run = false;
  const int rc = guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    flush_pending_check(s);
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipStreamSynchronize(s->check_stream));
    poll_checks(s, 0);
    RunState st;
    HIP_TRY(hipMemcpy(&st, s->state.p, sizeof st, hipMemcpyDeviceToHost));
    const int t = nonfinite_report(st.first_nonfinite, st.stopped ? st.iter_base : s->iters_enqueued, st.stopped);
    if (t != 0) {
      set_err(errbuf, errlen, "Numerical instability at iteration %d. Reduce k0 or c_repulsion.", t);
      rc_nonfinite = TOPOLOW_ERR_NONFINITE;
      return;
    }
    if (positions_out) download_positions(s, s->best[topolow_session::best_index(st)].p, positions_out);
    if (converged) *converged = st.converged;
    if (iterations) *iterations = st.ctl.best_iter;
    if (final_mae) *final_mae = st.ctl.best_mae;
    if (final_k) *final_k = st.ctl.best_k;
  });
  return rc != TOPOLOW_OK ? rc : rc_nonfinite;
}

int topolow_session_check_trace(topolow_session* s, double* out, int32_t max_checks, int32_t* n_checks) {
  if (!s || (!out && max_checks > 0) || !n_checks) return TOPOLOW_ERR_BAD_ARGUMENT;
  (void)hipSetDevice(s->device);
  try { flush_pending_check(s); } catch (const HipError&) { return TOPOLOW_ERR_HIP; }
  (void)hipStreamSynchronize(s->stream);
  (void)hipStreamSynchronize(s->check_stream);
  const int have = std::min(s->mailbox ? s->mailbox->n_checks : 0, s->trace_cap);
  *n_checks = have;
  const int take = std::min(have, (int)max_checks);
  if (take > 0) std::memcpy(out, s->trace, sizeof(double) * 3 * (size_t)take);
  return TOPOLOW_OK;
}

int topolow_session_set_profiling(topolow_session* s, int32_t enable) {
  if (!s) return TOPOLOW_ERR_BAD_ARGUMENT;
  s->profiling = enable != 0;
  return TOPOLOW_OK;
}

int topolow_session_profile(topolow_session* s, double* stage_ms, int64_t* stage_launches,
                            double* check_ms, int64_t* checks, char* errbuf, size_t errlen) {
  if (!s) return TOPOLOW_ERR_BAD_ARGUMENT;
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    flush_pending_check(s);
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipStreamSynchronize(s->check_stream));
    auto drain = [](std::vector<std::pair<hipEvent_t, hipEvent_t>>& v, double* ms, int64_t* cnt) {
      double total = 0.0;
      for (auto& pr : v) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, pr.first, pr.second) == hipSuccess) total += t;
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
      }
      if (ms) *ms = total;
      if (cnt) *cnt = (int64_t)v.size();
      v.clear();
    };
    // stage launches: the plain ones plus those that also reduced a check's MAE (reported apart by
    // topolow_session_profile_fused, which must be asked first)
    double ms_a = 0.0, ms_b = 0.0;
    int64_t n_a = 0, n_b = 0;
    drain(s->prof_stage, &ms_a, &n_a);
    drain(s->prof_stage_err, &ms_b, &n_b);
    if (stage_ms) *stage_ms = ms_a + ms_b;
    if (stage_launches) *stage_launches = n_a + n_b;
    drain(s->prof_check, check_ms, checks);
  });
}

int topolow_session_profile_fused(topolow_session* s, double* fused_ms, int64_t* fused_launches, char* errbuf,
                                  size_t errlen) {
  if (!s) return TOPOLOW_ERR_BAD_ARGUMENT;
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    flush_pending_check(s);
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipStreamSynchronize(s->check_stream));
    double total = 0.0;
    for (auto& pr : s->prof_stage_err) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, pr.first, pr.second) == hipSuccess) total += t;
    }
    if (fused_ms) *fused_ms = total;
    if (fused_launches) *fused_launches = (int64_t)s->prof_stage_err.size();
  });
}

int topolow_session_profile_symmetric(topolow_session* s, double* plain_ms, int64_t* plain_iterations, double* fused_ms,
                                      int64_t* fused_iterations, char* errbuf, size_t errlen) {
  if (!s) return TOPOLOW_ERR_BAD_ARGUMENT;
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    flush_pending_check(s);
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipStreamSynchronize(s->check_stream));
    auto drain = [](std::vector<std::pair<hipEvent_t, hipEvent_t>>& v, double* ms, int64_t* cnt) {
      double total = 0.0;
      for (auto& pr : v) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, pr.first, pr.second) == hipSuccess) total += t;
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
      }
      if (ms) *ms = total;
      if (cnt) *cnt = (int64_t)v.size();
      v.clear();
    };
    drain(s->prof_sym, plain_ms, plain_iterations);
    drain(s->prof_sym_err, fused_ms, fused_iterations);
  });
}

int topolow_session_set_stream(topolow_session* s, void* hip_stream, int32_t external) {
  if (!s) return TOPOLOW_ERR_BAD_ARGUMENT;
  (void)hipSetDevice(s->device);
  (void)hipStreamSynchronize(s->stream);
  (void)hipStreamSynchronize(s->check_stream);
  s->stream = external ? (hipStream_t)hip_stream : s->own_stream;
  return TOPOLOW_OK;
}

void* topolow_session_stream(topolow_session* s) { return s ? (void*)s->stream : nullptr; }

int topolow_session_set_schedule(topolow_session* s, int32_t schedule) {
  if (!s || (schedule != TOPOLOW_SCHEDULE_SLAB && schedule != TOPOLOW_SCHEDULE_GS))
    return TOPOLOW_ERR_BAD_ARGUMENT;
  if (s->row_begin != 0 || s->row_end != s->n) return TOPOLOW_ERR_UNSUPPORTED;  // tile GS: whole problem
  s->schedule = schedule;
  return TOPOLOW_OK;
}

int64_t topolow_tilegs_pair_order(int32_t n, uint64_t seed, int32_t iter, int32_t* pairs_out) {
  return tilegs_pair_order(n, seed, iter, pairs_out);
}

int32_t topolow_session_position_rows(const topolow_session* s) { return s ? s->pos_rows() : 0; }
int32_t topolow_session_position_dim(const topolow_session* s) { return s ? s->dim : 0; }

int32_t topolow_session_uses_dense_mae(const topolow_session* s) {
  return s && s->dense_mae ? 1 : 0;
}

int64_t topolow_session_stage_launches(const topolow_session* s) {
  return s ? s->stage_launches : 0;
}

int64_t topolow_session_checks_in_apply(const topolow_session* s) {
  return s ? s->checks_in_apply : 0;
}

int64_t topolow_session_bytes_per_iteration(const topolow_session* s) {
  if (!s) return 0;
  return 4ll * s->rows() * s->n + 8ll * s->n * s->udim + 4ll * s->n;
}

int topolow_session_stage(topolow_session* s, const void* d_pos_in, void* d_pos_out,
                          int32_t iter, int32_t stage, int32_t n_stages, double k,
                          char* errbuf, size_t errlen) {
  if (!s || !d_pos_in || !d_pos_out) return TOPOLOW_ERR_BAD_ARGUMENT;
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    const SlabGeom g = slab_geom(s->n, n_stages);
    if (stage < 0 || stage >= g.n_stages)
      throw HipError{TOPOLOW_ERR_BAD_ARGUMENT, "stage index out of range"};
    const SlabRanges rg = slab_ranges(g, s->seed, iter, stage);
    // inside a run (topolow_session_begin) the launch honours the run's stop flag and reports
    // non-finite results through its state, like the session's own loop
    TL_DISPATCH_DIM(s->dim, launch_stage, s, d_pos_in, d_pos_out, s->began ? s->state.p : (RunState*)nullptr, rg,
                    iter + 1, k);
    s->iters_enqueued = std::max(s->iters_enqueued, iter + 1);
  });
}

int32_t topolow_session_can_fuse_checks(const topolow_session* s) {
  return s && s->fuse_checks && s->dense_mae && s->precision == TOPOLOW_PRECISION_F32 && s->rows() % 2 == 0 ? 1 : 0;
}

int topolow_session_stage_fused(topolow_session* s, const void* d_pos_in, void* d_pos_out, int32_t iter,
                                double k, double* d_out2, char* errbuf, size_t errlen) {
  if (!s || !d_pos_in || !d_pos_out || !d_out2 || !s->began) return TOPOLOW_ERR_BAD_ARGUMENT;
  if (!topolow_session_can_fuse_checks(s)) {
    set_err(errbuf, errlen, "this session cannot fuse checks (needs the fp32 block-based MAE and an even row count)");
    return TOPOLOW_ERR_UNSUPPORTED;
  }
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    const SlabGeom g = slab_geom(s->n, 1);
    const SlabRanges rg = slab_ranges(g, s->seed, iter, 0);
    TL_DISPATCH_DIM(s->dim, launch_stage, s, d_pos_in, d_pos_out, s->state.p, rg, iter + 1, k, nullptr, 0, true);
    const int stage_blocks = (s->rows() + CfgProd::ROWS - 1) / CfgProd::ROWS;
    hipLaunchKernelGGL(reduce_total_kernel, dim3(1), dim3(1024), 0, s->stream, s->part_sum.p, s->part_cnt.p,
                       stage_blocks, d_out2, s->state.p);
    HIP_TRY(hipGetLastError());
    s->iters_enqueued = std::max(s->iters_enqueued, iter + 1);
  });
}

int topolow_session_check_partial(topolow_session* s, const void* d_pos, double* d_out2, char* errbuf,
                                  size_t errlen) {
  if (!s || !d_pos || !d_out2 || !s->part_sum.p || !s->began) return TOPOLOW_ERR_BAD_ARGUMENT;
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    TL_DISPATCH_DIM(s->dim, launch_edge_error, s, d_pos, s->state.p);
    hipLaunchKernelGGL(reduce_total_kernel, dim3(1), dim3(1024), 0, s->stream, s->part_sum.p, s->part_cnt.p,
                       error_parts(s), d_out2, s->state.p);
    HIP_TRY(hipGetLastError());
  });
}

int topolow_session_controller_step(topolow_session* s, const double* d_total2, const void* d_pos,
                                    int32_t iter1, double k_after, char* errbuf, size_t errlen) {
  if (!s || !d_total2 || !d_pos || !s->began) return TOPOLOW_ERR_BAD_ARGUMENT;
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    launch_controller(s, d_pos, iter1, k_after, nullptr, nullptr, 0, d_total2);
    s->iters_enqueued = std::max(s->iters_enqueued, (int)iter1);
  });
}

int32_t topolow_symm_stage_bounds(int32_t n, int32_t stages, int32_t* first_label) {
  if (n < 2 || !first_label || !(stages == 2 || stages == 4 || stages == 8)) return 0;
  const int npad = (n + kSymRows - 1) & ~(kSymRows - 1), TR = npad / kSymRows;
  if (TR < 2 * stages) return 0;
  for (int q = 0; q <= stages; ++q) first_label[q] = std::min(n, sym_rr_bound(TR, stages, q) * kSymRows);
  return 1;
}
int32_t topolow_symm_stage_order(uint64_t seed, int32_t iter, int32_t stages, int32_t* order) {
  if (!order || !(stages == 2 || stages == 4 || stages == 8)) return 0;
  int perm[8];
  sym_rr_order(seed, iter, stages, perm);
  for (int q = 0; q < stages; ++q) order[q] = perm[q];
  return 1;
}

int32_t topolow_symm_stage_rows(int32_t n, int32_t stages, int32_t stage, int32_t* rows_out) {
  if (n < 2 || !(stages == 2 || stages == 4 || stages == 8) || stage < 0 || stage >= stages) return -1;
  const int npad = (n + kSymRows - 1) & ~(kSymRows - 1), TR = npad / kSymRows;
  if (TR < 2 * stages) return -1;
  for (int R = 0; rows_out && R < TR; ++R) {
    int j0 = 0, j1 = 0, rp0 = 0, rp1 = 0;
    sym_rr_row(TR, stages, stage, R, j0, j1);
    sym_rr_above(TR, stages, stage, R, rp0, rp1);
    rows_out[4 * R] = j0;
    rows_out[4 * R + 1] = j1;
    rows_out[4 * R + 2] = rp0;
    rows_out[4 * R + 3] = rp1;
  }
  return TR;
}

int32_t topolow_symm_plan(int32_t n, int32_t n_waves, int32_t stages, int32_t stage, int32_t segment, int32_t n_segments,
                          int32_t* units_out, int32_t max_units, int32_t* wave_first_out) {
  if (n < 2 || n_waves < 1 || (units_out && max_units < 0)) return -1;
  const int npad = (n + kSymRows - 1) & ~(kSymRows - 1), TR = npad / kSymRows;
  SymPlan plan;
  if (stages != 0) {            // one stage of a multi-stage iteration (sym_rr_available)
    if (!sym_rr_stages_ok(stages) || stage < 0 || stage >= stages || TR < 2 * stages || n_segments > 1) return -1;
    plan = sym_rr_plan(npad, n_waves, stages, stage);
  } else if (n_segments >= 2) {   // a segment of the sharded sweep (sym_sharded_build, sym_segment_build)
    if (segment < 0 || segment >= n_segments) return -1;
    const SymSegment g = sym_segment(n, segment, n_segments);
    plan = relax_symm_plan(npad, n_waves, g.t0, g.t1);
  } else {                        // the whole triangle (sym_prepare)
    plan = relax_symm_plan(npad, n_waves, 0, -1);
  }
  const int n_units = (int)plan.units.size();
  for (int u = 0; units_out && u < std::min(n_units, (int)max_units); ++u) {
    units_out[4 * u] = plan.units[u].tile_row;
    units_out[4 * u + 1] = plan.units[u].j0;
    units_out[4 * u + 2] = plan.units[u].j1;
    units_out[4 * u + 3] = plan.units[u].tile0;
  }
  for (int w = 0; wave_first_out && w <= n_waves; ++w) wave_first_out[w] = plan.wave_first[w];
  return n_units;
}

int32_t topolow_session_symm_grid(const topolow_session* s) {
  return s && s->sym.holds != SymHolds::kNothing ? s->sym.grid : 0;
}

int32_t topolow_symm_segment_rows(int32_t n, int32_t segment, int32_t n_segments, int32_t* row_first,
                                  int32_t* row_end) {
  if (n < 2 || n_segments < 1 || segment < 0 || segment >= n_segments) return 0;
  const SymSegment g = sym_segment(n, segment, n_segments);
  if (g.total < 8ll * n_segments || g.r_first < 0) return 0;
  if (row_first) *row_first = g.r_first * kSymRows;
  if (row_end) *row_end = (int32_t)std::min<long long>(n, (long long)(g.r_last + 1) * kSymRows);
  return 1;
}

int32_t topolow_session_symm_segment_eligible(const topolow_session* s, int32_t n_segments) {
  return s && sym_shape_ok(s) && s->precision == TOPOLOW_PRECISION_F32 && s->gplus.p != nullptr &&
                 topolow_symm_segment_rows(s->n, 0, n_segments, nullptr, nullptr)
             ? 1 : 0;
}

float* topolow_session_degree_terms(topolow_session* s) { return s ? s->gplus.p : nullptr; }
int32_t topolow_session_has_thresholds(const topolow_session* s) { return s && s->gplus.p && s->any_threshold ? 1 : 0; }
float* topolow_session_symm_moves(topolow_session* s) {
  return s && s->sym.holds == SymHolds::kCallerSegment ? s->sym.inbox.p : nullptr;
}

int topolow_session_symm_segment_build(topolow_session* s, int32_t segment, int32_t n_segments, const void* d_rows,
                                       int32_t row_first, int32_t n_rows, int32_t any_threshold, char* errbuf,
                                       size_t errlen) {
  if (!s || !d_rows || n_segments < 1 || segment < 0 || segment >= n_segments || n_rows < 0 || row_first < 0 ||
      row_first + n_rows > s->n)
    return TOPOLOW_ERR_BAD_ARGUMENT;
  if (!topolow_session_symm_segment_eligible(s, n_segments)) {
    set_err(errbuf, errlen, "this session cannot take the symmetric sweep (fp32 slab schedule, ndim 2..10, at least %d "
                            "points, targets loaded)", s->sym.min_n);
    return TOPOLOW_ERR_UNSUPPORTED;
  }
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    try {
      TL_DISPATCH_SYM(s->dim, sym_segment_build, s, segment, n_segments, (const uint32_t*)d_rows, row_first, n_rows,
                      any_threshold != 0);
    } catch (const HipError&) {      // e.g. the device cannot hold the extra buffers: the session keeps its row-owner sweep
      s->sym.release();
      throw;
    }
  });
}

// The segment sweep's ERR instance reduces the block's measured cells (no even-rows rule, unlike the row-owner one): it may
// stand for a check only where the separate pass reduces the same cells.
int32_t topolow_session_can_fuse_segment_checks(const topolow_session* s) {
  return s && s->fuse_checks && s->dense_mae && s->precision == TOPOLOW_PRECISION_F32 ? 1 : 0;
}

int topolow_session_symm_segment_sweep(topolow_session* s, const void* d_pos_in, int32_t iter, double k,
                                       double* d_out2, char* errbuf, size_t errlen) {
  if (!s || !d_pos_in || !s->began) return TOPOLOW_ERR_BAD_ARGUMENT;
  if (s->sym.holds != SymHolds::kCallerSegment) {
    set_err(errbuf, errlen, "no segment built (topolow_session_symm_segment_build)");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (d_out2 != nullptr && !topolow_session_can_fuse_segment_checks(s)) {
    set_err(errbuf, errlen, "this session cannot reduce a check in its segment sweep (needs fp32, fused checks enabled and "
                            "the MAE reduced from the block); use topolow_session_check_partial");
    return TOPOLOW_ERR_UNSUPPORTED;
  }
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    TL_DISPATCH_SYM(s->dim, sym_sharded_sweep, s, d_pos_in, iter, k, d_out2 != nullptr);
    if (d_out2 != nullptr) {
      hipLaunchKernelGGL(reduce_total_kernel, dim3(1), dim3(1024), 0, s->stream, s->part_sum.p, s->part_cnt.p,
                         s->sym.tiles > 0 ? s->sym.plan.n_units : 0, d_out2, s->state.p);
      HIP_TRY(hipGetLastError());
    }
    s->iters_enqueued = std::max(s->iters_enqueued, iter + 1);
  });
}

int topolow_session_symm_segment_apply(topolow_session* s, const void* d_pos_in, void* d_pos_out, int32_t iter,
                                       char* errbuf, size_t errlen) {
  if (!s || !d_pos_in || !d_pos_out || !s->began || s->sym.holds != SymHolds::kCallerSegment)
    return TOPOLOW_ERR_BAD_ARGUMENT;
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    TL_DISPATCH_SYM(s->dim, sym_owner_apply, s, d_pos_in, d_pos_out, 0, s->n, nullptr, 0, iter);
  });
}

int topolow_session_first_nonfinite(topolow_session* s, int32_t* iteration) {
  if (!s || !iteration) return TOPOLOW_ERR_BAD_ARGUMENT;
  (void)hipSetDevice(s->device);
  (void)hipStreamSynchronize(s->stream);
  RunState st;
  if (hipMemcpy(&st, s->state.p, sizeof st, hipMemcpyDeviceToHost) != hipSuccess) return TOPOLOW_ERR_HIP;
  *iteration = st.first_nonfinite == 0x7fffffff ? 0 : st.first_nonfinite;
  return TOPOLOW_OK;
}

int topolow_session_edge_error(topolow_session* s, const void* d_pos, double* sum,
                               int64_t* count, char* errbuf, size_t errlen) {
  if (!s || !d_pos || !s->part_sum.p) return TOPOLOW_ERR_BAD_ARGUMENT;
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    TL_DISPATCH_DIM(s->dim, launch_edge_error, s, d_pos, (const RunState*)nullptr);
    const int np = error_parts(s);
    std::vector<double> ps(np);
    std::vector<unsigned long long> pc(np);
    HIP_TRY(hipMemcpyAsync(ps.data(), s->part_sum.p, np * 8, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(pc.data(), s->part_cnt.p, np * 8, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    double ts = 0.0;
    unsigned long long tc = 0;
    for (int p = 0; p < np; ++p) { ts += ps[p]; tc += pc[p]; }
    if (sum) *sum = ts;
    if (count) *count = (int64_t)tc;
  });
}

// ---- a cross-validation fold on a resident session (relax_cv.h) ---------------------------
int topolow_session_hold_out(topolow_session* s, const int32_t* pair_i, const int32_t* pair_j, int64_t n_pairs,
                             const int32_t* degrees, char* errbuf, size_t errlen) {
  if (!s || !degrees || n_pairs < 0 || (n_pairs > 0 && (!pair_i || !pair_j))) return TOPOLOW_ERR_BAD_ARGUMENT;
  const int rc0 = cv_check_hold_out(s, errbuf, errlen);
  if (rc0 != TOPOLOW_OK) return rc0;
  for (int64_t q = 0; q < n_pairs; ++q)
    if (pair_i[q] < 0 || pair_i[q] >= s->n || pair_j[q] < 0 || pair_j[q] >= s->n) {
      set_err(errbuf, errlen, "held-out pair %lld out of range", (long long)q);
      return TOPOLOW_ERR_BAD_ARGUMENT;
    }
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    // the host front: session labels, lo < hi, every pair once (i == j: nothing to hold out)
    std::vector<long long> key;
    key.reserve((size_t)n_pairs);
    for (int64_t q = 0; q < n_pairs; ++q) {
      int a = pair_i[q], b = pair_j[q];
      if (a == b) continue;
      if (!s->inv.empty()) { a = s->inv[a]; b = s->inv[b]; }
      key.push_back((long long)std::min(a, b) * s->n + std::max(a, b));
    }
    std::sort(key.begin(), key.end());
    key.erase(std::unique(key.begin(), key.end()), key.end());
    const long long np = (long long)key.size();
    std::vector<int> lo((size_t)np), hi((size_t)np);
    for (long long q = 0; q < np; ++q) { lo[(size_t)q] = (int)(key[(size_t)q] / s->n); hi[(size_t)q] = (int)(key[(size_t)q] % s->n); }
    cv_hold_out_pairs(s, np, degrees, [&](int* d_lo, int* d_hi) {
      HIP_TRY(hipMemcpyAsync(d_lo, lo.data(), (size_t)np * 4, hipMemcpyHostToDevice, s->stream));
      HIP_TRY(hipMemcpyAsync(d_hi, hi.data(), (size_t)np * 4, hipMemcpyHostToDevice, s->stream));
    });
  });
}

int topolow_session_restore_held_out(topolow_session* s, const int32_t* degrees, char* errbuf, size_t errlen) {
  if (!s || !degrees) return TOPOLOW_ERR_BAD_ARGUMENT;
  const int rc0 = cv_check_session(s, errbuf, errlen);
  if (rc0 != TOPOLOW_OK) return rc0;
  if (!s->cv.active) {
    set_err(errbuf, errlen, "nothing is held out");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    auto& h = s->cv;
    const long long np = h.n_pairs;
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipStreamSynchronize(s->check_stream));
    if (np > 0)
      hipLaunchKernelGGL(cv_unmask_kernel, dim3(pair_grid(np)), dim3(kThreads), 0, s->stream, h.lo.p, h.hi.p, np, s->enc.p,
                         s->ld, h.words.p);
    HIP_TRY(hipGetLastError());
    if (h.list_compacted) {
      swap_buf(s->ei, h.ei); swap_buf(s->ej, h.ej); swap_buf(s->et, h.et); swap_buf(s->ec, h.ec);
      s->n_edges = h.full_edges;
      s->n_parts = h.full_parts;
      h.list_compacted = false;
    }
    // (a copy built meanwhile holds the fold's block: rebuilt from the full one on first use)
    const bool put_back = s->sym.holds == SymHolds::kTriangle && h.tiles_patched && h.generation == s->sym.generation;
    if (put_back) {
      if (np > 0)
        hipLaunchKernelGGL(cv_tiles_kernel, dim3(pair_grid(np)), dim3(kThreads), 0, s->stream, h.lo.p, h.hi.p, np,
                           s->sym.tenc.p, s->sym.delta_ready ? s->sym.tdelta.p : (float*)nullptr, s->sym.npad / kSymCols,
                           (const uint32_t*)h.words.p, h.deltas.p);
      HIP_TRY(hipGetLastError());
    }
    h.tiles_patched = false;
    cv_refresh_flags(s, put_back);
    upload_degrees(s, degrees);
    HIP_TRY(hipStreamSynchronize(s->stream));
    h.active = false;
  });
}

int topolow_session_score_pairs(topolow_session* s, const int32_t* pair_i, const int32_t* pair_j, const double* truth,
                                int64_t n_pairs, double* sum_abs, int64_t* count, char* errbuf, size_t errlen) {
  if (!s || n_pairs < 0 || (n_pairs > 0 && (!pair_i || !pair_j || !truth))) return TOPOLOW_ERR_BAD_ARGUMENT;
  if (!s->began) {
    set_err(errbuf, errlen, "no run to score: the pairs are scored on the positions topolow_session_finish restores");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  for (int64_t q = 0; q < n_pairs; ++q)
    if (pair_i[q] < 0 || pair_i[q] >= s->n || pair_j[q] < 0 || pair_j[q] >= s->n) {
      set_err(errbuf, errlen, "scored pair %lld out of range", (long long)q);
      return TOPOLOW_ERR_BAD_ARGUMENT;
    }
  if (sum_abs) *sum_abs = 0.0;
  if (count) *count = 0;
  if (n_pairs == 0) return TOPOLOW_OK;
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    auto& h = s->cv;
    const size_t np = (size_t)n_pairs;
    grow_buf(h.sc_i, np); grow_buf(h.sc_j, np); grow_buf(h.sc_t, np);
    std::vector<int> si, sj;
    const int32_t* pi = pair_i;
    const int32_t* pj = pair_j;
    if (!s->inv.empty()) {
      si.resize(np); sj.resize(np);
      for (size_t q = 0; q < np; ++q) { si[q] = s->inv[pair_i[q]]; sj[q] = s->inv[pair_j[q]]; }
      pi = si.data(); pj = sj.data();
    }
    HIP_TRY(hipMemcpyAsync(h.sc_i.p, pi, np * 4, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(h.sc_j.p, pj, np * 4, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(h.sc_t.p, truth, np * 8, hipMemcpyHostToDevice, s->stream));
    cv_score_device(s, h.sc_i.p, h.sc_j.p, h.sc_t.p, (long long)n_pairs, sum_abs, count);
  });
}

// ---- ONE embedding row-sharded over several sessions (one process, one host thread per block) ----
int topolow_sessions_run_sharded(topolow_session** sessions, int32_t count, const double* initial_positions,
                                 int32_t n_iter, double k0, double cooling_rate, double c_repulsion,
                                 double relative_epsilon, int32_t convergence_window,
                                 int32_t convergence_check_freq, uint64_t seed, int32_t slab_stages,
                                 int32_t (*interrupt_cb)(void*), void* interrupt_user, int32_t profile,
                                 double* positions_out, int32_t* converged, int32_t* iterations,
                                 double* final_mae, double* final_k, topolow_shard_stats* stats, char* errbuf,
                                 size_t errlen) {
  if (!sessions || count < 1 || !initial_positions) return TOPOLOW_ERR_BAD_ARGUMENT;
  const int warmup_iters = stats != nullptr ? stats->warmup_iterations : 0;   // in: see the header
  int rc_extra = TOPOLOW_OK;
  const int rc = guarded(errbuf, errlen, [&] {
    ShardedRun R;
    R.ss.assign(sessions, sessions + count);
    const int n = R.ss[0]->n;
    int expect = 0;
    for (topolow_session* s : R.ss) {
      if (!s || s->n != n || s->dim != R.ss[0]->dim || s->precision != R.ss[0]->precision ||
          s->row_begin != expect || s->schedule != TOPOLOW_SCHEDULE_SLAB)
        throw HipError{TOPOLOW_ERR_BAD_ARGUMENT,
                       "row-sharded run: the sessions must be slab-schedule row blocks that tile [0, n) in order"};
      expect = s->row_end;
    }
    if (expect != n) throw HipError{TOPOLOW_ERR_BAD_ARGUMENT, "row-sharded run: the row blocks do not cover all n rows"};
    sharded_wire(R.ss);
    if (sym_sharded_eligible(R.ss)) {
      // one-stage iterations as the symmetric sweep sharded over the sessions; a device that cannot hold the extra
      // buffers (half a row block again per session) keeps the row-owner sweep
      try {
        sym_sharded_prepare(R.ss);
        R.pair_sharded = true;
      } catch (const HipError&) {
        (void)hipGetLastError();
        for (topolow_session* s : R.ss) s->sym.release();
        R.pair_sharded = false;
      }
    }
    // groups: blocks that share a GPU share one stream and one host thread
    const char* per_block = getenv("TOPOLOW_SHARD_THREAD_PER_BLOCK");
    const bool thread_per_block = per_block != nullptr && per_block[0] == '1';
    for (int b = 0; b < count; ++b) {
      int gidx = -1;
      if (!thread_per_block)
        for (size_t q = 0; q < R.groups.size(); ++q) if (R.groups[q].device == R.ss[b]->device) gidx = (int)q;
      if (gidx < 0) {
        R.groups.emplace_back();
        gidx = (int)R.groups.size() - 1;
        R.groups[gidx].device = R.ss[b]->device;
        R.groups[gidx].stream = R.ss[b]->own_stream;
      }
      R.groups[gidx].blocks.push_back(b);
    }
    const int n_groups = (int)R.groups.size();
    for (int b = 0; b < count; ++b) {
      topolow_session* s = R.ss[b];
      int rcb = topolow_session_set_stream(s, nullptr, 0);
      if (rcb == TOPOLOW_OK) rcb = topolow_session_set_positions(s, initial_positions, errbuf, errlen);
      if (rcb == TOPOLOW_OK)
        rcb = topolow_session_begin(s, n_iter, k0, cooling_rate, c_repulsion, relative_epsilon, convergence_window,
                                    convergence_check_freq, seed, slab_stages, errbuf, errlen);
      if (rcb != TOPOLOW_OK) throw HipError{rcb, errbuf ? errbuf : "session setup failed"};
      s->profiling = false;
    }
    for (const ShardedGroup& G : R.groups)
      for (int b : G.blocks) R.ss[b]->stream = G.stream;   // (idle: set_positions / begin have synchronised)
    R.interrupt_cb = interrupt_cb;
    R.interrupt_user = interrupt_user;
    R.flag[0].store(0);
    R.flag[1].store(0);
    ShardedAbortableBarrier bar(n_groups);
    R.bar = &bar;
    R.ev.resize(n_groups);
    for (auto& e : R.ev) e = {nullptr, nullptr};
    auto cleanup = [&] {
      for (int q = 0; q < n_groups; ++q) {
        (void)hipSetDevice(R.groups[q].device);
        (void)hipStreamSynchronize(R.groups[q].stream);
        for (hipEvent_t e : R.ev[q]) if (e) (void)hipEventDestroy(e);
      }
      for (topolow_session* s : R.ss) s->stream = s->own_stream;
    };
    try {
      for (int q = 0; q < n_groups; ++q) {
        HIP_TRY(hipSetDevice(R.groups[q].device));
        for (int e = 0; e < 2; ++e) HIP_TRY(hipEventCreateWithFlags(&R.ev[q][e], hipEventDisableTiming));
      }
      R.warmup_iters = warmup_iters;
      if (profile)   // the kernels of the first GPU's blocks are bracketed by timing events
        for (int b : R.groups[0].blocks) R.ss[b]->profiling = true;
      const long long launches0 = R.ss[0]->stage_launches;
      const double t0 = now_s();
      auto body = [&](int r) {
        try {
          sharded_worker(R, r);
        } catch (const HipError& e) {
          std::lock_guard<std::mutex> lock(R.err_mu);
          if (R.first_error.code == TOPOLOW_OK) R.first_error = e;
          bar.fail();
        } catch (const std::exception& e) {
          std::lock_guard<std::mutex> lock(R.err_mu);
          if (R.first_error.code == TOPOLOW_OK) R.first_error = HipError{TOPOLOW_ERR_HIP, e.what()};
          bar.fail();
        }
      };
      std::vector<std::thread> pool;
      for (int r = 1; r < n_groups; ++r) pool.emplace_back(body, r);
      body(0);   // the calling thread is the first GPU's thread (the interrupt callback runs here)
      for (auto& t : pool) t.join();
      if (R.first_error.code != TOPOLOW_OK) throw R.first_error;
      const double wall = now_s() - t0;
      // result: every block holds the same controller state and the same best snapshot
      topolow_session* s0 = R.ss[0];
      HIP_TRY(hipSetDevice(s0->device));
      RunState st;
      HIP_TRY(hipMemcpy(&st, s0->state.p, sizeof st, hipMemcpyDeviceToHost));
      int first_bad = 0x7fffffff;
      for (topolow_session* s : R.ss) {
        HIP_TRY(hipSetDevice(s->device));
        RunState sb;
        HIP_TRY(hipMemcpy(&sb, s->state.p, sizeof sb, hipMemcpyDeviceToHost));
        first_bad = std::min(first_bad, sb.first_nonfinite);
      }
      HIP_TRY(hipSetDevice(s0->device));
      const int ran = st.stopped ? st.iter_base : R.iters_enqueued;
      if (stats) {
        std::memset(stats, 0, sizeof *stats);
        stats->blocks = count;
        stats->groups = n_groups;
        stats->iterations_run = ran;
        stats->n_checks = st.n_checks;
        stats->loop_seconds = wall;
        stats->stage_launches = s0->stage_launches - launches0;
        stats->exchanges = R.exchanges;
        stats->warmup_iterations = warmup_iters;
        stats->symmetric_segments = R.pair_sharded ? count : 0;
        stats->timed_seconds = (warmup_iters > 0 && R.t_timed0 > 0.0) ? (t0 + wall) - R.t_timed0 : wall;
        if (profile) {
          for (int b : R.groups[0].blocks) {
            double sm = 0, cm = 0;
            int64_t sl = 0, cl = 0;
            (void)topolow_session_profile(R.ss[b], &sm, &sl, &cm, &cl, nullptr, 0);
            double ya = 0, yb = 0;    // a single block's one-stage iterations may have run as symmetric sweeps
            int64_t na = 0, nb = 0;
            (void)topolow_session_profile_symmetric(R.ss[b], &ya, &na, &yb, &nb, nullptr, 0);
            stats->stage_kernel_seconds += (sm + ya + yb) * 1e-3;
            stats->check_kernel_seconds += cm * 1e-3;
          }
        }
      }
      for (topolow_session* s : R.ss) s->profiling = false;
      if (R.interrupted) {
        set_err(errbuf, errlen, "interrupted by the caller");
        rc_extra = TOPOLOW_ERR_INTERRUPTED;
      } else if (const int t = nonfinite_report(first_bad, ran, st.stopped)) {
        set_err(errbuf, errlen, "Numerical instability at iteration %d. Reduce k0 or c_repulsion.", t);
        rc_extra = TOPOLOW_ERR_NONFINITE;
      } else {
        if (positions_out) download_positions(s0, s0->best[topolow_session::best_index(st)].p, positions_out);
        if (converged) *converged = st.converged;
        if (iterations) *iterations = st.ctl.best_iter;
        if (final_mae) *final_mae = st.ctl.best_mae;
        if (final_k) *final_k = st.ctl.best_k;
      }
    } catch (...) {
      cleanup();
      throw;
    }
    cleanup();
  });
  return rc != TOPOLOW_OK ? rc : rc_extra;
}

int32_t topolow_shard_rows(int32_t n, int32_t blocks, int32_t block, int32_t* row_begin, int32_t* row_end) {
  if (n < 1 || blocks < 1) return 0;
  int per = (n + blocks - 1) / blocks;
  per = (per + 7) & ~7;                       // whole workgroups of 8 rows
  const int used = (n + per - 1) / per;       // blocks that hold at least one row
  if (block >= 0 && block < used) {
    if (row_begin) *row_begin = block * per;
    if (row_end) *row_end = std::min(n, (block + 1) * per);
  } else {
    if (row_begin) *row_begin = n;
    if (row_end) *row_end = n;
  }
  return used;
}

// ---- the resident embedding: a session, the whole relaxation and the post-metrics from a prepared handle ----
// The matrix went up once (topolow_layout_prep_create); these entries read what the handle keeps on the device.
int topolow_session_load_prepared(topolow_session* s, topolow_layout_prep* p, char* errbuf, size_t errlen) {
  if (!s || !p) {
    set_err(errbuf, errlen, "null argument");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (const int rcu = prep_check_usable(p, errbuf, errlen)) return rcu;
  if (p->n != s->n) {
    set_err(errbuf, errlen, "the handle holds %d points, the session %d", p->n, s->n);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (s->row_begin != 0 || s->row_end != s->n) {
    set_err(errbuf, errlen, "whole-problem sessions only (rows [%d,%d) of %d): a row block loads from the caller's arrays",
            s->row_begin, s->row_end, s->n);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (p->device != s->device) {
    set_err(errbuf, errlen, "the handle lives on device %d, the session on device %d", p->device, s->device);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    const double t0 = now_s();
    const int n = s->n;
    // -- the encoded block (and an f64_exact session's deltas) from the resident dense fill, through the session's
    //    relabelling.  The fill is symmetric bit for bit, so the kernel's column-major reading of the upper triangle
    //    holds for either layout of the handle; enc_index covers a -DTOPOLOW_ENC_TILED=1 build.
    dim3 grid(s->rows(), (s->ld + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(encode_dense_kernel, grid, dim3(kThreads), 0, s->stream, p->dense.p, p->tdense.p, n,
                       s->row_begin, s->row_end, s->ld, s->enc.p, s->perm.empty() ? nullptr : s->d_perm.p,
                       s->exact ? s->denc.p : (float*)nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->stream));
    compute_row_flags(s);
    // -- the degree terms: upload_degrees' arithmetic, gathered on the device
    if (s->gplus.p == nullptr || s->gplus.n != (size_t)n) s->gplus.alloc(n);
    hipLaunchKernelGGL(prep_degree_terms_kernel, dim3((n + kPrepThreads - 1) / kPrepThreads), dim3(kPrepThreads), 0,
                       s->stream, p->ddeg.p, n, s->perm.empty() ? nullptr : s->d_perm.p, s->gplus.p);
    HIP_TRY(hipGetLastError());
    // -- the convergence edge list
    const int64_t E = p->n_edges;
    edges_begin(s, E);
    // Is the list the block's measured cells (topolow_session_set_edges' question)?  Both come from ONE dense fill:
    // the list holds exactly the cells i < j of the fill that are not +Inf (prep_edge_count_kernel, which counted E,
    // and prep_edge_write_kernel apply the same test to the same cells), each pair once, both ends in range, and the
    // block holds encode_target of the same cells under the same relabelling.  So every measured cell of the block's
    // upper triangle is an edge with the same word, and the two sets differ only where an edge's target encodes to
    // the unmeasured word (NaN never reaches the fill; a -Inf cell would) -- then the block has fewer measured cells
    // than the list has edges, which is what set_edges refuses a list for as well.  Hence: list_is_block iff the
    // block's count equals E.  The count comes from the device (upper_fingerprint_kernel); no host pass reads an edge.
    if (!edge_mae_forced()) {
      unsigned long long h[2];
      block_fingerprint(s, h);
      edges_decide(s, h[1] == (unsigned long long)E);
    }
    if (!edges_placeholders(s)) {
      // the list is gathered by the check: in session labels, from the handle's compacted list, device to device
      prep_compact_edges(p, s->stream);
      const size_t m = (size_t)E;
      const bool f64 = s->precision == TOPOLOW_PRECISION_F64;
      s->ei.alloc(m); s->ej.alloc(m); s->ec.alloc(m);
      s->et.alloc(m * (f64 ? 8 : 4));
      if (m) {
        hipLaunchKernelGGL(prep_session_edges_kernel, dim3((unsigned)((m + kPrepThreads - 1) / kPrepThreads)),
                           dim3(kPrepThreads), 0, s->stream, p->edge_i.p, p->edge_j.p, p->edge_dist.p, p->edge_thresh.p,
                           (long long)E, s->inv.empty() ? nullptr : s->d_inv.p, s->ei.p, s->ej.p, s->ec.p,
                           f64 ? reinterpret_cast<double*>(s->et.p) : nullptr,
                           f64 ? nullptr : reinterpret_cast<float*>(s->et.p));
        HIP_TRY(hipGetLastError());
      }
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    p->resident_seconds[0] = now_s() - t0;
  });
}

}  // extern "C"