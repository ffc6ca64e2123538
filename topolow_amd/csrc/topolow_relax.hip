// topolow_amd/csrc/topolow_relax.hip -- the session of libtopolow_relax.so and its loop: a session's buffers and loads,
// the launch helpers of the stage and check kernels (relax_kernels.h, relax_exact.h), the iteration plan, the
// row-sharded engine and the topolow_session_* C ABI of include/topolow_relax.h.  The symmetric sweep's host side is
// topolow_symm.hip, tile Gauss-Seidel topolow_tilegs.hip, hold-out and scoring topolow_cv.hip; what crosses between
// the four is declared in topolow_session.h.  The drivers that run whole embeddings on sessions are
// topolow_drivers.hip, the one-workgroup Gauss-Seidel entries topolow_gs.hip, the post-metrics topolow_post.hip, the
// prepared handle topolow_prep.hip with topolow_prep_graph.hip, topolow_spectrum.hip and topolow_prep_fold.hip.
//
// There is no CPU fallback in this library: without a HIP device every entry point that
// computes returns TOPOLOW_ERR_NO_DEVICE.

#include "topolow_session.h"
#include "topolow_prep.h"
#include "relax_kernels.h"
#include "relax_exact.h"

// =========================================================================================
// Session (slab path)
// =========================================================================================
namespace {

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

void compute_row_flags(topolow_session* s) {
  s->cv.active = false;   // a new block: whatever was held out of the old one is gone with it
  s->block_gen += 1;
  s->sym.invalidate();    // a new block invalidates whatever the sweep holds: rebuilt on first use
  s->rowflags.alloc(s->rows());
  scan_row_flags(s);
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

// ---- the iteration plan: how many stages, in which form (topolow_symm.hip: sym_form), and their launches ----
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
    sym_run_iteration(s, pin, pout, iter, k, err, 0, 0, true, in_apply);
  } else {   // S symmetric sweeps over the tiles of one stage each, in random order
    const int S = p.geo.n_stages;
    sym_run_iteration(s, pin, pout, iter, k, err, S, p.order[t], t == S - 1, nullptr);
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

}  // namespace

// ---- what the session's other sources call as well (declared in topolow_session.h) ----

// Workgroups (= partial sums) of the edge-list MAE pass over n_edges edges.
int edge_error_blocks(long long n_edges) {
  long long blocks = (n_edges + (long long)kThreads * 8 - 1) / ((long long)kThreads * 8);
  if (blocks < 1) blocks = 1;
  if (blocks > 2048) blocks = 2048;
  return (int)blocks;
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

void upload_degrees(topolow_session* s, const int32_t* degrees) {
  std::vector<float> g(s->n);
  for (int i = 0; i < s->n; ++i) g[i] = (float)degrees[s->perm.empty() ? i : s->perm[i]] + 1.0f;  // reference :137-140
  if (s->gplus.p == nullptr || s->gplus.n != (size_t)s->n) s->gplus.alloc(s->n);
  HIP_TRY(hipMemcpy(s->gplus.p, g.data(), (size_t)s->n * 4, hipMemcpyHostToDevice));
}

void reduce_total(topolow_session* s, int n_parts, double* d_out2) {
  hipLaunchKernelGGL(reduce_total_kernel, dim3(1), dim3(1024), 0, s->stream, s->part_sum.p, s->part_cnt.p, n_parts, d_out2,
                     s->state.p);
  HIP_TRY(hipGetLastError());
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
        sym_run_sharded_sweep(s, s->pos[cur].p, iter, k, fuse_now);
        if (fuse_now) { ProfScope prof(s, &s->prof_check); push_partials(s, s->sym.plan.n_units, tab); }
      }
      if (!exchange()) return;
      if (fuse_now) { controllers(pend, tab); pend.active = false; }
      for (int b : G.blocks) {
        topolow_session* s = R.ss[b];
        sym_run_owner_apply(s, s->pos[cur].p, s->pos[nxt].p, s->row_begin, s->row_end, s->push_tab[nxt].p, s->n_push, iter);
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
        tilegs_run_iteration(s, s->pos[s->cur].p, iter, s->k_host);
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
    reduce_total(s, stage_blocks, d_out2);
    s->iters_enqueued = std::max(s->iters_enqueued, iter + 1);
  });
}

int topolow_session_check_partial(topolow_session* s, const void* d_pos, double* d_out2, char* errbuf,
                                  size_t errlen) {
  if (!s || !d_pos || !d_out2 || !s->part_sum.p || !s->began) return TOPOLOW_ERR_BAD_ARGUMENT;
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    TL_DISPATCH_DIM(s->dim, launch_edge_error, s, d_pos, s->state.p);
    reduce_total(s, error_parts(s), d_out2);
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

float* topolow_session_degree_terms(topolow_session* s) { return s ? s->gplus.p : nullptr; }
int32_t topolow_session_has_thresholds(const topolow_session* s) { return s && s->gplus.p && s->any_threshold ? 1 : 0; }

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