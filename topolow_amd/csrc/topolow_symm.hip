// topolow_amd/csrc/topolow_symm.hip -- the symmetric sweep's host side (relax_symm.h, relax_symm64.h,
// relax_symm_wide.h): which sessions take it, the build of the tile-major copy and the plans, the launches of one
// iteration, multi-stage iterations, the sweep sharded over the row-block sessions of a run and over caller-driven
// sessions, and the topolow_symm_* / topolow_session_symm_* C ABI of include/topolow_relax.h.  The session's loop and
// the row-sharded engine (topolow_relax.hip) reach it through the functions declared in topolow_session.h.

#include "topolow_session.h"
#include "relax_symm.h"
#include "relax_symm64.h"
#include "relax_symm_wide.h"

namespace {

// ---- symmetric sweep (relax_symm.h, relax_symm_wide.h, relax_symm64.h) -------------------------------------
// Which sessions take it: the whole matrix on one GPU (no row block, nothing to push), slab schedule, ndim 2..10 in
// fp32 and 2..6 in f64, at least kSymMinPoints points.  Up to ndim 6 the register-tiled kernel keeps eight rows'
// coordinates, constants and sums in VGPRs (20 x ndim + 16 of them); fp32 sessions of ndim 7..10 run
// symm_sweep_wide_kernel, which keeps the rows in LDS and only their sums in VGPRs (relax_symm_wide.h); f64 sessions of
// ndim 7..10 stay on the row-owner kernel.  Row-sharded runs shard it over their sessions (sym_sharded_*, below).
// Everything else stays on the row-owner stage kernel.

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

// The shape every form of the sweep needs; the eligibility of each form adds its own terms.
// The precision term is part of the shape: the largest ndim differs (fp32: 10, f64: 6).
bool sym_shape_ok(const topolow_session* s) {
  const int max_dim = s->precision == TOPOLOW_PRECISION_F32 ? kSymMaxDimF32
                      : s->precision == TOPOLOW_PRECISION_F64 ? kSymMaxDimF64 : 0;
  return s->sym.allowed && s->schedule == TOPOLOW_SCHEDULE_SLAB && s->dim >= 2 && s->dim <= max_dim &&
         (sym_dim_default(s->dim) || s->sym.forced) && s->dim == s->udim && s->n >= s->sym.min_n;
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

}  // namespace

// ---- what the session's loop, the row-sharded engine and the hold-out call (declared in topolow_session.h) ----

bool sym_eligible(const topolow_session* s) {
  return sym_shape_ok(s) && s->row_begin == 0 && s->row_end == s->n && s->n_push == 0;
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

// f64: whether a sweep may reduce a check's MAE.  Plain f64 sessions: the delta tiles exist (they are made from the edge
// list when it is the block's measured cells).  Exact sessions always have delta tiles, from the matrix; the fused
// check's sum and count run over the block's measured cells, so the list must still be exactly those.
bool sym_fused_ok(const topolow_session* s) {
  if (!s->sym.delta_ready) return false;
  return !s->exact || (s->list_is_block && s->n_edges > 0 && s->sym.holds == SymHolds::kTriangle);
}

// How an iteration of n_stages stages runs on a whole-matrix session: one symmetric sweep (one stage), S sweeps over the
// tiles of one stage each (S = 2, 4, 8), or the row-owner stage kernel.  Builds the sweep on first use.
SymForm sym_form(topolow_session* s, int n_stages) {
  if (n_stages == 1) return sym_eligible(s) && sym_available(s) ? SymForm::kSweep : SymForm::kRowOwner;
  return s->sym.two_stage && sym_rr_stages_ok(n_stages) && sym_eligible(s) && sym_available(s) &&
                 sym_rr_available(s, n_stages)
             ? SymForm::kStages
             : SymForm::kRowOwner;
}

// Whether the row-block sessions of one run shard the sweep of their one-stage iterations (the engine: topolow_relax.hip).
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

// Every session's segment, built where it is not held already, and the inboxes wired to one another.
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

// sym_iteration, sym_sharded_sweep and sym_owner_apply at the session's ndim: the dispatch stays on this side.
void sym_run_iteration(topolow_session* s, const void* pin, void* pout, int iter, double k, bool err, int S, int st, bool last,
                       const PendingCheck* in_apply) {
  TL_DISPATCH_SYM(s->dim, sym_iteration, s, pin, pout, iter, k, err, S, st, last, in_apply);
}

void sym_run_sharded_sweep(topolow_session* s, const void* pin, int iter, double k, bool err) {
  TL_DISPATCH_SYM(s->dim, sym_sharded_sweep, s, pin, iter, k, err);
}

void sym_run_owner_apply(topolow_session* s, const void* pin, void* pout, int row_begin, int row_end, const void* push,
                         int n_push, int iter) {
  TL_DISPATCH_SYM(s->dim, sym_owner_apply, s, pin, pout, row_begin, row_end, push, n_push, iter);
}

extern "C" {

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
    sym_run_sharded_sweep(s, d_pos_in, iter, k, d_out2 != nullptr);
    if (d_out2 != nullptr) reduce_total(s, s->sym.tiles > 0 ? s->sym.plan.n_units : 0, d_out2);   // (the kernel is topolow_relax.hip's)
    s->iters_enqueued = std::max(s->iters_enqueued, iter + 1);
  });
}

int topolow_session_symm_segment_apply(topolow_session* s, const void* d_pos_in, void* d_pos_out, int32_t iter,
                                       char* errbuf, size_t errlen) {
  if (!s || !d_pos_in || !d_pos_out || !s->began || s->sym.holds != SymHolds::kCallerSegment)
    return TOPOLOW_ERR_BAD_ARGUMENT;
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(s->device));
    sym_run_owner_apply(s, d_pos_in, d_pos_out, 0, s->n, nullptr, 0, iter);
  });
}

}  // extern "C"
