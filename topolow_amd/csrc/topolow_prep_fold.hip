// topolow_amd/csrc/topolow_prep_fold.hip -- what reads a prepared handle through its fold mask: the cross-validation
// folds and the CV sweep (relax_prep_fold.h), and the fit report with its order statistics (relax_fit.h).  One source,
// because both mark their picks with fold_mark_kernel.  The masked sums come down through PrepSums<FoldTotals>::fetch
// of topolow_prep.hip.

#include "topolow_prep.h"
#include "topolow_drivers.h"
#include "relax_fold.h"
#include "relax_prep_fold.h"
#include "relax_fit.h"

// ---- cross-validation folds from a prepared handle (relax_prep_fold.h) -----------------------------------------------
// The matrix is on the device already; a fold is its picks.  Per fold the host sees 2 n sums, 2 n counts, n diagonal
// flags, 2 n column counts and the totals, and sends the picks, 2 (n + 1) offsets and, where one is applied, the order.
namespace {

// One fold as the device prepared it: the n-sized results on the host, the lists in the handle's device buffers.
struct FoldPrepared {
  std::vector<int32_t> order, degrees;   // order[0] = -1: input order kept; degrees per caller's point
  int32_t route = TOPOLOW_ORDER_PRESERVED;
  double numeric_max = NAN;
  int64_t n_edges = 0, n_pairs = 0, n_scored = 0;
  const int32_t* d_order = nullptr;      // on the device, where the scored cells are gathered through the order
};

int prep_fold_check_handle(const topolow_layout_prep* p, char* errbuf, size_t errlen) {
  if (!p->declined && !p->order.empty() && p->order[0] == -1) return TOPOLOW_OK;
  set_err(errbuf, errlen, "a fold's labels are the caller's, the full matrix's order is of no use to it: create the "
          "handle with preserve_order");
  return TOPOLOW_ERR_BAD_ARGUMENT;
}

void prep_fold_alloc(topolow_layout_prep* p) {   // on the handle's device, which it makes the current one
  auto& f = p->fold;
  HIP_TRY(hipSetDevice(p->device));
  if (f.ready) return;
  const size_t N = (size_t)p->n;
  if (!f.stream) HIP_TRY(hipStreamCreateWithFlags(&f.stream, hipStreamNonBlocking));
  f.mask_words = (N * N + 31) / 32;
  prep_alloc(f.mask, f.mask_words, "the fold mask");
  f.sums.alloc(p->n);
  prep_alloc(f.col_counts, 2 * N, "the column counts");
  prep_alloc(f.offsets, 2 * (N + 1), "the column offsets");
  prep_alloc(f.order, N, "the fold's order");
  HIP_TRY(hipMemsetAsync(f.mask.p, 0, f.mask_words * 4, f.stream));
  HIP_TRY(hipStreamSynchronize(f.stream));   // whichever stream the first fold works on finds the mask empty
  f.ready = true;
}

// The mask is empty again when this leaves scope, whatever happened in between.
struct FoldMaskGuard {
  topolow_layout_prep* p;
  hipStream_t stream;
  ~FoldMaskGuard() {
    if (!p->fold.ready) return;
    (void)hipMemsetAsync(p->fold.mask.p, 0, p->fold.mask_words * 4, stream);
    (void)hipStreamSynchronize(stream);
  }
};

// Once per handle (the first fold): is the matrix symmetric?  Throws kAsymmetricCells where it is not.
void prep_fold_symmetry(topolow_layout_prep* p) {
  auto& f = p->fold;
  if (!f.symmetry_known) {
    const int nb = (p->n + kPrepTile - 1) / kPrepTile;
    FoldTotals tot;
    HIP_TRY(hipMemsetAsync(f.sums.totals.p, 0, sizeof(FoldTotals), f.stream));
    hipLaunchKernelGGL(fold_symmetry_kernel, dim3(nb, nb), dim3(kPrepThreads), 0, f.stream, p->vals.p,
                       p->has_codes ? p->codes.p : nullptr, p->n, f.sums.totals.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&tot, f.sums.totals.p, sizeof tot, hipMemcpyDeviceToHost, f.stream));
    HIP_TRY(hipStreamSynchronize(f.stream));
    f.symmetric = tot.n_asymmetric == 0;
    f.symmetry_known = true;
  }
  if (!f.symmetric) throw HipError{TOPOLOW_ERR_UNSUPPORTED, kAsymmetricCells};
}

// mark, masked sums, order, compaction -- on `stream`, which is idle when this returns.  The mask stays set: the caller
// holds a FoldMaskGuard.
void prep_fold_prepare(topolow_layout_prep* p, hipStream_t stream, const int64_t* picks, int64_t n_picks,
                       int32_t preserve_order, int32_t named, FoldPrepared& out) {
  auto& f = p->fold;
  const int n = p->n;
  const size_t N = (size_t)n;
  const int nb = (n + kPrepTile - 1) / kPrepTile;
  const int8_t* codes = p->has_codes ? p->codes.p : nullptr;
  auto& S = f.sums;
  HIP_TRY(hipMemsetAsync(S.totals.p, 0, sizeof(FoldTotals), stream));
  if (n_picks > 0) {
    grow_buf(f.picks, (size_t)n_picks);
    HIP_TRY(hipMemcpyAsync(f.picks.p, picks, (size_t)n_picks * 8, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(fold_mark_kernel, dim3((unsigned)((n_picks + kPrepThreads - 1) / kPrepThreads)), dim3(kPrepThreads),
                       0, stream, f.picks.p, (long long)n_picks, n, f.mask.p, S.totals.p);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(fold_sums_kernel, dim3(nb, nb), dim3(kPrepThreads), 0, stream, p->vals.p, codes, f.mask.p, n,
                     S.part_slow_sum.p, S.part_slow_cnt.p, S.part_fast_sum.p, S.part_fast_cnt.p, S.diag.p, S.totals.p);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(fold_compact_count_kernel, dim3(n), dim3(kPrepThreads), 0, stream, p->vals.p, codes, f.mask.p, n,
                     f.col_counts.p, f.col_counts.p + N);
  HIP_TRY(hipGetLastError());
  std::vector<int32_t> per_col(2 * N);
  S.fetch(n, stream);
  HIP_TRY(hipMemcpyAsync(per_col.data(), f.col_counts.p, 2 * N * 4, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (S.tot.n_bad_picks > 0)
    throw HipError{TOPOLOW_ERR_BAD_ARGUMENT, std::to_string(S.tot.n_bad_picks) + " of the fold's picks lie outside the matrix (linear column-major indices 0 .. n * n - 1)"};

  // -- the n-sized results.  The buffer is read column-major (relax_prep_fold.h): slow lines are columns, fast lines rows.
  const size_t row_at = N, col_at = 0;
  out.order.assign(N, 0);
  out.order[0] = -1;
  out.route = preserve_order ? TOPOLOW_ORDER_PRESERVED
                             : S.order(n, row_at, col_at, p->exact_sums, p->negative_or_infinite, out.order.data());
  out.degrees.assign(S.cnts.begin() + row_at, S.cnts.begin() + row_at + N);
  out.n_edges = (int64_t)S.tot.n_upper;
  out.numeric_max = S.numeric_max();

  // -- the stable compaction of the mask: held-out pairs and scored cells, column by column
  std::vector<int64_t> off(2 * (N + 1));
  out.n_pairs = prep_offsets(per_col.data(), N, off.data());
  out.n_scored = prep_offsets(per_col.data() + N, N, off.data() + N + 1);
  out.d_order = nullptr;
  if (out.n_pairs + out.n_scored > 0) {
    grow_buf(f.pair_i, (size_t)out.n_pairs); grow_buf(f.pair_j, (size_t)out.n_pairs);
    grow_buf(f.score_r, (size_t)out.n_scored); grow_buf(f.score_c, (size_t)out.n_scored);
    grow_buf(f.score_truth, (size_t)out.n_scored);
    HIP_TRY(hipMemcpyAsync(f.offsets.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(fold_compact_write_kernel, dim3(n), dim3(kPrepThreads), 0, stream, p->vals.p, codes, f.mask.p, n,
                       f.offsets.p, f.offsets.p + N + 1, f.pair_i.p, f.pair_j.p, f.score_r.p, f.score_c.p,
                       f.score_truth.p);
    HIP_TRY(hipGetLastError());
  }
  if (!named && out.order[0] != -1 && out.n_scored > 0) {   // an unnamed matrix is scored in the returned numbering
    HIP_TRY(hipMemcpyAsync(f.order.p, out.order.data(), N * 4, hipMemcpyHostToDevice, stream));
    out.d_order = f.order.p;
  }
  HIP_TRY(hipStreamSynchronize(stream));   // (the host arrays of the offsets go out of scope)
}

unsigned fold_grid(int64_t count) { return (unsigned)((count + kPrepThreads - 1) / kPrepThreads); }

// Folds prepared from a handle on the session's stream (prep_fold_prepare); a fold's guard empties the mask after it.
struct HandleFolds {
  topolow_layout_prep* p;
  const SweepArgs& a;
  int32_t* order_route;
  struct Fold { FoldMaskGuard guard; int code = TOPOLOW_OK; FoldPrepared fp; std::vector<double> pos; };
  int n = 0, device = 0;
  const int32_t* degrees = nullptr;
  double* seconds = nullptr;
  int begin(char* errbuf, size_t errlen) {
    if (const int rch = prep_fold_check_handle(p, errbuf, errlen)) return rch;
    n = p->n; device = p->device; degrees = p->degrees.data(); seconds = p->fold.seconds;
    const int64_t cells = (int64_t)n * n;
    for (int f = 0; f < a.n_folds; ++f)
      for (int64_t q = a.picks_offset[f]; q < a.picks_offset[f + 1]; ++q)
        if (!a.picks || a.picks[q] < 0 || a.picks[q] >= cells) {
          set_err(errbuf, errlen, "fold %d: pick %lld lies outside the matrix (linear column-major indices 0 .. n * n - 1)",
                  f, (long long)(q - a.picks_offset[f]));
          return TOPOLOW_ERR_BAD_ARGUMENT;
        }
    const int rc = guarded(errbuf, errlen, [&] { prep_fold_alloc(p); prep_fold_symmetry(p); });
    for (int f = 0; f < a.n_folds && rc == TOPOLOW_OK; ++f) order_route[f] = TOPOLOW_ORDER_PRESERVED;
    return rc;
  }
  int load(topolow_session* t, char* eb, size_t el) const { return topolow_session_load_prepared(t, p, eb, el); }
  void prefetch(int) {}   // (nothing is prepared ahead, so drain() has nothing to wait for)
  void drain() {}
  std::unique_ptr<Fold> prepare(topolow_session* s, int f, int* rc, char* errbuf, size_t errlen) {
    std::unique_ptr<Fold> o;
    *rc = guarded(errbuf, errlen, [&] {
      o.reset(new Fold{FoldMaskGuard{p, s->stream}});
      HIP_TRY(hipSetDevice(p->device));
      prep_fold_prepare(p, s->stream, a.picks + a.picks_offset[f], a.picks_offset[f + 1] - a.picks_offset[f],
                        a.preserve_order, a.named, o->fp);
      order_route[f] = o->fp.route;
      if (o->fp.route == TOPOLOW_ORDER_DECLINED) {   // the caller reruns this fold with the host's ordering
        o->code = TOPOLOW_ERR_UNSUPPORTED;
        return;
      }
      o->code = fold_check(TOPOLOW_OK, o->fp.n_edges, o->fp.numeric_max, a.ndim[f], a.draws_offset[f + 1] - a.draws_offset[f], p->n);
      if (o->code == TOPOLOW_OK)
        start_walk(a.unit_draws + a.draws_offset[f], o->fp.numeric_max, p->n, a.ndim[f],
                   o->fp.order[0] >= 0 ? o->fp.order.data() : nullptr, o->pos);
    });
    return o;
  }
  // the shared hold-out, its pairs mapped to session labels on the device
  int hold_out(topolow_session* s, const Fold& o, char* errbuf, size_t errlen) const {
    if (const int rc = cv_check_hold_out(s, errbuf, errlen)) return rc;
    return guarded(errbuf, errlen, [&] {
      cv_hold_out_pairs(s, (long long)o.fp.n_pairs, o.fp.degrees.data(), [&](int* d_lo, int* d_hi) {
        hipLaunchKernelGGL(fold_pair_labels_kernel, dim3(fold_grid(o.fp.n_pairs)), dim3(kPrepThreads), 0, s->stream,
                           p->fold.pair_i.p, p->fold.pair_j.p, (long long)o.fp.n_pairs,
                           s->inv.empty() ? nullptr : s->d_inv.p, d_lo, d_hi);
        HIP_TRY(hipGetLastError());
      });
    });
  }
  // the shared score: the scored cells' points gathered through the order and the session's labels on the device
  int score(topolow_session* s, const Fold& o, double* sum_abs, int64_t* count, char* errbuf, size_t errlen) const {
    if (o.fp.n_scored == 0) return TOPOLOW_OK;
    return guarded(errbuf, errlen, [&] {
      auto& c = s->cv;
      const auto& h = p->fold;
      grow_buf(c.sc_i, (size_t)o.fp.n_scored); grow_buf(c.sc_j, (size_t)o.fp.n_scored);
      hipLaunchKernelGGL(fold_score_points_kernel, dim3(fold_grid(o.fp.n_scored)), dim3(kPrepThreads), 0, s->stream,
                         h.score_r.p, h.score_c.p, (long long)o.fp.n_scored, o.fp.d_order,
                         s->inv.empty() ? nullptr : s->d_inv.p, c.sc_i.p, c.sc_j.p);
      HIP_TRY(hipGetLastError());
      cv_score_device(s, c.sc_i.p, c.sc_j.p, h.score_truth.p, (long long)o.fp.n_scored, sum_abs, count);
    });
  }
};

}  // namespace

// ---- the fit report of a resident embedding (relax_fit.h) ---------------------------------------------------------------
// fit_check_arguments, fit_check_series and fit_run are declared in topolow_prep.h: the binned diagnostics
// (topolow_fit_bins.hip) check their arguments and mark their picks through them.

static_assert(kFitMaxRanks == TOPOLOW_FIT_MAX_RANKS, "relax_fit.h and the header disagree");

int fit_check_arguments(const char* entry, const topolow_layout_prep* p, const double* positions, int32_t ndim,
                        const int64_t* picks, int64_t n_picks, const void* out, char* errbuf, size_t errlen) {
  if (!p || !positions || !out) {
    set_err(errbuf, errlen, "%s: the handle, positions and the outputs must not be NULL", entry);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (ndim < 1) {
    set_err(errbuf, errlen, "%s: ndim >= 1 is required (got %d)", entry, ndim);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (n_picks < 0 || (!picks && n_picks > 0)) {
    set_err(errbuf, errlen, "%s: n_picks >= 0 is required, and picks must not be NULL when it is > 0", entry);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  return TOPOLOW_OK;
}

int fit_check_series(const char* entry, int32_t series, char* errbuf, size_t errlen) {
  if (series == TOPOLOW_FIT_IN || series == TOPOLOW_FIT_OUT || series == TOPOLOW_FIT_ALL) return TOPOLOW_OK;
  set_err(errbuf, errlen, "%s: unknown series %d (TOPOLOW_FIT_IN, _OUT or _ALL)", entry, series);
  return TOPOLOW_ERR_BAD_ARGUMENT;
}

// The positions go up, the picks are marked in the handle's fold mask, body(inputs) runs, and the mask is empty again
// when this returns, whatever body threw.  No picks: no mask is allocated and none is read.
int fit_run(topolow_layout_prep* p, const double* positions, int32_t ndim, const int64_t* picks, int64_t n_picks,
            char* errbuf, size_t errlen, const std::function<void(const FitInputs&)>& body) {
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(p->device));
    const int n = p->n;
    std::vector<double> rowmajor((size_t)n * ndim);
    for (int i = 0; i < n; ++i)
      for (int d = 0; d < ndim; ++d) rowmajor[(size_t)i * ndim + d] = positions[i + (size_t)d * n];
    DevBuf<double> dpos;
    PostPipe P;   // destroyed before dpos
    prep_alloc(dpos, rowmajor.size(), "the positions");
    P.create(0, 0);
    std::unique_ptr<FoldMaskGuard> guard;   // destroyed before the stream it clears the mask on
    FitInputs in = {dpos.p, p->vals.p, p->has_codes ? p->codes.p : nullptr, p->order[0] != -1 ? p->ord.p : nullptr, nullptr,
                    P.run};
    HIP_TRY(hipMemcpyAsync(dpos.p, rowmajor.data(), rowmajor.size() * 8, hipMemcpyHostToDevice, P.run));
    if (n_picks > 0) {
      auto& f = p->fold;
      prep_fold_alloc(p);
      guard.reset(new FoldMaskGuard{p, P.run});
      FoldTotals tot;
      if (f.picks.p == nullptr || f.picks.n < (size_t)n_picks) prep_alloc(f.picks, (size_t)n_picks, "the picks");
      HIP_TRY(hipMemsetAsync(f.sums.totals.p, 0, sizeof(FoldTotals), P.run));
      HIP_TRY(hipMemcpyAsync(f.picks.p, picks, (size_t)n_picks * 8, hipMemcpyHostToDevice, P.run));
      hipLaunchKernelGGL(fold_mark_kernel, dim3((unsigned)((n_picks + kPrepThreads - 1) / kPrepThreads)), dim3(kPrepThreads),
                         0, P.run, f.picks.p, (long long)n_picks, n, f.mask.p, f.sums.totals.p);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(&tot, f.sums.totals.p, sizeof tot, hipMemcpyDeviceToHost, P.run));
      HIP_TRY(hipStreamSynchronize(P.run));
      if (tot.n_bad_picks > 0)
        throw HipError{TOPOLOW_ERR_BAD_ARGUMENT, std::to_string(tot.n_bad_picks) + " of the fold's picks lie outside the matrix (linear column-major indices 0 .. n * n - 1)"};
      in.mask = f.mask.p;
    }
    HIP_TRY(hipStreamSynchronize(P.run));   // rowmajor is pageable
    body(in);
  });
}

extern "C" {

int topolow_layout_prep_fold(topolow_layout_prep* p, const int64_t* picks, int64_t n_picks, int32_t preserve_order,
                             int32_t named, int32_t* order, int32_t* degrees, double* numeric_max, int64_t* n_edges,
                             int32_t* pair_i, int32_t* pair_j, int64_t* n_pairs, int32_t* score_i, int32_t* score_j,
                             double* score_truth, int64_t* n_scored, int32_t* order_route, char* errbuf, size_t errlen) {
  if (!p || n_picks < 0 || (!picks && n_picks > 0) || !order || !degrees || !numeric_max || !n_edges || !pair_i ||
      !pair_j || !n_pairs || !score_i || !score_j || !score_truth || !n_scored || !order_route) {
    set_err(errbuf, errlen, "null argument, or n_picks < 0");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (const int rch = prep_fold_check_handle(p, errbuf, errlen)) return rch;
  return guarded(errbuf, errlen, [&] {
    prep_fold_alloc(p);
    prep_fold_symmetry(p);
    auto& f = p->fold;
    FoldMaskGuard guard{p, f.stream};
    FoldPrepared fp;
    prep_fold_prepare(p, f.stream, picks, n_picks, preserve_order, named, fp);
    std::copy(fp.order.begin(), fp.order.end(), order);
    std::copy(fp.degrees.begin(), fp.degrees.end(), degrees);
    *numeric_max = fp.numeric_max;
    *n_edges = fp.n_edges;
    *n_pairs = fp.n_pairs;
    *n_scored = fp.n_scored;
    *order_route = fp.route;
    if (fp.n_pairs > 0) {
      HIP_TRY(hipMemcpyAsync(pair_i, f.pair_i.p, (size_t)fp.n_pairs * 4, hipMemcpyDeviceToHost, f.stream));
      HIP_TRY(hipMemcpyAsync(pair_j, f.pair_j.p, (size_t)fp.n_pairs * 4, hipMemcpyDeviceToHost, f.stream));
    }
    if (fp.n_scored > 0) {
      grow_buf(f.score_i, (size_t)fp.n_scored); grow_buf(f.score_j, (size_t)fp.n_scored);
      hipLaunchKernelGGL(fold_score_points_kernel, dim3(fold_grid(fp.n_scored)), dim3(kPrepThreads), 0, f.stream,
                         f.score_r.p, f.score_c.p, (long long)fp.n_scored, fp.d_order, (const int*)nullptr, f.score_i.p,
                         f.score_j.p);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(score_i, f.score_i.p, (size_t)fp.n_scored * 4, hipMemcpyDeviceToHost, f.stream));
      HIP_TRY(hipMemcpyAsync(score_j, f.score_j.p, (size_t)fp.n_scored * 4, hipMemcpyDeviceToHost, f.stream));
      HIP_TRY(hipMemcpyAsync(score_truth, f.score_truth.p, (size_t)fp.n_scored * 8, hipMemcpyDeviceToHost, f.stream));
    }
    HIP_TRY(hipStreamSynchronize(f.stream));
  });
}

int topolow_layout_prep_cv_sweep(topolow_layout_prep* p, int32_t named, int32_t preserve_order, int32_t n_folds,
                                 const int32_t* ndim, const double* k0, const double* cooling_rate,
                                 const double* c_repulsion, const int64_t* picks, const int64_t* picks_offset,
                                 const double* unit_draws, const int64_t* draws_offset, const uint64_t* seeds,
                                 int32_t n_iter, double relative_epsilon, int32_t convergence_window,
                                 int32_t convergence_check_freq, int32_t precision, int32_t schedule,
                                 double* holdout_sum_abs, int64_t* holdout_count, int32_t* iterations, int32_t* converged,
                                 int32_t* error_code, int32_t* order_route, double* device_seconds, char* errbuf,
                                 size_t errlen) {
  const SweepArgs a{named, preserve_order, n_folds, ndim, k0, cooling_rate, c_repulsion, picks, picks_offset, unit_draws,
                    draws_offset, seeds, n_iter, relative_epsilon, convergence_window, convergence_check_freq, precision,
                    schedule, holdout_sum_abs, holdout_count, iterations, converged, error_code, device_seconds};
  if (n_folds > 0 && !order_route) {
    set_err(errbuf, errlen, "null argument: order_route");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  HandleFolds src{p, a, order_route};
  return cv_sweep_resident(p, src, a, errbuf, errlen);
}

int topolow_layout_prep_fold_seconds(const topolow_layout_prep* p, double* seconds) {
  if (!p || !seconds) return TOPOLOW_ERR_BAD_ARGUMENT;
  for (int q = 0; q < 4; ++q) seconds[q] = p->fold.seconds[q];
  return TOPOLOW_OK;
}

int topolow_layout_prep_fit_report(topolow_layout_prep* p, const double* positions, int32_t ndim,
                                   const int64_t* picks, int64_t n_picks, topolow_fit_report* out, char* errbuf,
                                   size_t errlen) {
  if (const int rca = fit_check_arguments("topolow_layout_prep_fit_report", p, positions, ndim, picks, n_picks, out, errbuf,
                                          errlen))
    return rca;
  if (const int rcu = prep_check_usable(p, errbuf, errlen)) return rcu;
  const double t0 = now_s();
  return fit_run(p, positions, ndim, picks, n_picks, errbuf, errlen, [&](const FitInputs& in) {
    const int n = p->n;
    const size_t N = (size_t)n;
    *out = topolow_fit_report();
    // -- pass 1: one partial per line, the lines added in index order
    DevBuf<FitLineSums> dsums;
    DevBuf<FitLineCentred> dcss;
    prep_alloc(dsums, N, "the lines' sums");
    prep_alloc(dcss, N, "the lines' centred sums");
    std::vector<FitLineSums> ls(N);
    std::vector<FitLineCentred> lc(N);
    hipLaunchKernelGGL(fit_sums_kernel, dim3(n), dim3(kFitThreads), 0, in.stream, in.pos, n, ndim, in.vals, in.codes, in.ord,
                       in.mask, dsums.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ls.data(), dsums.p, N * sizeof(FitLineSums), hipMemcpyDeviceToHost, in.stream));
    HIP_TRY(hipStreamSynchronize(in.stream));
    double sum[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < kFitSeries; ++s) {
      out->series[s].min_e = INFINITY;
      out->series[s].max_e = -INFINITY;
    }
    for (size_t a = 0; a < N; ++a) {
      for (int k = 0; k < 12; ++k) sum[k] += ls[a].sum[k];
      for (int s = 0; s < kFitSeries; ++s) {
        topolow_fit_series& o = out->series[s];
        o.count += ls[a].count[s];
        o.min_e = std::fmin(o.min_e, ls[a].min_e[s]);
        o.max_e = std::fmax(o.max_e, ls[a].max_e[s]);
        if (s < 2) o.pct_count += ls[a].pct_count[s];
      }
    }
    FitMeans means = {{0.0, 0.0, 0.0}, 0.0, 0.0};
    for (int s = 0; s < kFitSeries; ++s) {
      topolow_fit_series& o = out->series[s];
      o.sum_e = sum[s];
      o.sum_abs_e = sum[3 + s];
      if (s < 2) { o.sum_pct = sum[6 + s]; o.sum_abs_pct = sum[8 + s]; }
      if (o.count == 0) o.min_e = o.max_e = NAN;
      else means.e[s] = o.sum_e / (double)o.count;
    }
    topolow_fit_series& all = out->series[TOPOLOW_FIT_ALL];
    all.sum_v = sum[10];
    all.sum_r = sum[11];
    if (all.count > 0) {
      means.v = all.sum_v / (double)all.count;
      means.r = all.sum_r / (double)all.count;
    }
    const double t1 = now_s();
    // -- pass 2: about the means
    hipLaunchKernelGGL(fit_centred_kernel, dim3(n), dim3(kFitThreads), 0, in.stream, in.pos, n, ndim, in.vals, in.codes,
                       in.ord, in.mask, means, dcss.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(lc.data(), dcss.p, N * sizeof(FitLineCentred), hipMemcpyDeviceToHost, in.stream));
    HIP_TRY(hipStreamSynchronize(in.stream));
    double css[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (size_t a = 0; a < N; ++a)
      for (int k = 0; k < 6; ++k) css[k] += lc[a].css[k];
    for (int s = 0; s < kFitSeries; ++s) out->series[s].css_e = css[s];
    all.css_v = css[3];
    all.css_r = css[4];
    all.css_vr = css[5];
    const double t2 = now_s();
    out->seconds[0] = t1 - t0;
    out->seconds[1] = t2 - t1;
    out->seconds[2] = t2 - t0;
  });
}

int topolow_layout_prep_fit_order_stats(topolow_layout_prep* p, const double* positions, int32_t ndim,
                                        const int64_t* picks, int64_t n_picks, int32_t series,
                                        const int64_t* ranks, int32_t n_ranks, double* values_out, int64_t* count_out,
                                        char* errbuf, size_t errlen) {
  const char* entry = "topolow_layout_prep_fit_order_stats";
  if (const int rca = fit_check_arguments(entry, p, positions, ndim, picks, n_picks,
                                          ranks && values_out && count_out ? (const void*)values_out : nullptr, errbuf,
                                          errlen))
    return rca;
  if (const int rcs = fit_check_series(entry, series, errbuf, errlen)) return rcs;
  if (n_ranks < 1 || n_ranks > TOPOLOW_FIT_MAX_RANKS) {
    set_err(errbuf, errlen, "%s: 1 <= n_ranks <= %d is required (got %d)", entry, TOPOLOW_FIT_MAX_RANKS, n_ranks);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  for (int k = 0; k < n_ranks; ++k) {
    if (ranks[k] >= 0) continue;
    const int64_t code = -1 - ranks[k], q = code >= TOPOLOW_FIT_RANK_UPPER ? code - TOPOLOW_FIT_RANK_UPPER : code;
    if (q > 1000000) {
      set_err(errbuf, errlen, "%s: rank %d: a negative rank is -1 - q or -1 - (q + TOPOLOW_FIT_RANK_UPPER) with q in "
              "0 .. 1000000", entry, k);
      return TOPOLOW_ERR_BAD_ARGUMENT;
    }
  }
  if (const int rcu = prep_check_usable(p, errbuf, errlen)) return rcu;
  return fit_run(p, positions, ndim, picks, n_picks, errbuf, errlen, [&](const FitInputs& in) {
    const int n = p->n;
    DevBuf<FitSelect> sel;
    prep_alloc(sel, 1, "the select histograms");
    std::vector<FitSelect> hbuf(1);
    FitSelect& h = hbuf[0];
    FitPrefixes prefix = {};
    unsigned long long rank[kFitMaxRanks] = {}, m = 0;
    unsigned digit[kFitMaxRanks] = {};
    for (int shift = 56; shift >= 0; shift -= 8) {   // exactly eight passes
      HIP_TRY(hipMemsetAsync(sel.p, 0, sizeof(FitSelect), in.stream));
      hipLaunchKernelGGL(fit_select_kernel, dim3(n), dim3(kFitThreads), 0, in.stream, in.pos, n, ndim, in.vals, in.codes,
                         in.ord, in.mask, series, shift, n_ranks, prefix, sel.p);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(&h, sel.p, sizeof(FitSelect), hipMemcpyDeviceToHost, in.stream));
      HIP_TRY(hipStreamSynchronize(in.stream));
      if (shift == 56) {
        for (int q = 0; q < 256; ++q) m += h.hist[0][q];
        *count_out = (int64_t)m;
        if (m == 0) {
          for (int k = 0; k < n_ranks; ++k) values_out[k] = NAN;
          return;
        }
        for (int k = 0; k < n_ranks; ++k) {
          if (ranks[k] >= 0) {
            rank[k] = (unsigned long long)ranks[k];
          } else {
            const int64_t code = -1 - ranks[k];
            const bool upper = code >= TOPOLOW_FIT_RANK_UPPER;
            const unsigned __int128 h6 = (unsigned __int128)(m - 1) * (unsigned long long)(upper ? code - TOPOLOW_FIT_RANK_UPPER : code);
            rank[k] = (unsigned long long)(h6 / 1000000u) + (upper && h6 % 1000000u != 0 ? 1ull : 0ull);
          }
          if (rank[k] >= m)
            throw HipError{TOPOLOW_ERR_BAD_ARGUMENT, "rank " + std::to_string(rank[k]) + " (entry " + std::to_string(k) +
                                                         ") is not below the series' count " + std::to_string(m)};
        }
      }
      for (int k = 0; k < n_ranks; ++k) {
        digit[k] = spec_pick_digit(h.hist[k], rank[k]);
        prefix.key[k] |= (unsigned long long)digit[k] << shift;
      }
    }
    for (int k = 0; k < n_ranks; ++k) {
      if (h.hist[k][digit[k]] < 1 || rank[k] >= h.hist[k][digit[k]])
        throw HipError{TOPOLOW_ERR_HIP, "the select did not find the key of rank entry " + std::to_string(k) +
                                            " in its eighth pass: the matrix or the positions changed during the call"};
      values_out[k] = spec_key_value(prefix.key[k]);
    }
  });
}

}  // extern "C"
