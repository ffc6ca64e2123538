// topolow_amd/csrc/topolow_drivers.hip -- the drivers of libtopolow_relax.so: whole embeddings and cross-validation
// sweeps run on sessions, the host's fold entries and the verbose report.  Host code only: it reaches a session through
// the C ABI and the fields of topolow_session.h, as the handle's sources do, and this source compiles no kernel -- it
// includes no header that defines a plain __global__ function (relax_gs.h is here for gs_lds_bytes).
//
// Replaces the native half of the reference's euclidean_embedding():
//   .Call(`_topolow_optimize_layout_exact_cpp`, ...)  (reference R/RcppExports.R:4-6)
//   -> optimize_layout_exact_cpp                       (reference src/optimization.cpp:109-382)

#include "topolow_drivers.h"
#include "relax_fold.h"
#include "relax_gs.h"

namespace {

constexpr int kDefaultGsMaxN = 1024;

// verbose lines go to the caller's sink (topolow_options.print_cb) or stdout
void emit(const topolow_options& opt, const char* fmt, ...) {
  char line[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(line, sizeof line, fmt, ap);
  va_end(ap);
  if (opt.print_cb) opt.print_cb(line, opt.print_user);
  else { std::fputs(line, stdout); std::fflush(stdout); }
}

// The reference's opening lines (src/optimization.cpp:183-188) plus which device path runs.
void emit_header(const topolow_options& opt, const char* path, int n, double k0, double cooling, double c_rep) {
  emit(opt, "=== Exact Algorithm (O(N^2) Full Pairwise) on HIP: %s ===\n", path);
  emit(opt, "Points: %d, Pairs per iteration: %lld\n", n, (long long)n * (n - 1) / 2);
  emit(opt, "Parameters: k0=%g, cooling=%g, c_rep=%g\n", k0, cooling, c_rep);
}

// Progress lines of the checks [from, to) of a trace (3 doubles per check), with the reference's
// cadence: checks that fall on a multiple of 10 iterations or on the last one (:298-301).
void emit_checks(const topolow_options& opt, const double* trace, int from, int to, int n_iter) {
  for (int c = from; c < to; ++c) {
    const int it = (int)trace[3 * c];
    if (it % 10 == 0 || it == n_iter)
      emit(opt, "Iter %d/%d, MAE=%g, k=%g\n", it, n_iter, trace[3 * c + 1], trace[3 * c + 2]);
  }
}

// Closing line of a converged run (:334-336, :351-353): the controller's counters tell which rule fired.
void emit_converged(const topolow_options& opt, bool plateau, int best_iter, double best_mae) {
  if (plateau) emit(opt, "Converged (plateau) at iter %d, MAE=%g\n", best_iter, best_mae);
  else emit(opt, "Converged (MAE worsening, best restored) at iter %d, MAE=%g\n", best_iter, best_mae);
}

// Schedule gs is tuned up to kMaxTunedDim dimensions: the one place that says so to a caller.
int check_gs_dim(int ndim, char* errbuf, size_t errlen) {
  if (ndim <= kMaxTunedDim) return TOPOLOW_OK;
  set_err(errbuf, errlen, "schedule gs: ndim must be between 1 and %d (wider embeddings run the slab schedule)", kMaxTunedDim);
  return TOPOLOW_ERR_UNSUPPORTED;
}

// Folds from the host's cell list (fold_pairs), each prepared on a host thread while the fold before it runs.
struct CellFolds {
  const topolow_cell_list* cells;
  const SweepArgs& a;
  int32_t device, n = 0;
  struct Fold { int code = TOPOLOW_OK; FoldPairs fp; std::vector<double> pos; };
  std::vector<int32_t> fi, fj, ft, fdeg;   // what the sessions load: the (symmetric) list's upper triangle, degrees
  std::vector<double> fd;
  const int32_t* degrees = nullptr;
  double untold[4], *seconds = untold;
  std::future<std::unique_ptr<Fold>> next;
  bool next_valid = false;
  int begin(char* errbuf, size_t errlen) {
    n = cells->n;
    return guarded(errbuf, errlen, [&] {
      if (n < 2) throw HipError{TOPOLOW_ERR_TOO_FEW_POINTS, "Need at least 2 points for embedding"};
      if (!fold_cells_symmetric(cells)) throw HipError{TOPOLOW_ERR_UNSUPPORTED, kAsymmetricCells};
      fdeg.resize((size_t)n); degrees = fdeg.data();
      for (int i = 0; i < n; ++i) fdeg[(size_t)i] = (int32_t)(cells->row_ptr[i + 1] - cells->row_ptr[i]);
      for (int64_t q = 0; q < cells->n_cells; ++q)
        if (cells->row[q] < cells->col[q]) {
          fi.push_back(cells->row[q]); fj.push_back(cells->col[q]); fd.push_back(cells->value[q]); ft.push_back(cells->code[q]);
        }
    });
  }
  int load(topolow_session* t, char* eb, size_t el) const {
    const int rcl = topolow_session_load_coo(t, fi.data(), fj.data(), fd.data(), ft.data(), (int64_t)fi.size(), fdeg.data(), eb, el);
    return rcl ? rcl : topolow_session_set_edges(t, fi.data(), fj.data(), fd.data(), ft.data(), (int64_t)fi.size(), eb, el);
  }
  std::unique_ptr<Fold> build(int f) const {
    auto p = std::make_unique<Fold>();
    try {
      p->code = fold_pairs(cells, a.picks + a.picks_offset[f], a.picks_offset[f + 1] - a.picks_offset[f], a.preserve_order, a.named, p->fp);
      p->code = fold_check(p->code, p->fp.n_edges, p->fp.numeric_max, a.ndim[f], a.draws_offset[f + 1] - a.draws_offset[f], n);
      if (p->code != TOPOLOW_OK) return p;
      // the random walk of topolow_cv_sweep in the caller's labels
      start_walk(a.unit_draws + a.draws_offset[f], p->fp.numeric_max, n, a.ndim[f],
                 p->fp.order[0] >= 0 ? p->fp.order.data() : nullptr, p->pos);
    } catch (const std::bad_alloc&) {
      p->code = TOPOLOW_ERR_HIP;
    }
    return p;
  }
  void prefetch(int f) { next = std::async(std::launch::async, [this, f] { return build(f); }); next_valid = true; }
  std::unique_ptr<Fold> prepare(topolow_session*, int, int*, char*, size_t) { next_valid = false; return next.get(); }
  void drain() { if (next_valid) (void)next.get(); next_valid = false; }
  int hold_out(topolow_session* s, const Fold& p, char* errbuf, size_t errlen) const {
    return topolow_session_hold_out(s, p.fp.pair_i.data(), p.fp.pair_j.data(), (int64_t)p.fp.pair_i.size(),
                                    p.fp.degrees.data(), errbuf, errlen);
  }
  int score(topolow_session* s, const Fold& p, double* sum_abs, int64_t* count, char* errbuf, size_t errlen) const {
    return topolow_session_score_pairs(s, p.fp.score_i.data(), p.fp.score_j.data(), p.fp.score_truth.data(),
                                       (int64_t)p.fp.score_i.size(), sum_abs, count, errbuf, errlen);
  }
};

}  // namespace

// The arguments the sweeps share: the cell list (or the prepared handle) always, the per-fold arrays wherever there is a fold.
bool cv_sweep_args_ok(const void* cells, int32_t n_folds, const int32_t* ndim, const double* k0,
                      const double* cooling_rate, const double* c_repulsion, const int64_t* picks_offset,
                      const double* unit_draws, const int64_t* draws_offset, const uint64_t* seeds,
                      const double* holdout_sum_abs, const int64_t* holdout_count, const int32_t* iterations,
                      const int32_t* converged, const int32_t* error_code) {
  if (!cells || n_folds < 0) return false;
  return n_folds == 0 || (ndim && k0 && cooling_rate && c_repulsion && picks_offset && unit_draws && draws_offset && seeds &&
                          holdout_sum_abs && holdout_count && iterations && converged && error_code);
}

// A whole-problem session, opened: session_create, tile Gauss-Seidel where asked for, the labels shuffled by
// relabel_seed (slabs / tiles of random points instead of index-contiguous ones; NULL: the caller's labels), then the
// loader.  Where a step fails nothing stays open and *out is NULL.
int open_session(topolow_session** out, int32_t n, int32_t ndim, bool tile_gs, int32_t precision, int32_t device,
                 const uint64_t* relabel_seed, const SessionLoader& load, char* errbuf, size_t errlen) {
  *out = nullptr;
  topolow_session* s = nullptr;
  int rc = topolow_session_create(&s, n, ndim, 0, n, precision, device, errbuf, errlen);
  if (rc != TOPOLOW_OK) return rc;
  if (tile_gs) {
    rc = check_gs_dim(ndim, errbuf, errlen);
    if (rc == TOPOLOW_OK) rc = topolow_session_set_schedule(s, TOPOLOW_SCHEDULE_GS);
  }
  if (rc == TOPOLOW_OK && relabel_seed)
    rc = topolow_session_set_relabel(s, mix64(*relabel_seed ^ 0x1abe15eedull) | 1ull, errbuf, errlen);
  if (rc == TOPOLOW_OK) rc = load(s, errbuf, errlen);
  if (rc != TOPOLOW_OK) {
    topolow_session_destroy(s);
    return rc;
  }
  *out = s;
  return TOPOLOW_OK;
}

// Every iteration of a begun run, enqueued 50 at a time: the reference's interrupt cadence (src/optimization.cpp:364).
// after_chunk, where there is one, runs after each chunk that enqueued work; anything but TOPOLOW_OK from it ends the
// run with that code.
int enqueue_run(topolow_session* s, const std::function<int()>& after_chunk, char* errbuf, size_t errlen) {
  for (;;) {
    int enq = 0;
    int rc = topolow_session_enqueue(s, 50, &enq, errbuf, errlen);
    if (rc || enq == 0) return rc;
    if (after_chunk && (rc = after_chunk()) != TOPOLOW_OK) return rc;
  }
}

int layout_route(int n, int ndim, const topolow_options& opt, LayoutRoute* r, char* errbuf, size_t errlen) {
  int schedule = opt.schedule;
  const int gs_max_n = opt.gs_max_n > 0 ? opt.gs_max_n : kDefaultGsMaxN;
  if (schedule == TOPOLOW_SCHEDULE_AUTO)
    schedule = (n <= gs_max_n && ndim <= kMaxTunedDim) ? TOPOLOW_SCHEDULE_GS : TOPOLOW_SCHEDULE_SLAB;
  if (schedule == TOPOLOW_SCHEDULE_GS) {
    if (const int rc = check_gs_dim(ndim, errbuf, errlen)) return rc;
  }

  // exact GS: one workgroup while the problem fits its LDS, the tile schedule beyond that
  const bool gs_fits_lds =
      gs_lds_bytes(n, kernel_dim(ndim), (opt.precision == TOPOLOW_PRECISION_F32) ? 4 : 8) <= 150 * 1024 && n <= 2048;
  r->schedule = schedule;
  r->tile_gs = schedule == TOPOLOW_SCHEDULE_GS && !gs_fits_lds;
  return TOPOLOW_OK;
}

// One embedding on a session, from session_create to session_finish: the slab schedule or tile Gauss-Seidel.  The
// body of topolow_optimize_layout_exact (its loader: the 16 arguments) and of topolow_layout_prep_optimize (its
// loader: the handle).  t_start: when the caller's entry began (stats->total_seconds, ->setup_seconds).
int run_session_layout(int32_t n, int32_t ndim, bool tile_gs, const topolow_options& opt, const SessionLoader& load,
                       const double* initial_positions, int32_t n_iter, double k0, double cooling_rate,
                       double c_repulsion, double relative_epsilon, int32_t convergence_window,
                       int32_t convergence_check_freq, int32_t verbose, double* positions_out, int32_t* converged,
                       int32_t* iterations, double* final_mae, double* final_k, topolow_run_stats* stats,
                       double t_start, char* errbuf, size_t errlen) {
  const int precision = opt.precision == TOPOLOW_PRECISION_AUTO
                            ? (tile_gs ? TOPOLOW_PRECISION_F64 : TOPOLOW_PRECISION_F32)
                            : opt.precision;
  topolow_session* s = nullptr;
  int rc = open_session(&s, n, ndim, tile_gs, precision, opt.device, opt.keep_labels ? nullptr : &opt.seed, load, errbuf, errlen);
  if (rc != TOPOLOW_OK) return rc;
  double t_dev0 = 0.0, t_dev1 = 0.0;
  int iters_run = 0, stopped = 0;
  double t_setup = 0.0;
  do {
    rc = topolow_session_set_positions(s, initial_positions, errbuf, errlen);
    if (rc) break;
    rc = topolow_session_begin(s, n_iter, k0, cooling_rate, c_repulsion, relative_epsilon,
                               convergence_window, convergence_check_freq, opt.seed,
                               opt.slab_stages, errbuf, errlen);
    if (rc) break;
    t_dev0 = now_s();
    t_setup = t_dev0 - t_start;
    if (verbose)
      emit_header(opt, tile_gs ? "tile Gauss-Seidel" : "row-owner slabs", n, k0, cooling_rate, c_repulsion);
    int reported = 0;
    std::vector<double> trace;
    auto report = [&] {   // verbose: the checks since the last report (waits for the enqueued work)
      int nc = 0;
      if (topolow_session_check_trace(s, nullptr, 0, &nc) != TOPOLOW_OK || nc <= reported) return;
      trace.resize(3 * (size_t)nc);
      if (topolow_session_check_trace(s, trace.data(), nc, &nc) != TOPOLOW_OK) return;
      emit_checks(opt, trace.data(), reported, nc, n_iter);
      reported = nc;
    };
    rc = enqueue_run(s, [&]() -> int {
      if (opt.interrupt_cb && opt.interrupt_cb(opt.interrupt_user)) {
        set_err(errbuf, errlen, "interrupted by the caller");
        return TOPOLOW_ERR_INTERRUPTED;
      }
      if (verbose) report();
      return TOPOLOW_OK;
    }, errbuf, errlen);
    if (rc == TOPOLOW_OK && verbose) report();
    if (rc) break;
    double last = 0.0;
    rc = topolow_session_sync(s, &iters_run, &stopped, &last, errbuf, errlen);
    if (rc) break;
    t_dev1 = now_s();
    rc = topolow_session_finish(s, positions_out, converged, iterations, final_mae, final_k,
                                errbuf, errlen);
  } while (0);
  if (rc == TOPOLOW_OK && stats) {
    std::memset(stats, 0, sizeof *stats);
    stats->schedule_used = tile_gs ? TOPOLOW_SCHEDULE_GS : TOPOLOW_SCHEDULE_SLAB;
    stats->precision_used = precision;
    stats->iterations_run = iters_run;
    stats->n_checks = s->mailbox->n_checks;
    stats->device_seconds = t_dev1 - t_dev0;
    stats->setup_seconds = t_setup;
    stats->stage_launches = s->stage_launches;
  }
  if (rc == TOPOLOW_OK && verbose && *converged)
    emit_converged(opt, s->mailbox->ctl.plateau >= s->mailbox->ctl.window, *iterations, *final_mae);
  topolow_session_destroy(s);
  if (rc == TOPOLOW_OK && stats) stats->total_seconds = now_s() - t_start;
  return rc;
}

extern "C" {

void topolow_default_options(topolow_options* opt) {
  if (!opt) return;
  std::memset(opt, 0, sizeof(*opt));
  opt->seed = 0;
  opt->schedule = TOPOLOW_SCHEDULE_AUTO;
  opt->precision = TOPOLOW_PRECISION_AUTO;
  opt->slab_stages = 0;
  opt->device = -1;
  opt->gs_max_n = 0;
  opt->keep_labels = 0;
  opt->interrupt_cb = nullptr;
  opt->interrupt_user = nullptr;
}

// ---- cross-validation folds from the host's cell list ----
int topolow_cell_list_index(int32_t n, int64_t n_cells, const int32_t* row, const int32_t* col,
                            int64_t* pos_of, int64_t* by_row, int64_t* row_ptr) {
  if (n < 1 || n_cells < 0 || !pos_of || !by_row || !row_ptr || (n_cells > 0 && (!row || !col)))
    return TOPOLOW_ERR_BAD_ARGUMENT;
  for (int64_t q = 0; q < (int64_t)n * n; ++q) pos_of[q] = -1;
  for (int i = 0; i <= n; ++i) row_ptr[i] = 0;
  for (int64_t c = 0; c < n_cells; ++c) {
    if (row[c] < 0 || row[c] >= n || col[c] < 0 || col[c] >= n) return TOPOLOW_ERR_BAD_ARGUMENT;
    pos_of[(int64_t)row[c] + (int64_t)col[c] * n] = c;   // linear column-major index, as R's which()
    row_ptr[row[c] + 1] += 1;
  }
  for (int i = 0; i < n; ++i) row_ptr[i + 1] += row_ptr[i];
  try {
    // counting sort by row; the listing is column-major, so columns ascend inside every row
    std::vector<int64_t> at(row_ptr, row_ptr + n);
    for (int64_t c = 0; c < n_cells; ++c) by_row[at[row[c]]++] = c;
  } catch (const std::bad_alloc&) {
    return TOPOLOW_ERR_HIP;
  }
  return TOPOLOW_OK;
}

int topolow_cv_fold(const topolow_cell_list* cells, const int64_t* picks, int64_t n_picks,
                    int32_t preserve_order, int32_t named, int32_t* order, int32_t* degrees,
                    int32_t* edge_i, int32_t* edge_j, double* edge_dist, int32_t* edge_thresh,
                    int64_t* n_edges, int32_t* holdout_i, int32_t* holdout_j, double* holdout_truth,
                    int64_t* n_holdout, double* numeric_max) {
  if (!cells || (!picks && n_picks > 0) || !order || !degrees || !edge_i || !edge_j || !edge_dist ||
      !edge_thresh || !n_edges || !holdout_i || !holdout_j || !holdout_truth || !n_holdout || !numeric_max)
    return TOPOLOW_ERR_BAD_ARGUMENT;
  try {
    return fold_problem(cells, picks, n_picks, preserve_order, named, order, degrees, edge_i, edge_j,
                        edge_dist, edge_thresh, n_edges, holdout_i, holdout_j, holdout_truth, n_holdout,
                        numeric_max);
  } catch (const std::bad_alloc&) {
    return TOPOLOW_ERR_HIP;
  }
}

// All folds of a cross-validation sweep in ONE call: the folds' problems are built side by side on host threads
// (fold_problem; start positions from the caller's unit draws with NumPy's / R's arithmetic: a random walk whose
// steps are uniform(0, 2 max / n), R/core.R:407-415) and relaxed as one batch; only the per-fold scores come back.
int topolow_cv_sweep(const topolow_cell_list* cells, int32_t named, int32_t preserve_order, int32_t n_folds,
                     const int32_t* ndim, const double* k0, const double* cooling_rate, const double* c_repulsion,
                     const int64_t* picks, const int64_t* picks_offset, const double* unit_draws,
                     const int64_t* draws_offset, const uint64_t* seeds, int32_t n_iter, double relative_epsilon,
                     int32_t convergence_window, int32_t convergence_check_freq, int32_t precision, int32_t device,
                     double* holdout_sum_abs, int64_t* holdout_count, int32_t* iterations, int32_t* converged,
                     int32_t* error_code, double* device_seconds, char* errbuf, size_t errlen) {
  if (!cv_sweep_args_ok(cells, n_folds, ndim, k0, cooling_rate, c_repulsion, picks_offset, unit_draws, draws_offset, seeds,
                        holdout_sum_abs, holdout_count, iterations, converged, error_code))
    return TOPOLOW_ERR_BAD_ARGUMENT;
  if (device_seconds) *device_seconds = 0.0;
  if (n_folds == 0) return TOPOLOW_OK;
  const int n = cells->n;
  const size_t m = (size_t)cells->n_cells;
  struct Fold {
    std::vector<int32_t> order, deg, ei, ej, et, hi, hj;
    std::vector<double> ed, ht, pos, out;
    int64_t ne = 0, nh = 0;
    int rc = TOPOLOW_OK;
  };
  std::vector<Fold> F;
  const int rc_folds = guarded(errbuf, errlen, [&] {
    F.resize((size_t)n_folds);
    host_parallel(n_folds, 16, [&](size_t lo, size_t hi) {
      for (size_t f = lo; f < hi; ++f) {
        Fold& x = F[f];
        x.order.resize(n); x.deg.resize(n);
        x.ei.resize(m); x.ej.resize(m); x.et.resize(m); x.ed.resize(m);
        x.hi.resize(m); x.hj.resize(m); x.ht.resize(m);
        double vmax = 0.0;
        x.rc = fold_problem(cells, picks + picks_offset[f], picks_offset[f + 1] - picks_offset[f], preserve_order, named,
                            x.order.data(), x.deg.data(), x.ei.data(), x.ej.data(), x.ed.data(), x.et.data(), &x.ne,
                            x.hi.data(), x.hj.data(), x.ht.data(), &x.nh, &vmax);
        x.rc = fold_check(x.rc, x.ne, vmax, ndim[f], draws_offset[f + 1] - draws_offset[f], n);
        if (x.rc != TOPOLOW_OK) continue;
        start_walk(unit_draws + draws_offset[f], vmax, n, ndim[f], nullptr, x.pos);
        x.out.assign((size_t)n * ndim[f], 0.0);
      }
    });
  });
  if (rc_folds != TOPOLOW_OK) return rc_folds;
  std::vector<topolow_problem> P;
  std::vector<topolow_result> R;
  std::vector<int> idx;
  for (int f = 0; f < n_folds; ++f) {
    Fold& x = F[(size_t)f];
    holdout_sum_abs[f] = 0.0; holdout_count[f] = 0; iterations[f] = 0; converged[f] = 0;
    error_code[f] = x.rc;
    if (x.rc != TOPOLOW_OK) continue;
    topolow_problem p;
    std::memset(&p, 0, sizeof p);
    p.initial_positions = x.pos.data();
    p.degrees = x.deg.data();
    p.edge_i = x.ei.data(); p.edge_j = x.ej.data(); p.edge_dist = x.ed.data(); p.edge_thresh = x.et.data();
    p.n_edges = x.ne; p.n = n; p.ndim = ndim[f]; p.n_iter = n_iter;
    p.convergence_window = convergence_window; p.convergence_check_freq = convergence_check_freq;
    p.k0 = k0[f]; p.cooling_rate = cooling_rate[f]; p.c_repulsion = c_repulsion[f]; p.relative_epsilon = relative_epsilon;
    p.seed = seeds[f];
    if (x.nh > 0) { p.holdout_i = x.hi.data(); p.holdout_j = x.hj.data(); p.holdout_truth = x.ht.data(); p.n_holdout = x.nh; }
    topolow_result r;
    std::memset(&r, 0, sizeof r);
    r.positions_out = x.out.data();
    P.push_back(p); R.push_back(r); idx.push_back(f);
  }
  if (P.empty()) return TOPOLOW_OK;
  const int rc = topolow_optimize_layout_exact_batch(P.data(), R.data(), (int32_t)P.size(), precision, device, device_seconds,
                                                     errbuf, errlen);
  if (rc != TOPOLOW_OK) return rc;
  for (size_t q = 0; q < idx.size(); ++q) {
    const int f = idx[q];
    error_code[f] = R[q].error_code;
    holdout_sum_abs[f] = R[q].holdout_sum_abs; holdout_count[f] = R[q].holdout_count;
    iterations[f] = R[q].iterations; converged[f] = R[q].converged;
  }
  return TOPOLOW_OK;
}

int topolow_cv_fold_pairs(const topolow_cell_list* cells, const int64_t* picks, int64_t n_picks, int32_t preserve_order,
                          int32_t named, int32_t* order, int32_t* degrees, double* numeric_max, int64_t* n_edges,
                          int32_t* pair_i, int32_t* pair_j, int64_t* n_pairs, int32_t* score_i, int32_t* score_j,
                          double* score_truth, int64_t* n_scored, char* errbuf, size_t errlen) {
  if (!cells || (!picks && n_picks > 0) || !order || !degrees || !numeric_max || !n_edges || !pair_i || !pair_j ||
      !n_pairs || !score_i || !score_j || !score_truth || !n_scored)
    return TOPOLOW_ERR_BAD_ARGUMENT;
  int rc = TOPOLOW_OK;
  const int rcg = guarded(errbuf, errlen, [&] {
    if (!fold_cells_symmetric(cells))
      throw HipError{TOPOLOW_ERR_UNSUPPORTED, kAsymmetricCells};
    FoldPairs fp;
    rc = fold_pairs(cells, picks, n_picks, preserve_order, named, fp);
    if (rc != TOPOLOW_OK) return;
    std::copy(fp.order.begin(), fp.order.end(), order);
    std::copy(fp.degrees.begin(), fp.degrees.end(), degrees);
    *numeric_max = fp.numeric_max;
    *n_edges = fp.n_edges;
    std::copy(fp.pair_i.begin(), fp.pair_i.end(), pair_i);
    std::copy(fp.pair_j.begin(), fp.pair_j.end(), pair_j);
    *n_pairs = (int64_t)fp.pair_i.size();
    std::copy(fp.score_i.begin(), fp.score_i.end(), score_i);
    std::copy(fp.score_j.begin(), fp.score_j.end(), score_j);
    std::copy(fp.score_truth.begin(), fp.score_truth.end(), score_truth);
    *n_scored = (int64_t)fp.score_i.size();
  });
  return rcg != TOPOLOW_OK ? rcg : rc;
}

int topolow_cv_sweep_session(const topolow_cell_list* cells, int32_t named, int32_t preserve_order, int32_t n_folds,
                             const int32_t* ndim, const double* k0, const double* cooling_rate, const double* c_repulsion,
                             const int64_t* picks, const int64_t* picks_offset, const double* unit_draws,
                             const int64_t* draws_offset, const uint64_t* seeds, int32_t n_iter, double relative_epsilon,
                             int32_t convergence_window, int32_t convergence_check_freq, int32_t precision, int32_t device,
                             int32_t schedule, double* holdout_sum_abs, int64_t* holdout_count, int32_t* iterations,
                             int32_t* converged, int32_t* error_code, double* device_seconds, char* errbuf, size_t errlen) {
  const SweepArgs a{named, preserve_order, n_folds, ndim, k0, cooling_rate, c_repulsion, picks, picks_offset, unit_draws,
                    draws_offset, seeds, n_iter, relative_epsilon, convergence_window, convergence_check_freq, precision,
                    schedule, holdout_sum_abs, holdout_count, iterations, converged, error_code, device_seconds};
  CellFolds src{cells, a, device};
  return cv_sweep_resident(cells, src, a, errbuf, errlen);
}

int topolow_optimize_layout_exact_sharded(
    const double* initial_positions, int32_t n, int32_t ndim, const double* dissimilarity_matrix,
    const int32_t* threshold_matrix, const int32_t* degrees, const int32_t* edge_i, const int32_t* edge_j,
    const double* edge_dist, const int32_t* edge_thresh, int64_t n_edges, int32_t n_iter, double k0,
    double cooling_rate, double c_repulsion, double relative_epsilon, int32_t convergence_window,
    int32_t convergence_check_freq, int32_t verbose, const topolow_options* opt_in, double* positions_out,
    int32_t* converged, int32_t* iterations, double* final_mae, double* final_k, topolow_shard_stats* stats,
    char* errbuf, size_t errlen) {
  if (n < 2) {  // reference :131
    set_err(errbuf, errlen, "Need at least 2 points for embedding");
    return TOPOLOW_ERR_TOO_FEW_POINTS;
  }
  if (!initial_positions || !degrees || !positions_out || !converged || !iterations || !final_mae || !final_k ||
      ((dissimilarity_matrix == nullptr) != (threshold_matrix == nullptr)) || n_edges < 0 ||
      (n_edges > 0 && (!edge_i || !edge_j || !edge_dist || !edge_thresh))) {
    set_err(errbuf, errlen, "null argument");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  topolow_options opt;
  if (opt_in) opt = *opt_in; else topolow_default_options(&opt);
  if (opt.schedule == TOPOLOW_SCHEDULE_GS) {
    set_err(errbuf, errlen, "the row-sharded path runs the slab schedule; exact Gauss-Seidel is a one-GPU schedule");
    return TOPOLOW_ERR_UNSUPPORTED;
  }
  if (opt.precision == TOPOLOW_PRECISION_F64_EXACT) {
    set_err(errbuf, errlen, "precision f64_exact: one GPU only (the row-sharded engine has no exact kernels)");
    return TOPOLOW_ERR_UNSUPPORTED;
  }
  const int want = opt.n_devices > 0 ? opt.n_devices : 1;
  const int blocks = topolow_shard_rows(n, want, -1, nullptr, nullptr);
  const int precision = opt.precision == TOPOLOW_PRECISION_F64 ? TOPOLOW_PRECISION_F64 : TOPOLOW_PRECISION_F32;
  const double t_start = now_s();
  std::vector<topolow_session*> ss(blocks, nullptr);
  int rc = TOPOLOW_OK;
  for (int b = 0; b < blocks && rc == TOPOLOW_OK; ++b) {
    int rb = 0, re = 0;
    topolow_shard_rows(n, want, b, &rb, &re);
    const int dev = opt.devices ? opt.devices[b % want] : (opt.n_devices > 1 ? b : opt.device);
    rc = topolow_session_create(&ss[b], n, ndim, rb, re, precision, dev, errbuf, errlen);
    if (rc) break;
    if (!opt.keep_labels) {   // every block draws the same permutation (same n, same seed)
      rc = topolow_session_set_relabel(ss[b], mix64(opt.seed ^ 0x1abe15eedull) | 1ull, errbuf, errlen);
      if (rc) break;
    }
    if (dissimilarity_matrix)
      rc = topolow_session_load_dense(ss[b], dissimilarity_matrix, threshold_matrix, degrees, errbuf, errlen);
    else
      rc = topolow_session_load_coo(ss[b], edge_i, edge_j, edge_dist, edge_thresh, n_edges, degrees, errbuf, errlen);
    if (rc) break;
    // this block's share of the convergence MAE: pair {lo, hi} belongs to the owner of lo when lo + hi
    // is even, of hi when it is odd (every block then reduces about half of its row block's pairs)
    try {
      std::vector<int32_t> bi, bj, bt;
      std::vector<double> bd;
      const int* inv = ss[b]->inv.empty() ? nullptr : ss[b]->inv.data();   // ownership is by session label
      for (int64_t e = 0; e < n_edges; ++e) {
        const int a = edge_i[e], c = edge_j[e];
        if (a < 0 || c < 0 || a >= n || c >= n) continue;
        const int sa = inv ? inv[a] : a, sc = inv ? inv[c] : c;
        const int lo = sa < sc ? sa : sc, hi = sa < sc ? sc : sa;
        const int owner = blocks == 1 ? lo : ((((lo + hi) & 1) == 0) ? lo : hi);
        if (owner >= rb && owner < re) { bi.push_back(a); bj.push_back(c); bd.push_back(edge_dist[e]); bt.push_back(edge_thresh[e]); }
      }
      rc = topolow_session_set_edges(ss[b], bi.data(), bj.data(), bd.data(), bt.data(), (int64_t)bi.size(), errbuf, errlen);
    } catch (const std::bad_alloc&) {
      set_err(errbuf, errlen, "out of host memory");
      rc = TOPOLOW_ERR_HIP;
    }
  }
  if (rc == TOPOLOW_OK) {
    if (verbose) {
      char what[64];
      snprintf(what, sizeof what, "row-owner slabs, %d row blocks", blocks);
      emit_header(opt, what, n, k0, cooling_rate, c_repulsion);
    }
    rc = topolow_sessions_run_sharded(ss.data(), blocks, initial_positions, n_iter, k0, cooling_rate, c_repulsion,
                                      relative_epsilon, convergence_window, convergence_check_freq, opt.seed,
                                      opt.slab_stages, opt.interrupt_cb, opt.interrupt_user, stats != nullptr,
                                      positions_out, converged, iterations, final_mae, final_k, stats, errbuf, errlen);
    if (rc == TOPOLOW_OK && verbose) {
      int nc = 0;
      if (topolow_session_check_trace(ss[0], nullptr, 0, &nc) == TOPOLOW_OK && nc > 0) {
        std::vector<double> trace(3 * (size_t)nc);
        if (topolow_session_check_trace(ss[0], trace.data(), nc, &nc) == TOPOLOW_OK)
          emit_checks(opt, trace.data(), 0, nc, n_iter);
      }
      if (*converged)
        emit_converged(opt, ss[0]->mailbox->ctl.plateau >= ss[0]->mailbox->ctl.window, *iterations, *final_mae);
    }
  }
  for (topolow_session* s : ss) topolow_session_destroy(s);
  if (rc == TOPOLOW_OK && stats) stats->total_seconds = now_s() - t_start;
  return rc;
}

// ---- the .Call payload -------------------------------------------------------------------
int topolow_optimize_layout_exact(
    const double* initial_positions, int32_t n, int32_t ndim,
    const double* dissimilarity_matrix, const int32_t* threshold_matrix,
    const int32_t* degrees, const int32_t* edge_i, const int32_t* edge_j,
    const double* edge_dist, const int32_t* edge_thresh, int64_t n_edges, int32_t n_iter,
    double k0, double cooling_rate, double c_repulsion, double relative_epsilon,
    int32_t convergence_window, int32_t convergence_check_freq, int32_t verbose,
    const topolow_options* opt_in, double* positions_out, int32_t* converged,
    int32_t* iterations, double* final_mae, double* final_k, topolow_run_stats* stats,
    char* errbuf, size_t errlen) {
  if (n < 2) {  // reference :131
    set_err(errbuf, errlen, "Need at least 2 points for embedding");
    return TOPOLOW_ERR_TOO_FEW_POINTS;
  }
  if (!initial_positions || !dissimilarity_matrix || !threshold_matrix || !degrees ||
      !positions_out || !converged || !iterations || !final_mae || !final_k ||
      (n_edges > 0 && (!edge_i || !edge_j || !edge_dist || !edge_thresh)) || n_edges < 0) {
    set_err(errbuf, errlen, "null argument");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  topolow_options opt;
  if (opt_in) opt = *opt_in; else topolow_default_options(&opt);
  const double t_start = now_s();
  if (opt.n_devices > 1 || opt.devices != nullptr) {   // ONE embedding over several GPUs / row blocks
    topolow_shard_stats sh;
    const int rcs = topolow_optimize_layout_exact_sharded(
        initial_positions, n, ndim, dissimilarity_matrix, threshold_matrix, degrees, edge_i, edge_j, edge_dist,
        edge_thresh, n_edges, n_iter, k0, cooling_rate, c_repulsion, relative_epsilon, convergence_window,
        convergence_check_freq, verbose, &opt, positions_out, converged, iterations, final_mae, final_k,
        stats ? &sh : nullptr, errbuf, errlen);
    if (rcs == TOPOLOW_OK && stats) {
      std::memset(stats, 0, sizeof *stats);
      stats->schedule_used = TOPOLOW_SCHEDULE_SLAB;
      stats->precision_used = opt.precision == TOPOLOW_PRECISION_F64 ? TOPOLOW_PRECISION_F64 : TOPOLOW_PRECISION_F32;
      stats->iterations_run = sh.iterations_run;
      stats->n_checks = sh.n_checks;
      stats->device_seconds = sh.loop_seconds;
      stats->total_seconds = sh.total_seconds;
      stats->stage_launches = sh.stage_launches;
    }
    return rcs;
  }

  LayoutRoute route;
  if (const int rcr = layout_route(n, ndim, opt, &route, errbuf, errlen)) return rcr;
  const int schedule = route.schedule;
  const bool tile_gs = route.tile_gs;
  if (schedule == TOPOLOW_SCHEDULE_GS && !tile_gs) {
    const int precision = opt.precision == TOPOLOW_PRECISION_AUTO ? TOPOLOW_PRECISION_F64 : opt.precision;
    topolow_problem pb;
    std::memset(&pb, 0, sizeof pb);
    pb.initial_positions = initial_positions; pb.n = n; pb.ndim = ndim;
    pb.dissimilarity_matrix = dissimilarity_matrix; pb.threshold_matrix = threshold_matrix; pb.degrees = degrees;
    pb.edge_i = edge_i; pb.edge_j = edge_j; pb.edge_dist = edge_dist; pb.edge_thresh = edge_thresh;
    pb.n_edges = n_edges; pb.n_iter = n_iter; pb.k0 = k0; pb.cooling_rate = cooling_rate;
    pb.c_repulsion = c_repulsion; pb.relative_epsilon = relative_epsilon; pb.convergence_window = convergence_window;
    pb.convergence_check_freq = convergence_check_freq; pb.seed = opt.seed;
    topolow_result res;
    std::memset(&res, 0, sizeof res);
    res.positions_out = positions_out;
    double dev_s = 0.0;
    std::vector<double> trace;
    if (verbose) emit_header(opt, "one-workgroup Gauss-Seidel", n, k0, cooling_rate, c_repulsion);
    const int rc = guarded(errbuf, errlen, [&] {
      select_device(opt.device);
      gs_relax_by_precision(precision, &pb, &res, 1, &dev_s, opt.interrupt_cb, opt.interrupt_user, verbose ? &trace : nullptr);
    });
    if (rc != TOPOLOW_OK) return rc;
    if (res.error_code == TOPOLOW_ERR_NONFINITE)
      set_err(errbuf, errlen, "Numerical instability at iteration %d. Reduce k0 or c_repulsion.", res.error_iteration);
    if (res.error_code == TOPOLOW_ERR_INTERRUPTED) set_err(errbuf, errlen, "interrupted by the caller");
    if (res.error_code != TOPOLOW_OK) return res.error_code;
    *converged = res.converged; *iterations = res.iterations; *final_mae = res.final_mae;
    *final_k = res.final_k;
    if (stats) {
      std::memset(stats, 0, sizeof *stats);
      stats->schedule_used = TOPOLOW_SCHEDULE_GS;
      stats->precision_used = precision;
      stats->iterations_run = res.iterations_run;
      stats->n_checks = res.n_checks;
      stats->device_seconds = dev_s;
      stats->total_seconds = now_s() - t_start;
    }
    if (verbose) {
      const int nc = (int)(trace.size() / 3);
      emit_checks(opt, trace.data(), 0, nc, n_iter);
      if (res.converged) {
        // the rule that stopped the run: the last `window` checks all lie inside the plateau band
        // (plateau) or above it (worsening); the last check decides
        const bool plateau = nc > 0 && trace[3 * (nc - 1) + 1] <= res.final_mae * (1.0 + relative_epsilon);
        emit_converged(opt, plateau, res.iterations, res.final_mae);
      }
    }
    return TOPOLOW_OK;
  }

  // ---- slab schedule, or exact tile Gauss-Seidel (same session, different iteration body) ----
  return run_session_layout(n, ndim, tile_gs, opt, [&](topolow_session* s, char* eb, size_t el) -> int {
    int rc = TOPOLOW_OK;
    // The 16 arguments carry the matrix twice: dense (800 + 400 MB at config 3) and as the list of its
    // measured upper-triangle cells (R/core.R:383-402 and :429-436 build both from one matrix).  When
    // the list is verified to BE the matrix, the encoded block is built from the list -- a quarter of
    // the bytes over PCIe -- and the dense arrays are only read on the host, once, to verify it.
    bool from_edges = false;
    if (s->precision == TOPOLOW_PRECISION_F32 && getenv("TOPOLOW_DENSE_UPLOAD") == nullptr &&
        edges_are_the_matrix(dissimilarity_matrix, threshold_matrix, n, edge_i, edge_j, edge_dist, edge_thresh, n_edges,
                             true)) {
      rc = topolow_session_load_coo(s, edge_i, edge_j, edge_dist, edge_thresh, n_edges, degrees, eb, el);
      if (rc) return rc;
      rc = topolow_session_set_edges(s, edge_i, edge_j, edge_dist, edge_thresh, n_edges, eb, el);
      if (rc) return rc;
      // the device-side fingerprint (count and hash of the block's measured cells == the list) rules
      // out what the host pass cannot see cheaply: a pair listed twice
      from_edges = topolow_session_uses_dense_mae(s) != 0;
    }
    if (!from_edges) {
      rc = topolow_session_load_dense(s, dissimilarity_matrix, threshold_matrix, degrees, eb, el);
      if (rc) return rc;
      rc = topolow_session_set_edges(s, edge_i, edge_j, edge_dist, edge_thresh, n_edges, eb, el);
      if (rc) return rc;
    }
    return rc;
  }, initial_positions, n_iter, k0, cooling_rate, c_repulsion, relative_epsilon, convergence_window,
  convergence_check_freq, verbose, positions_out, converged, iterations, final_mae, final_k, stats, t_start, errbuf, errlen);
}

}  // extern "C"
