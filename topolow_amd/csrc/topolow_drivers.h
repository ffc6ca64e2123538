// topolow_amd/csrc/topolow_drivers.h -- what the drivers in topolow_drivers.hip share with the entries of a prepared
// handle (topolow_prep.hip, topolow_prep_fold.hip): opening and running a whole-problem session, the route of an embedding, and the sweep
// over resident folds; and the one door to the one-workgroup Gauss-Seidel kernels (topolow_gs.hip).  Types,
// declarations and the one template; no kernels.
#pragma once

#include "topolow_session.h"

#pragma GCC visibility push(hidden)

// Targets, degrees and the convergence edge list into a fresh whole-problem session (relabelled already).
using SessionLoader = std::function<int(topolow_session*, char*, size_t)>;

// ---- defined in topolow_drivers.hip ----
bool cv_sweep_args_ok(const void* cells, int32_t n_folds, const int32_t* ndim, const double* k0,
                      const double* cooling_rate, const double* c_repulsion, const int64_t* picks_offset,
                      const double* unit_draws, const int64_t* draws_offset, const uint64_t* seeds,
                      const double* holdout_sum_abs, const int64_t* holdout_count, const int32_t* iterations,
                      const int32_t* converged, const int32_t* error_code);
int open_session(topolow_session** out, int32_t n, int32_t ndim, bool tile_gs, int32_t precision, int32_t device,
                 const uint64_t* relabel_seed, const SessionLoader& load, char* errbuf, size_t errlen);
int enqueue_run(topolow_session* s, const std::function<int()>& after_chunk, char* errbuf, size_t errlen);

// What both resident sweeps take, in the ORDER of their signatures: an entry fills it with its own parameter list.
struct SweepArgs {
  int32_t named, preserve_order, n_folds;
  const int32_t* ndim;
  const double *k0, *cooling_rate, *c_repulsion;
  const int64_t *picks, *picks_offset;
  const double* unit_draws;
  const int64_t* draws_offset;
  const uint64_t* seeds;
  int32_t n_iter;
  double relative_epsilon;
  int32_t convergence_window, convergence_check_freq, precision, schedule;
  double* holdout_sum_abs;
  int64_t* holdout_count;
  int32_t *iterations, *converged, *error_code;
  double* device_seconds;
};

// The sweep of topolow_cv_sweep on resident sessions, the loop of both entries: one session per ndim, loaded once with
// the full matrix (`matrix`: NULL is refused); a fold is held out of it, run, scored on the device and put back.  Where
// a fold comes from is its source's business (CellFolds: the host's cell list; HandleFolds: a prepared handle).  After
// the shared refusals begin() checks what only the source checks and sets n, device, degrees (the full matrix's, for
// the restore) and seconds (prepare, hold out, score, restore); load() fills a fresh session; prefetch(f) names the
// fold that prepare() is asked for next; prepare() returns fold f with its `code` (not OK: reported, not run) and `pos`
// (n x ndim start positions, column-major, caller's labels), or sets rc; drain() ends a group, in whichever way.
template <typename Folds>
int cv_sweep_resident(const void* matrix, Folds& src, const SweepArgs& a, char* errbuf, size_t errlen) {
  if (!cv_sweep_args_ok(matrix, a.n_folds, a.ndim, a.k0, a.cooling_rate, a.c_repulsion, a.picks_offset, a.unit_draws,
                        a.draws_offset, a.seeds, a.holdout_sum_abs, a.holdout_count, a.iterations, a.converged, a.error_code) ||
      (a.schedule != TOPOLOW_SCHEDULE_AUTO && a.schedule != TOPOLOW_SCHEDULE_SLAB && a.schedule != TOPOLOW_SCHEDULE_GS)) {
    set_err(errbuf, errlen, "null argument, n_folds < 0 or an unknown schedule");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (a.device_seconds) *a.device_seconds = 0.0;
  if (a.precision == TOPOLOW_PRECISION_F64_EXACT) {
    set_err(errbuf, errlen, "precision f64_exact: no cross-validation on resident sessions (holding a fold out does not "
            "cover the delta block); topolow_cv_sweep runs it on the one-workgroup kernel");
    return TOPOLOW_ERR_UNSUPPORTED;
  }
  if (a.n_folds == 0) return TOPOLOW_OK;
  if (const int rcb = src.begin(errbuf, errlen)) return rcb;
  const bool tile_gs = a.schedule == TOPOLOW_SCHEDULE_GS;
  const int prec = a.precision == TOPOLOW_PRECISION_AUTO ? (tile_gs ? TOPOLOW_PRECISION_F64 : TOPOLOW_PRECISION_F32) : a.precision;
  auto nothing = [&](int f) { a.holdout_sum_abs[f] = 0.0; a.holdout_count[f] = 0; a.iterations[f] = 0; a.converged[f] = 0; };
  for (int f = 0; f < a.n_folds; ++f) { nothing(f); a.error_code[f] = TOPOLOW_OK; }
  double* secs = src.seconds;
  secs[0] = secs[1] = secs[2] = secs[3] = 0.0;
  std::vector<char> done((size_t)a.n_folds, 0);
  for (int g0 = 0; g0 < a.n_folds; ++g0) {
    if (done[(size_t)g0]) continue;
    std::vector<int> members;   // the folds that share this ndim, in the caller's order
    for (int f = g0; f < a.n_folds; ++f)
      if (!done[(size_t)f] && a.ndim[f] == a.ndim[g0]) { members.push_back(f); done[(size_t)f] = 1; }
    if (a.ndim[g0] < 1) {
      for (int f : members) a.error_code[f] = TOPOLOW_ERR_BAD_ARGUMENT;
      continue;
    }
    src.prefetch(members[0]);
    topolow_session* s = nullptr;   // the labels are shuffled by the first fold's seed
    int rc = open_session(&s, src.n, a.ndim[g0], tile_gs, prec, src.device, &a.seeds[members[0]],
                          [&](topolow_session* t, char* eb, size_t el) -> int { return src.load(t, eb, el); }, errbuf, errlen);
    for (size_t q = 0; q < members.size() && rc == TOPOLOW_OK; ++q) {
      const int f = members[q];
      const double tp = now_s();
      auto fold = src.prepare(s, f, &rc, errbuf, errlen);
      secs[0] += now_s() - tp;
      if (q + 1 < members.size()) src.prefetch(members[q + 1]);
      if (rc != TOPOLOW_OK) break;   // (error_code[f] stays TOPOLOW_OK: the call fails, not the fold)
      a.error_code[f] = fold->code;
      if (fold->code != TOPOLOW_OK) continue;   // the session was not touched
      const double th = now_s();
      rc = src.hold_out(s, *fold, errbuf, errlen);
      secs[1] += now_s() - th;
      if (rc) break;
      const double t0 = now_s();
      int rcf = topolow_session_set_positions(s, fold->pos.data(), errbuf, errlen);
      if (rcf == TOPOLOW_OK)
        rcf = topolow_session_begin(s, a.n_iter, a.k0[f], a.cooling_rate[f], a.c_repulsion[f], a.relative_epsilon,
                                    a.convergence_window, a.convergence_check_freq, a.seeds[f], 0, errbuf, errlen);
      if (rcf == TOPOLOW_OK) rcf = enqueue_run(s, nullptr, errbuf, errlen);
      if (rcf == TOPOLOW_OK)
        rcf = topolow_session_finish(s, nullptr, &a.converged[f], &a.iterations[f], nullptr, nullptr, errbuf, errlen);
      else
        (void)topolow_session_finish(s, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0);   // the run is over either way
      if (a.device_seconds) *a.device_seconds += now_s() - t0;
      const double ts = now_s();
      if (rcf == TOPOLOW_OK) rcf = src.score(s, *fold, &a.holdout_sum_abs[f], &a.holdout_count[f], errbuf, errlen);
      secs[2] += now_s() - ts;
      // the session is the full matrix again before the next fold starts, whatever this one did
      const double tr = now_s();
      char rerr[256] = "";
      const int rcr = topolow_session_restore_held_out(s, src.degrees, rerr, sizeof rerr);
      secs[3] += now_s() - tr;
      if (rcf == TOPOLOW_ERR_NONFINITE) {   // a diverged fold is this fold's result, not the call's
        a.error_code[f] = TOPOLOW_ERR_NONFINITE;
        nothing(f);
        rcf = TOPOLOW_OK;
      }
      if (rcf != TOPOLOW_OK) { rc = rcf; break; }
      if (rcr != TOPOLOW_OK) { set_err(errbuf, errlen, "%s", rerr); rc = rcr; break; }
    }
    src.drain();
    if (s) topolow_session_destroy(s);
    if (rc != TOPOLOW_OK) return rc;
  }
  return TOPOLOW_OK;
}

// Which device path an embedding of n points in ndim dimensions takes under `opt`: the decision of
// topolow_optimize_layout_exact, shared with topolow_layout_prep_optimize.
struct LayoutRoute {
  int schedule = TOPOLOW_SCHEDULE_SLAB;   // AUTO resolved
  bool tile_gs = false;                   // schedule gs beyond one workgroup: the session runs tile Gauss-Seidel
};

int layout_route(int n, int ndim, const topolow_options& opt, LayoutRoute* r, char* errbuf, size_t errlen);
int run_session_layout(int32_t n, int32_t ndim, bool tile_gs, const topolow_options& opt, const SessionLoader& load,
                       const double* initial_positions, int32_t n_iter, double k0, double cooling_rate,
                       double c_repulsion, double relative_epsilon, int32_t convergence_window,
                       int32_t convergence_check_freq, int32_t verbose, double* positions_out, int32_t* converged,
                       int32_t* iterations, double* final_mae, double* final_k, topolow_run_stats* stats,
                       double t_start, char* errbuf, size_t errlen);

// ---- defined in topolow_gs.hip: gs_relax (relax_gs.h) in the precision asked for; see there ----
void gs_relax_by_precision(int32_t precision, const topolow_problem* problems, topolow_result* results, int32_t count,
                           double* device_seconds, int32_t (*interrupt_cb)(void*), void* interrupt_user,
                           std::vector<double>* trace_out);

#pragma GCC visibility pop
