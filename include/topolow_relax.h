/* include/topolow_relax.h -- C ABI of libtopolow_relax.so (MI355X / gfx950, HIP).
 *
 * Drop-in boundary for ONE path of omid-arhami/topolow v2.1.0: the native relaxation kernel
 * `optimize_layout_exact_cpp` (reference src/optimization.cpp:109-382) that
 * `euclidean_embedding()` reaches through
 *     .Call(`_topolow_optimize_layout_exact_cpp`, <16 args>)        (reference R/RcppExports.R:4-6,
 *                                                                    src/RcppExports.cpp:16-49)
 * plus the dense post-metric `as.matrix(dist(positions))` (reference R/core.R:474).
 *
 * Plain pointers and sizes only; no torch / R / C++ types.  Matrices are laid out as R lays
 * them out (column-major), so an R `.Call` shim or a ctypes/cgo/JNI stub can pass its buffers
 * straight through.  Every function returns 0 on success or a TOPOLOW_ERR_* code and writes a
 * message into errbuf (when given).  Inputs are never modified.
 */
#ifndef TOPOLOW_RELAX_H
#define TOPOLOW_RELAX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TOPOLOW_OK 0
#define TOPOLOW_ERR_TOO_FEW_POINTS 1 /* "Need at least 2 points for embedding" (reference :131) */
#define TOPOLOW_ERR_NONFINITE 2      /* "Numerical instability at iteration %d. ..." (:359-361) */
#define TOPOLOW_ERR_BAD_ARGUMENT 3
#define TOPOLOW_ERR_NO_DEVICE 4      /* no usable HIP device: there is NO CPU fallback */
#define TOPOLOW_ERR_HIP 5            /* a HIP runtime call failed; message has the call */
#define TOPOLOW_ERR_UNSUPPORTED 6
#define TOPOLOW_ERR_INTERRUPTED 7    /* the caller's interrupt callback asked to stop */

/* Parity statement.  The reference visits the pairs of an iteration in std::shuffle order seeded from
 * std::random_device (src/optimization.cpp:153-154,196): it cannot be reproduced run for run, its own test
 * accepts relative 1e-2 between two runs (tests/testthat/test-deprecated.R:65-67).  The CPU oracle the tests compare
 * with (oracle/, a restatement of src/optimization.cpp:109-382) is pinned by the results the reference itself ships
 * (tests/test_reference_results.py, data under tests/golden/ref_results/): the edge MAE of the reference's own H3N2
 * and HIV embeddings lies inside the oracle's 64-run distribution of the same call (0.59241 vs 0.58806 +- 0.0037;
 * 1.22454 vs 1.21109 +- 0.0121), those embeddings are rest points of the oracle's relaxation (error moves 0.05 %),
 * 3 x 48 likelihood_function() calls recorded in the reference's chains (H3N2, HIV, DENV) are reproduced to +1.3 % /
 * -0.2 % / +1.7 % in the mean (one call scatters by 1.5-2.4 %), its 20 per-fold CV errors to within 3 standard errors,
 * the mean, sd and quartiles of its pooled signed out-of-sample errors in sign and size.  What this library guarantees,
 * and tests (tests/test_gpu_contract.py against >= 20 oracle seeds per problem committed under tests/golden/;
 * tests/test_gpu_reference_results.py against the reference-held numbers directly):
 *   GS    the reference's arithmetic pair by pair in f64, in round-robin tournament order; the CPU oracle
 *         replaying that order agrees to <= 1e-12.  Final-MAE mean inside the oracle's
 *         mean +- max(3 sd, 1 %) on every pinned problem up to 1500 points and at config 3;
 *         stated band at N = 2048: 3 % (measured +1.8 % +- 0.6 %).
 *   SLAB  (AUTO above gs_max_n) the reference's per-pair update, applied row-owner style in Jacobi
 *         stages over random labels, fp32.  Final-MAE mean inside the oracle's
 *         mean +- max(3 sd, 1 %) on every pinned problem (N = 1500 ... 10 000, ndim 2 ... 5, thresholds,
 *         relative_epsilon 1e-4 ... 1e-10); run-to-run scatter: robust sd <= 2 sd_oracle + 0.5 %, at most 15 % of the runs
 *         further than max(4 sd_oracle, 3 %) from the oracle's mean (plain sd 0.9-1.8 x the oracle's, 3.3 x at
 *         N = 2048: DESIGN.md section 2b); the MAE it reports is the reference's edge MAE of the positions
 *         it returns to 2e-5; stop iteration within max(3 sd, 10 %) of the oracle's except on 2-D data
 *         (+55 %, same MAE).  Iterations that are ONE stage (k <= 3) of a problem with ndim 2..10 in fp32, 2..6 in f64,
 *         and >= 7168 points run as a symmetric sweep (csrc/relax_symm.h; fp32 ndim 7..10: csrc/relax_symm_wide.h, the
 *         same sweep with the lane's rows in LDS, same tests in tests/test_gpu_symmetric_wide.py and,
 *         on plans with long runs, tests/test_gpu_symmetric_wide_long_runs.py; at ndim 7..10
 *         it is on by default at ndim 7..10 -- where it measured faster than the row-owner kernel by more than the spread of
 *         repeated runs: at N = 10 000 (70 % missing) sweep + apply takes 68.8 / 71.3 / 76.1 / 82.4 us per iteration at ndim 7 / 8 / 9 / 10 against 96.0 / 107.4 / 108.7 / 116.0 us of the row-owner kernel, which ran these dims before (x1.40 / 1.51 / 1.43 / 1.41; with 15 % thresholds x1.69 / 1.75 / 1.71 / 1.66; spreads 5-12 us), so the >= 1.25x hoped for is met (profiles/r05_symm_wide.txt); TOPOLOW_SYMMETRIC=1 switches it on at every ndim it exists for): the same update -- every
 *         point moved by the sum of its own halves of all its pairs at the positions the previous iteration
 *         left -- with each pair's distance and factor computed once; checked against a CPU model of that
 *         iteration in f64 (positions: mean 5e-5, max 5e-3 of the displacement scale; the fused check's MAE against
 *         the oracle's edge error to 2e-5: tests/test_gpu_symmetric.py) and against the row-owner sweep (fp32
 *         summation order only: 2e-6 per iteration, same stop iteration and final MAE to 1e-6 on whole runs);
 *         a row-sharded run shards it over its sessions (same band against one block); f64 sessions take an f64 form
 *         of it (csrc/relax_symm64.h; equal to the f64 CPU model to 1e-12 per iteration; its fused check is exact --
 *         the sweep also reads exact-minus-rounded target differences -- and equals the reference's edge MAE to 1e-11);
 *         TOPOLOW_SYMMETRIC=0 / TOPOLOW_SHARD_SYMMETRIC=0 switch it off; TOPOLOW_SYMMETRIC=1 is not the same as leaving
 *         the variable unset: it also switches the sweep on at an ndim whose default is off (none at present).  Where the sweep applies, 2-, 4- and 8-stage
 *         iterations whose stages leave a resident wave >= 5 tiles (config 3: the two-stage ones, 3 < k <= 6) run as S
 *         symmetric sweeps that split the PAIRS -- stage st: the pairs between slabs a and b of the randomly labelled
 *         points with (a + b) mod S == st, stages in random order -- instead of "all points against one slab of the
 *         columns, S times": every point still meets one slab of partners per stage, both ends of a pair move together as
 *         in the reference; equal to a CPU model of that schedule (f64: 1e-12 per stage), final-MAE statistics unchanged
 *         on the pinned problems and seed for seed (profiles/r03_two_stage_study.txt); TOPOLOW_SYMMETRIC_TWO_STAGE=0
 *         keeps the row-owner form.  The fp32 sweep's waves run at an issue priority that falls with the share of
 *         their run still to do, so that the two waves of a SIMD end together (results unchanged bit for bit;
 *         TOPOLOW_SYM_PRIO=0 at session creation leaves every wave at priority 0; a sharded sweep's segments always do).
 *   F64 and F64_EXACT beyond one workgroup.  The session stores every target as a 4-byte word: fp32 rounded to 4 ulp,
 *         up to 3e-7 relative off the caller's f64 value.  With precision F64 positions, sums and the pair update are
 *         double, the convergence MAE is exact (f64 edge list; delta tiles in the fused check), but the FORCES come from
 *         the words: the result sits about 1e-7 of the displacement scale from what the caller's own targets give.  With
 *         precision F64_EXACT the session also keeps what the rounding took away, one fp32 delta per cell, and every
 *         kernel that runs reads target = word + delta, exact to 2e-14 relative: the row-owner stage kernel
 *         (csrc/relax_exact.h), the symmetric sweep and its multi-stage form (csrc/relax_symm64.h: symm64x_sweep_kernel)
 *         and tile Gauss-Seidel -- equal to the CPU model / the oracle fed the caller's UNROUNDED matrix in the bands
 *         the F64 tests hold against the rounded one (tests/test_gpu_exact_f64.py).  It costs 4 n ld more bytes of
 *         device memory and the time stated in DESIGN.md section 6.  The one-workgroup GS paths (small n, the batch,
 *         topolow_cv_sweep) read f64 targets at either value: there F64_EXACT is F64, reported back as asked.
 *         F64_EXACT answers TOPOLOW_ERR_UNSUPPORTED for: a row-block session (row_begin != 0 or row_end != n) and so
 *         every row-sharded path and a `devices` list; ndim > 16; topolow_session_commit_encoded (the caller's words
 *         carry no deltas); topolow_session_hold_out and topolow_cv_sweep_session (their patches do not cover the delta
 *         block).  F64 and AUTO are unchanged bit for bit.
 * The deterministic pieces -- controller, cooling, error rule, guards, messages -- are exact. */

/* Schedules (topolow_options.schedule). */
#define TOPOLOW_SCHEDULE_AUTO 0   /* GS tournament for n <= gs_max_n, slab above */
#define TOPOLOW_SCHEDULE_SLAB 1   /* S-stage row-owner slabs, HBM-bound, multi-workgroup */
#define TOPOLOW_SCHEDULE_GS 2     /* exact Gauss-Seidel, round-robin tournament order, one workgroup */

/* Arithmetic of positions and pair updates (topolow_options.precision). */
#define TOPOLOW_PRECISION_AUTO 0  /* f64 for the GS kernel, f32 for the slab kernel */
#define TOPOLOW_PRECISION_F32 1
#define TOPOLOW_PRECISION_F64 2
#define TOPOLOW_PRECISION_F64_EXACT 3  /* F64 with every target read as word + delta (2e-14 relative): see the parity statement */

typedef struct topolow_options {
  uint64_t seed;        /* seeds the pair-order / slab-order stream (the reference uses
                           std::random_device, src/optimization.cpp:153-154) */
  int32_t schedule;     /* TOPOLOW_SCHEDULE_* */
  int32_t precision;    /* TOPOLOW_PRECISION_* */
  int32_t slab_stages;  /* 0 = adaptive: topolow_slab_stages_at(iteration, k, ndim) */
  int32_t device;       /* HIP device ordinal; -1 = current device */
  int32_t gs_max_n;     /* AUTO switches to the slab schedule above this n; 0 = default */
  int32_t n_devices;    /* > 1 (or a non-NULL `devices`): ONE embedding row-block sharded over
                           devices[0..n_devices) -- see topolow_optimize_layout_exact_sharded */
  int32_t keep_labels;  /* 0 (default): the multi-workgroup schedules relabel the points at random (seeded
                           by `seed`), so that a slab / a tile is a random subset of the points rather
                           than a run of consecutive ones; non-zero: keep the caller's order */
  int32_t reserved[3];
  /* Polled every 50 iterations like Rcpp::checkUserInterrupt() in the reference
   * (src/optimization.cpp:364); a non-zero return abandons the run with TOPOLOW_ERR_INTERRUPTED
   * after device memory has been released.  NULL = never. */
  int32_t (*interrupt_cb)(void* user);
  void* interrupt_user;
  /* Sink of the `verbose` lines (the reference prints them with Rcpp::Rcout,
   * src/optimization.cpp:183-188,298-301,334-336,351-353): called with one NUL-terminated line
   * (newline included) at a time, on the calling thread.  NULL = stdout.  The R shim maps it to
   * Rprintf so the lines obey sink() and the console. */
  void (*print_cb)(const char* line, void* user);
  void* print_user;
  const int32_t* devices;   /* n_devices HIP ordinals; an ordinal may repeat (several row blocks on
                               one GPU).  NULL with n_devices > 1: ordinals 0..n_devices-1 */
} topolow_options;

/* Run statistics, filled by topolow_optimize_layout_exact when `stats` is non-NULL. */
typedef struct topolow_run_stats {
  int32_t schedule_used;
  int32_t precision_used;
  int32_t iterations_run;   /* iterations executed before stopping (>= `iterations` out) */
  int32_t n_checks;
  double  device_seconds;   /* relaxation loop only, device resident */
  double  total_seconds;    /* including upload/encode/download */
  int64_t stage_launches;
  double  setup_seconds;    /* session creation, verification of the inputs, upload, encode */
  int64_t reserved[3];
} topolow_run_stats;

void topolow_default_options(topolow_options* opt);

/* Replaces the payload of `_topolow_optimize_layout_exact_cpp` (reference
 * src/RcppExports.cpp:16-39 -> src/optimization.cpp:109-126), argument for argument:
 *   initial_positions     n x ndim  float64, column-major           (NumericMatrix)
 *   dissimilarity_matrix  n x n     float64, column-major, +Inf = unmeasured, symmetric
 *   threshold_matrix      n x n     int32,   column-major, 0 exact / 1 ">" / -1 "<"
 *   degrees               n         int32    (non-NA cells per row, R/core.R:341)
 *   edge_i, edge_j        n_edges   int32, 0-based, i<j   } upper-triangle measured pairs,
 *   edge_dist             n_edges   float64               } used by the convergence MAE only
 *   edge_thresh           n_edges   int32                 } (src/optimization.cpp:54-81)
 *   n_iter, k0, cooling_rate, c_repulsion, relative_epsilon, convergence_window,
 *   convergence_check_freq, verbose  -- as in the reference.
 * Outputs (the reference's returned list, src/optimization.cpp:375-381):
 *   positions_out n x ndim float64 column-major; converged (0/1); iterations (= best
 *   iteration); final_mae (= best MAE); final_k (= k at the best iteration).
 * opt may be NULL (defaults).  stats may be NULL.
 */
int topolow_optimize_layout_exact(
    const double* initial_positions, int32_t n, int32_t ndim,
    const double* dissimilarity_matrix, const int32_t* threshold_matrix,
    const int32_t* degrees,
    const int32_t* edge_i, const int32_t* edge_j, const double* edge_dist,
    const int32_t* edge_thresh, int64_t n_edges,
    int32_t n_iter, double k0, double cooling_rate, double c_repulsion,
    double relative_epsilon, int32_t convergence_window, int32_t convergence_check_freq,
    int32_t verbose, const topolow_options* opt,
    double* positions_out, int32_t* converged, int32_t* iterations, double* final_mae,
    double* final_k, topolow_run_stats* stats, char* errbuf, size_t errlen);

/* Batch form: `count` independent embeddings in one call -- one workgroup per embedding on the
 * exact Gauss-Seidel kernel (the reference's only parallel mode is one embedding per forked
 * process: R/adaptive_sampling.R:666,1301; its CV evaluator `likelihood_function`,
 * R/adaptive_sampling.R:2552-2726, runs `folds` such embeddings per parameter set).  Problems may
 * differ in every field, ndim included.  A problem that fails (e.g. non-finite positions) gets
 * its own error_code / message-free status; the call itself still returns TOPOLOW_OK. */
typedef struct topolow_problem {
  const double* initial_positions;     /* n x ndim, column-major */
  const double* dissimilarity_matrix;  /* n x n, +Inf = unmeasured; NULL together with           */
  const int32_t* threshold_matrix;     /* n x n   threshold_matrix: the edge list IS the matrix   */
  const int32_t* degrees;              /* n */
  const int32_t* edge_i;
  const int32_t* edge_j;
  const double* edge_dist;
  const int32_t* edge_thresh;
  int64_t n_edges;
  int32_t n, ndim, n_iter, convergence_window, convergence_check_freq, reserved0;
  double k0, cooling_rate, c_repulsion, relative_epsilon;
  uint64_t seed;
  /* Optional held-out pairs (0-based, any orientation) with their true dissimilarities: scored on
   * the returned positions, sum |truth - distance| -- the OutSampleError of the reference's
   * error_calculator_comparison (R/error_metrics.R:55-144) without materialising est_distances. */
  const int32_t* holdout_i;
  const int32_t* holdout_j;
  const double* holdout_truth;
  int64_t n_holdout;
} topolow_problem;

typedef struct topolow_result {
  double* positions_out;               /* n x ndim, column-major, caller-allocated */
  double final_mae, final_k;
  int32_t converged, iterations, iterations_run, n_checks;
  int32_t error_code;                  /* TOPOLOW_OK or TOPOLOW_ERR_NONFINITE */
  int32_t error_iteration;             /* iteration reported by the non-finite guard */
  double holdout_sum_abs;              /* sum |truth - distance| over the holdout pairs */
  int64_t holdout_count;
} topolow_result;

int topolow_optimize_layout_exact_batch(const topolow_problem* problems, topolow_result* results,
                                        int32_t count, int32_t precision, int32_t device,
                                        double* device_seconds, char* errbuf, size_t errlen);

/* Host-side helper of the batched CV evaluator: one fold's problem from the list of the full
 * matrix's non-NA cells, i.e. what the reference obtains per fold by masking the held-out cells
 * (R/adaptive_sampling.R:2600-2640) and re-running euclidean_embedding's pre-processing
 * (R/core.R:269-436) on the n x n matrix.  No device work.  Cells are listed in column-major order
 * (as R's which()); `pos_of` maps a linear column-major index to its cell or -1; `by_row`/`row_ptr`
 * list the same cells row by row (columns ascending).  `picks`: held-out linear indices (their
 * mirrors are held out too).  Outputs are caller-allocated: order n (order[0] = -1: input order
 * kept), degrees n, edges and holdout up to n_cells entries; `numeric_max` = largest value among the
 * remaining unprefixed cells (the scale of the random-walk start, R/core.R:407-415). */
typedef struct topolow_cell_list {
  int32_t n, reserved;
  int64_t n_cells;
  const int32_t* row;
  const int32_t* col;
  const double* value;      /* threshold prefix stripped */
  const int32_t* code;      /* 0 none, 1 ">", -1 "<" */
  const int64_t* pos_of;    /* n * n */
  const int64_t* by_row;    /* n_cells */
  const int64_t* row_ptr;   /* n + 1 */
} topolow_cell_list;

/* Fills the index arrays of a cell list from its (row, col) columns, listed in column-major order:
 * pos_of (n*n, -1 where no cell), by_row (n_cells), row_ptr (n+1).  No device work. */
int topolow_cell_list_index(int32_t n, int64_t n_cells, const int32_t* row, const int32_t* col,
                            int64_t* pos_of, int64_t* by_row, int64_t* row_ptr);

int topolow_cv_fold(const topolow_cell_list* cells, const int64_t* picks, int64_t n_picks,
                    int32_t preserve_order, int32_t named, int32_t* order, int32_t* degrees,
                    int32_t* edge_i, int32_t* edge_j, double* edge_dist, int32_t* edge_thresh,
                    int64_t* n_edges, int32_t* holdout_i, int32_t* holdout_j, double* holdout_truth,
                    int64_t* n_holdout, double* numeric_max);

/* A whole cross-validation sweep in one call (the consumer of the hot path: the reference's likelihood_function,
 * R/adaptive_sampling.R:2552-2726, folds x parameter sets times).  Fold f holds out the cells picks[picks_offset[f] ..
 * picks_offset[f + 1]) (linear column-major indices, as topolow_cv_fold) and runs with ndim[f], k0[f], ...; its start
 * positions are the reference's random walk (R/core.R:407-415) built from unit_draws[draws_offset[f] ..], the
 * ndim[f] x (n - 1) uniform(0, 1) numbers, row-major, that the caller drew at this point of its stream.  The folds'
 * problems are built on host threads and relaxed as ONE batch (topolow_optimize_layout_exact_batch); per fold only
 * the out-of-sample score comes back: sum |truth - distance| and count over its held-out numeric cells, the best
 * iteration and the converged flag; error_code[f] = TOPOLOW_ERR_BAD_ARGUMENT for a fold without valid measurements,
 * TOPOLOW_ERR_NONFINITE for a diverged one. */
int topolow_cv_sweep(const topolow_cell_list* cells, int32_t named, int32_t preserve_order, int32_t n_folds,
                     const int32_t* ndim, const double* k0, const double* cooling_rate, const double* c_repulsion,
                     const int64_t* picks, const int64_t* picks_offset, const double* unit_draws,
                     const int64_t* draws_offset, const uint64_t* seeds, int32_t n_iter, double relative_epsilon,
                     int32_t convergence_window, int32_t convergence_check_freq, int32_t precision, int32_t device,
                     double* holdout_sum_abs, int64_t* holdout_count, int32_t* iterations, int32_t* converged,
                     int32_t* error_code, double* device_seconds, char* errbuf, size_t errlen);


/* 1 when a problem of n points in ndim dimensions with n_edges measured pairs fits the one-workgroup kernel of
 * topolow_optimize_layout_exact_batch / topolow_cv_sweep (its LDS: 160 KB; about 2 900 points in f64 at ndim 5), 0 when
 * those calls would answer TOPOLOW_ERR_UNSUPPORTED -- the problems topolow_cv_sweep_session is for.  precision AUTO = f64,
 * as in the batch call.  Host only. */
int32_t topolow_batch_problem_fits(int32_t n, int32_t ndim, int32_t precision, int64_t n_edges);

/* topolow_cv_fold without the fold's edge list, for folds that are held out of a resident session
 * (topolow_session_hold_out): the same fold -- same ordering, degrees, numeric_max, scored cells -- with every index in
 * the CALLER's labels and host memory O(n + picks):
 *   order        n entries as topolow_cv_fold (order[0] = -1: input order kept); the fold's start positions are laid out
 *                along it: point i of the random walk is the caller's point order[i]
 *   degrees      n entries per CALLER's point (topolow_cv_fold's degrees[q] is the degree of point order[q])
 *   n_edges      measured upper-triangle cells the fold keeps (0: no valid measurements)
 *   pair_i/_j    the unique held-out unordered pairs, i < j (up to n_picks entries)
 *   score_i/_j/_truth  the scored cells: held out AND numeric, each non-NA mirror on its own (up to 2 n_picks entries);
 *                an unnamed matrix is scored in the returned numbering (R/error_metrics.R:100-112), i.e. cell (r, c)
 *                against the points order[r], order[c]
 * The cell list must be symmetric -- every off-diagonal cell has its mirror with the same value and code; with
 * asymmetric NA the reference reads the upper triangle of the per-fold reordered matrix, which one fixed block cannot
 * represent: TOPOLOW_ERR_UNSUPPORTED.  No device work. */
int topolow_cv_fold_pairs(const topolow_cell_list* cells, const int64_t* picks, int64_t n_picks, int32_t preserve_order,
                          int32_t named, int32_t* order, int32_t* degrees, double* numeric_max, int64_t* n_edges,
                          int32_t* pair_i, int32_t* pair_j, int64_t* n_pairs, int32_t* score_i, int32_t* score_j,
                          double* score_truth, int64_t* n_scored, char* errbuf, size_t errlen);

/* topolow_cv_sweep for problems beyond one workgroup: arguments and outputs as topolow_cv_sweep, plus `schedule`
 * (TOPOLOW_SCHEDULE_AUTO / _SLAB: the slab schedule; _GS: the tile Gauss-Seidel schedule of topolow_session_set_schedule;
 * precision AUTO: f32 for slab, f64 for GS, as the one-shot call).  The folds are grouped by ndim; a group shares ONE
 * device-resident session, relabelled as the one-shot call does (from the group's first seed) and loaded once with the
 * full matrix (the upper triangle of the cell list, which must be symmetric: see topolow_cv_fold_pairs).  Per fold:
 * topolow_session_hold_out, start positions from unit_draws (topolow_cv_sweep's arithmetic, laid out along the fold's
 * order), begin(seeds[f]), the run, finish without a download, topolow_session_score_pairs, restore -- the next fold is
 * prepared on a host thread meanwhile, host memory per fold O(n + picks).  error_code[f] as topolow_cv_sweep; the
 * session is the full matrix again before the next fold starts in every case. */
int topolow_cv_sweep_session(const topolow_cell_list* cells, int32_t named, int32_t preserve_order, int32_t n_folds,
                             const int32_t* ndim, const double* k0, const double* cooling_rate, const double* c_repulsion,
                             const int64_t* picks, const int64_t* picks_offset, const double* unit_draws,
                             const int64_t* draws_offset, const uint64_t* seeds, int32_t n_iter, double relative_epsilon,
                             int32_t convergence_window, int32_t convergence_check_freq, int32_t precision, int32_t device,
                             int32_t schedule, double* holdout_sum_abs, int64_t* holdout_count, int32_t* iterations,
                             int32_t* converged, int32_t* error_code, double* device_seconds, char* errbuf, size_t errlen);

/* Replaces `as.matrix(stats::dist(positions))` (reference R/core.R:474):
 * positions n x ndim float64 column-major (host) -> est_distances n x n float64 (host). */
int topolow_est_distances(const double* positions, int32_t n, int32_t ndim,
                          double* est_distances, int32_t device, char* errbuf, size_t errlen);
/* Rows [row_begin, row_end) of the same matrix: out is (row_end - row_begin) x n, row-major (= rows
 * row_begin.. of the symmetric n x n result).  For problems whose n x n float64 result should not be
 * held at once (BASELINE config 4: 20 GB): the caller streams row blocks.  Either entry keeps device
 * memory bounded (tiles of <= 256 MB). */
int topolow_est_distances_rows(const double* positions, int32_t n, int32_t ndim, int32_t row_begin,
                               int32_t row_end, double* out, int32_t device, char* errbuf, size_t errlen);

/* Replaces the reference's post-processing (R/core.R:474-481) in one pass over the device:
 * est_distances = as.matrix(dist(positions)) and the two terms of mae = mean(|as.numeric(D) - est|).
 *   positions      n x ndim f64 column-major (host), any ndim >= 1
 *   values         n x n f64 column-major (host)
 *   codes          n x n i32 column-major (host), or NULL
 *   est_distances  n x n f64 out (host), or NULL: not wanted.  Bit-identical to topolow_est_distances.
 * A cell counts iff values[cell] is finite (not NaN, not +-Inf) and (codes == NULL or codes[cell] == 0); the
 * diagonal counts like any other cell.  So the same rule reads both forms of the input: as.numeric(D) with NaN
 * for NA and for threshold strings and codes = NULL, or the matrices of the 16-argument call (+Inf = unmeasured,
 * threshold_mask as codes).
 *   *sum_abs = sum over the counting cells of |values[i,j] - ||p_i - p_j|||,  *count = their number.
 * mae = sum_abs / count is the caller's division (count 0: R's mean of nothing, NaN).  Non-finite positions
 * propagate: sum_abs is NaN.
 * The sum is reproducible: one partial per column, reduced in a fixed order on the device, the columns added in
 * index order on the host -- the same bits whatever the tile size, and whether or not est_distances is asked for.
 * The matrices travel in tiles of columns (device buffers and pinned memory bounded, uploads, kernels and
 * downloads overlapped); TOPOLOW_POST_TILE_COLS=<c> in the environment caps the columns per tile (a test knob,
 * read per call).
 * TOPOLOW_ERR_BAD_ARGUMENT, before any device call: NULL positions, values, sum_abs or count; n < 1; ndim < 1. */
int topolow_post_metrics(const double* positions, int32_t n, int32_t ndim, const double* values,
                         const int32_t* codes, double* est_distances, double* sum_abs, int64_t* count,
                         int32_t device, char* errbuf, size_t errlen);

/* How topolow_post_metrics_ex reaches the caller's pageable matrices. */
#define TOPOLOW_POST_STAGING_DEFAULT 0   /* what topolow_post_metrics uses */
#define TOPOLOW_POST_STAGING_PINNED 1    /* through pinned staging buffers that host threads fill and drain */
#define TOPOLOW_POST_STAGING_REGISTER 2  /* hipHostRegister on the caller's matrices for the length of the call */
#define TOPOLOW_POST_STAGING_PAGEABLE 3  /* asynchronous copies on the pageable memory as it is */

/* The same call with the staging chosen by the caller and the time of each phase measured (a study entry:
 * tests/study/post_metrics_timing.py).  phase_seconds: NULL, or 3 doubles out -- the sums over all tiles of the
 * host-to-device copies, the kernels and the device-to-host copies, from device events (the phases overlap, so
 * they do not add up to the call's wall-clock time).  Every staging computes the same bits. */
int topolow_post_metrics_ex(const double* positions, int32_t n, int32_t ndim, const double* values,
                            const int32_t* codes, double* est_distances, double* sum_abs, int64_t* count,
                            int32_t device, int32_t staging, double* phase_seconds, char* errbuf, size_t errlen);

/* Replaces the reference's compute_kernel_velocity (R/visualization.R:802-843): the kernel-weighted antigenic
 * velocity of every point of a finished map, one pairwise pass on the device, all of it in f64.
 *   positions      n x ndim f64 column-major (host), 1 <= ndim <= 16
 *   times          n f64 (host); NaN = NA
 *   sigma_t, sigma_x   the bandwidths of the temporal and of the spatial Gaussian kernel
 *   excluded_bits  NULL: every earlier point is eligible.  Else n rows of ceil(n / 64) 64-bit words, row-major, in the
 *                  caller's order: bit (j % 64) of word (j / 64) of row i set = point j does not contribute to row i.
 *                  The reference's clade rule (:816-823) sets it when i has an entry in clade_members, j is in
 *                  tree_present_points and j is not in i's clade; any dictionary of member lists is so represented
 *                  exactly.  Bits of later or tied points are never read.
 *   velocity       n x ndim f64 out, column-major;  weight_sum  n f64 out, or NULL: not wanted
 * For row i over the points j with times[j] < times[i] (strictly: a tie contributes in neither direction; a NaN
 * time is nobody's past and has none) whose bit is clear:
 *   w_ij = exp(-(||x_i - x_j||^2 / (2 sigma_x^2) + (t_i - t_j)^2 / (2 sigma_t^2)))
 *   weight_sum[i] = sum_j w_ij      velocity[i, d] = sum_j w_ij (x_id - x_jd) / (t_i - t_j) / weight_sum[i]
 * and velocity[i, ] = NaN (R's NA) when weight_sum[i] is not > 0: no eligible past point, or every weight 0.
 * One exp of the summed exponent replaces the reference's product of two: the two agree to a few ulp of a weight,
 * and can differ on whether a weight is exactly 0 only where the summed exponent lies between about 700 and 760.
 * The library sorts the points by time (stable; points of equal time by their coordinates) and permutes the bits
 * itself; everything is taken and returned in the caller's order.  The result is reproducible: no floating-point
 * atomic, every row's sums formed in an order that depends on n alone (columns in ascending sorted order inside
 * chunks of columns, the chunks' partials added in chunk order; the chunk is 256 columns up to 16 384 points and
 * n / 64 rounded up to a multiple of 256 beyond), so every call returns the same bits, and a point's row does not
 * depend on the order the caller lists the points in -- with one exception: points that are equal in time AND in
 * every coordinate keep the caller's order among themselves.  They add equal terms, so without bits nothing
 * changes; with exclusion bits that differ between such twins, a row that takes one twin and not the other may add
 * that term at another place in the order, and its last bits may then follow the caller's order.
 * Host cost of the bits: the library permutes the bits of every row's past to the sorted order one bit at a time,
 * about n^2 / 2 single-bit moves over up to 16 host threads (5 * 10^7 at 10 000 points, 1.25 * 10^9 at 50 000), and
 * holds a second copy of the n^2 / 8 bytes (313 MB at 50 000).
 * TOPOLOW_ERR_BAD_ARGUMENT, before any device call: NULL positions, times or velocity; n < 1; ndim < 1; a sigma
 * that is not finite or not > 0.  TOPOLOW_ERR_UNSUPPORTED: ndim > 16. */
int topolow_kernel_velocity(const double* positions, const double* times, int32_t n, int32_t ndim, double sigma_t,
                            double sigma_x, const uint64_t* excluded_bits, double* velocity, double* weight_sum,
                            int32_t device, char* errbuf, size_t errlen);

/* The same call with the columns per chunk chosen by the caller and the device time measured (a test and study
 * entry: tests/study/velocity_timing.py).  chunk_cols: 0 = the library's width, else a positive multiple of 64
 * (anything else: TOPOLOW_ERR_BAD_ARGUMENT).  Two widths group a row's additions differently, so their results may
 * differ in the last bits; one width always returns the same bits.  seconds: NULL, or 1 double out -- the two
 * kernels from device events (the host's sort, the uploads and the downloads are not in it). */
int topolow_kernel_velocity_ex(const double* positions, const double* times, int32_t n, int32_t ndim, double sigma_t,
                               double sigma_x, const uint64_t* excluded_bits, double* velocity, double* weight_sum,
                               int32_t device, int32_t chunk_cols, double* seconds, char* errbuf, size_t errlen);

/* Replaces the two n x n distance matrices and the objective of the reference's scale_to_original_distances
 * (R/visualization.R:624-640), the scale = TRUE step of reduce_dimensions: one pairwise pass on the device over the
 * coordinates themselves, all of it in f64.
 *   positions   n x ndim f64 column-major (host), 1 <= ndim <= 16: the map
 *   reduced     n x k f64 column-major (host), 1 <= k <= ndim: its plot coordinates (the PCA scores)
 *   scales      m f64, 1 <= m <= 8: all m are evaluated in the one pass (they share the square roots)
 *   objective   m f64 out;  sum_orig, sum_reduced  1 f64 out each, or NULL: not wanted
 * With d_ij = ||x_i - x_j|| and r_ij = ||y_i - y_j||:
 *   objective[q] = sum_{i != j} |d_ij - scales[q] r_ij|     sum_orig = sum_{i != j} d_ij     sum_reduced = sum_{i != j} r_ij
 * -- the reference's sums over the full matrices (the diagonal adds 0).  Only the pairs j < i are visited and the
 * sums doubled, which is exact; a pair's term is |fma(-s, r, d)|.  The result is reproducible: no floating-point
 * atomic; a row's terms are added in ascending column order inside units of 256 rows by chunk_cols columns, the rows
 * of a unit by a fixed tree, the units in a fixed order -- an order that depends on n and the chunk alone (256
 * columns up to 16 384 points, n / 64 rounded up to a multiple of 256 beyond), so every call returns the same bits,
 * and a call with m scales returns the bits of m calls with one.
 * TOPOLOW_ERR_BAD_ARGUMENT, before any device call: NULL positions, reduced, scales or objective; n < 2; k < 1 or
 * k > ndim; m outside 1..8; a scale or a coordinate that is not finite (the reference's optimize fails on one).
 * TOPOLOW_ERR_UNSUPPORTED: ndim > 16. */
int topolow_scale_objective(const double* positions, const double* reduced, int32_t n, int32_t ndim, int32_t k,
                            const double* scales, int32_t m, double* objective, double* sum_orig, double* sum_reduced,
                            int32_t device, char* errbuf, size_t errlen);

/* The same call with the columns per unit chosen by the caller and the device time measured (a test and study
 * entry: tests/study/reduce_timing.py).  chunk_cols: 0 = the library's width, else 64, 128, 256 or 512 (anything
 * else: TOPOLOW_ERR_BAD_ARGUMENT).  Two widths group the additions differently, so their results may differ in the
 * last bits; one width always returns the same bits.  seconds: NULL, or 1 double out -- the two kernels from device
 * events (the uploads and the download are not in it). */
int topolow_scale_objective_ex(const double* positions, const double* reduced, int32_t n, int32_t ndim, int32_t k,
                               const double* scales, int32_t m, double* objective, double* sum_orig, double* sum_reduced,
                               int32_t device, int32_t chunk_cols, double* seconds, char* errbuf, size_t errlen);

/* The reference's scale_to_original_distances: the scale s in [lower, upper] that minimises objective(s) above.
 * positions and reduced are uploaded once; Brent's fmin -- the algorithm behind R's optimize: golden section with
 * parabolic steps, eps = sqrt(DBL_EPSILON), tol1 = eps |x| + tol / 3 -- runs on the host inside the library, every
 * evaluation one launch pair with one scale.  (The reference calls optimize on [0.01, 40] with R's default tol,
 * DBL_EPSILON^0.25.)
 *   scale        1 f64 out: the minimiser;  objective  1 f64 out, or NULL: its objective, the smallest one evaluated
 *   evaluations  1 i32 out, or NULL: how often the objective was evaluated
 *   trace_scale, trace_objective   NULL, or trace_len f64 each: the first trace_len evaluated (s, objective) pairs
 *                in the order of evaluation (both or neither)
 * TOPOLOW_ERR_BAD_ARGUMENT, before any device call: NULL positions, reduced or scale; n < 2; k < 1 or k > ndim; a
 * bound or tol that is not finite; lower >= upper; tol <= 0; trace_len < 0 or one trace array without the other; a
 * coordinate that is not finite.  TOPOLOW_ERR_UNSUPPORTED: ndim > 16. */
int topolow_scale_to_original_distances(const double* positions, const double* reduced, int32_t n, int32_t ndim, int32_t k,
                                        double lower, double upper, double tol, double* scale, double* objective,
                                        int32_t* evaluations, double* trace_scale, double* trace_objective,
                                        int32_t trace_len, int32_t device, char* errbuf, size_t errlen);

/* ---------------------------------------------------------------------------------------
 * Prepared layout: the reference's pre-processing (R/core.R:269-436) on the device -- ordering means, degrees,
 * the upper-triangle edge list in which() order, the symmetric dense fill, the scale of the random-walk start.
 * The edge count is unknown before the first pass, hence a handle: create() uploads the matrix and computes,
 * info->n_edges sizes the caller's edge arrays, fetch() downloads.
 *   values   n x n f64, NaN = NA, any threshold prefix stripped
 *   codes    n x n int8 {0, 1 ">", -1 "<"}, or NULL: all zero
 *   transposed != 0: the buffers hold the matrix row-major.  The results are those of the matrix itself; no
 *            transposed n x n copy is made anywhere.  Every n x n output of fetch() is laid out as the inputs are
 *            (dense and tdense are symmetric bit for bit, so their layout does not show).
 * First pass: per point the sum and count of its non-NA off-diagonal cells along its row and along its column
 * (thresholds with their stripped value), per row the non-NA count with the diagonal (the degrees), and info.
 * The summation order is fixed: one partial per (point, block of 64 cells) -- the cells of the block added in index
 * order from 0.0, NA and the diagonal as 0.0 -- and a point's partials added in block order.  The same bits
 * whatever the grid, the chunking of the upload and the layout.
 * Order: topolow_layout_order_from_sums on those sums (unless preserve_order or order_in decide it).
 * Second pass, on the matrix gathered through the order: the edge list (non-NA cells of the strict upper triangle
 * whose distance is not +Inf, column after column, rows ascending: a stable compaction), edge_thresh from the codes,
 * degrees[i] = row count of point order[i], dense / tdense as the 16-argument call takes them (unmeasured = +Inf,
 * the lower triangle the transpose of the upper, R/core.R:429-436), and the raw reordered matrix.
 * Memory: the matrix (9 n^2 bytes, 8 without codes) and the dense fill (12 n^2 bytes; the edge list is compacted from
 * it) stay on the device between create() and destroy(); the first fetch() (or session loaded from the handle that
 * gathers an edge list) adds the edge list, which then stays too; fetch() adds, when asked for, the reordered matrix.  A failed device allocation: TOPOLOW_ERR_UNSUPPORTED with a message.
 * ------------------------------------------------------------------------------------- */
typedef struct topolow_layout_prep topolow_layout_prep;

#define TOPOLOW_ORDER_PRESERVED 0     /* preserve_order: input order kept */
#define TOPOLOW_ORDER_DEVICE_EXACT 1  /* the device sums are exact: keys equal NumPy's bit for bit, ties included */
#define TOPOLOW_ORDER_DEVICE_GAP 2    /* neighbouring keys further apart than both implementations' error */
#define TOPOLOW_ORDER_DECLINED 3      /* the caller orders (order_in); also reported when order_in was given */

typedef struct topolow_layout_prep_info {
  int64_t n_edges;            /* measured cells of the strict upper triangle of the (re)ordered matrix; -1: declined */
  int64_t n_finite_nonzero;   /* cells with code 0, finite, != 0: _validate's warning (R/core.R:202-264) */
  int64_t n_infinite, n_negative;   /* over every non-NA cell, whatever its code */
  double  numeric_max;        /* max over non-NA cells with code 0 (as.numeric form); NaN when there is none */
  int32_t reordered;          /* 0: input order kept (order[0] = -1), as spectral_order() returning None */
  int32_t order_route;        /* TOPOLOW_ORDER_* */
  int32_t exact_sums;         /* every non-NA value is k * 2^-10 with 0 <= value < 2^20 */
  int32_t reserved[5];
} topolow_layout_prep_info;

/* order_in: NULL, or the caller's order -- n entries, a permutation of 0..n-1, or order_in[0] = -1 for "keep the
 * input order" (then one entry is read).  preserve_order != 0 wins over it.
 * With neither, the device keys decide the order where they provably sort as NumPy's do (routes 1 and 2, see
 * topolow_layout_order_from_sums).  Otherwise the call declines: it returns TOPOLOW_OK with order_route 3,
 * n_edges = -1 and a handle that holds no second pass (fetch() on it: TOPOLOW_ERR_BAD_ARGUMENT; destroy it); the
 * caller computes the order as it did before and creates again with order_in.
 * TOPOLOW_ERR_BAD_ARGUMENT before any device call: NULL out, values or info; n < 2; an order_in that is no
 * permutation. */
int topolow_layout_prep_create(topolow_layout_prep** out, const double* values, const int8_t* codes, int32_t n,
                               int32_t transposed, int32_t preserve_order, const int32_t* order_in, int32_t device,
                               topolow_layout_prep_info* info, char* errbuf, size_t errlen);

/* order, degrees: n entries each.  edge_*: info.n_edges entries each.  dense (f64), tdense (i32), values_reordered
 * (f64), codes_reordered (i8): n x n each, or NULL: not wanted -- the other outputs do not depend on it. */
int topolow_layout_prep_fetch(topolow_layout_prep* p, int32_t* order, int32_t* degrees, int32_t* edge_i,
                              int32_t* edge_j, double* edge_dist, int32_t* edge_thresh, double* dense, int32_t* tdense,
                              double* values_reordered, int8_t* codes_reordered, char* errbuf, size_t errlen);
void topolow_layout_prep_destroy(topolow_layout_prep* p);

/* A study entry (tests/study/prepare_layout_timing.py): wall-clock seconds of {upload overlapped with the first pass,
 * the ordering rule on the host, the second pass, fetch()'s compaction and reorder gather, fetch()'s downloads} of
 * this handle; 5 doubles out.  A handle that declined has the first figure only. */
int topolow_layout_prep_phase_seconds(const topolow_layout_prep* p, double* seconds);

/* ---------------------------------------------------------------------------------------
 * Resident embedding: prepare, relax and score from ONE upload.  The three entries below read what a handle keeps on
 * the device instead of the arrays fetch() would download and the caller upload again; each returns the bits the
 * route over fetch() returns (tests/test_gpu_resident_embedding.py).  The handle is not consumed by any of them:
 * fetch() afterwards returns what it returned before.
 * Memory: between create() and destroy() the handle holds 21 n^2 bytes (the matrix 8 + its codes 1, the dense fill
 * 8 + 4; 20 without codes), after the first compaction also its edge list (20 bytes per edge), beside the session's
 * blocks (4 ld n bytes, 8 with f64_exact).  A failed device allocation: TOPOLOW_ERR_UNSUPPORTED with a message.
 * ------------------------------------------------------------------------------------- */

/* Loads a whole-problem session (row_begin = 0, row_end = n) from a handle that holds a second pass: what
 * topolow_session_load_dense / _load_coo + topolow_session_set_edges do with the arrays fetch() returns, device to
 * device -- the encoded block (and the deltas of an f64_exact session) from the resident dense fill through the
 * session's relabelling, the degree terms, and the convergence edge list in session labels where the session gathers
 * one (f64 sessions, ndim > 16, TOPOLOW_EDGE_MAE=1); otherwise the check reads the block, as after set_edges, and the
 * handle's list is not even compacted.  A -DTOPOLOW_ENC_TILED=1 build is covered (the encoder addresses the block
 * through enc_index).
 * TOPOLOW_ERR_BAD_ARGUMENT with a message, before any device call: a NULL argument; a handle that declined; a handle
 * of another n; a row-block session; a handle on another device than the session's. */
struct topolow_session;   /* the session type: "Device-resident session" below */
int topolow_session_load_prepared(struct topolow_session* s, topolow_layout_prep* p, char* errbuf, size_t errlen);

/* topolow_optimize_layout_exact with the matrix, the degrees and the edges taken from the handle (n is the handle's):
 * the same route for the same n, ndim and options, the same run, the same verbose lines, interrupt polls and stats.
 * initial_positions: n x ndim, row q for the q-th point of the ORDERED matrix.  The slab and tile Gauss-Seidel routes
 * load their session with topolow_session_load_prepared; the one-workgroup route (small n) fetches into temporaries
 * inside the call.  opt->device: -1, or the handle's device.
 * TOPOLOW_ERR_BAD_ARGUMENT before any device call: a NULL handle, initial_positions or output (stats may be NULL); a
 * handle that declined; opt->device naming another device.  TOPOLOW_ERR_UNSUPPORTED: a sharded run (opt->n_devices > 1
 * or opt->devices) -- the caller keeps the route over fetch(). */
int topolow_layout_prep_optimize(topolow_layout_prep* p, const double* initial_positions, int32_t ndim,
                                 int32_t n_iter, double k0, double cooling_rate, double c_repulsion,
                                 double relative_epsilon, int32_t convergence_window, int32_t convergence_check_freq,
                                 int32_t verbose, const topolow_options* opt, double* positions_out,
                                 int32_t* converged, int32_t* iterations, double* final_mae, double* final_k,
                                 topolow_run_stats* stats, char* errbuf, size_t errlen);

/* topolow_post_metrics on the handle's resident matrix, gathered through its order: positions n x ndim f64
 * column-major (host), row q for the q-th point of the ordered matrix; est_distances n x n f64 out (host) or NULL,
 * bit-identical to topolow_est_distances, leaving through the same tiled, pinned, overlapped download
 * (TOPOLOW_POST_TILE_COLS applies).  A cell counts iff its value is finite and its code is 0, the diagonal included.
 * The sum: one partial per LINE of the handle's buffer, reduced on the device in topolow_post_metrics' fixed order,
 * the lines added in index order on the host -- the same bits whatever the tile size and whether or not est_distances
 * is asked for.  For a handle created with transposed = 1 a line is a row of the matrix: sum_abs has the bits
 * topolow_post_metrics gives when it reads the C-ordered reordered matrix as its transpose (what
 * euclidean_embedding() did before).  For transposed = 0 a line is a column: count and est_distances are identical,
 * sum_abs / count agrees with that reading to 1e-12 relative (the same terms, grouped by columns instead of rows).
 * TOPOLOW_ERR_BAD_ARGUMENT before any device call: NULL handle, positions, sum_abs or count; ndim < 1; a handle that
 * declined. */
int topolow_layout_prep_post_metrics(topolow_layout_prep* p, const double* positions, int32_t ndim,
                                     double* est_distances, double* sum_abs, int64_t* count, char* errbuf,
                                     size_t errlen);

/* The n-sized outputs of fetch() alone, from the handle's host side (no device call, nothing of edge-list size moves):
 * order (order[0] = -1: the input order is kept) and degrees, n entries each; either may be NULL, not both.
 * TOPOLOW_ERR_BAD_ARGUMENT: a NULL or declined handle. */
int topolow_layout_prep_order(const topolow_layout_prep* p, int32_t* order, int32_t* degrees);

/* A study entry (tests/study/resident_embedding_timing.py): wall-clock seconds of this handle's last
 * topolow_session_load_prepared, last topolow_layout_prep_optimize (the whole call) and last
 * topolow_layout_prep_post_metrics; 3 doubles out, 0 where none ran. */
int topolow_layout_prep_resident_seconds(const topolow_layout_prep* p, double* seconds);

/* Host only: the ordering rule on given sums -- what create() runs after its first pass.
 * NOTE: exact_sums is three-valued here, unlike the 0 / 1 field of the info struct.  0 asserts that the data hold no
 * negative and no infinite cell; a caller whose data may hold one passes -1 (create() does, from info.n_negative and
 * info.n_infinite), or the gap rule would be applied where its error bound does not hold.
 *   key = (row_sum / row_cnt + col_sum / col_cnt) / 2, NaN (a count of 0) -> 0.
 *   No reordering (order_out[0] = -1) unless more than one key is > 0; otherwise a stable ascending sort.
 *   exact_sums > 0: the sums are exact (info.exact_sums, n <= 2^23), the keys are NumPy's bit for bit: route 1.
 *   exact_sums == 0: no negative and no infinite cell.  Route 2 if every two neighbouring keys of the sorted list are
 *     further apart than 8 n 2^-53 of the larger one (or both exactly 0) and the smallest positive key is >= 2^-1000:
 *     with non-negative terms either implementation is within (n + 2) 2^-53 relative of the true key, so keys
 *     further apart than 4 (n + 2) 2^-53 sort alike in both; the bound is doubled.  Otherwise route 3.
 *   exact_sums < 0: the data hold a negative or an infinite cell and are not exact: route 3.
 * Returns the route; on route 3 order_out[0] = -1 and nothing else is written. */
int32_t topolow_layout_order_from_sums(int32_t n, const double* row_sum, const int64_t* row_cnt,
                                       const double* col_sum, const int64_t* col_cnt, int32_t exact_sums,
                                       int32_t* order_out);

/* ---------------------------------------------------------------------------------------
 * Cross-validation folds from a prepared handle: a whole sweep from ONE upload of the matrix.  A fold is its picks
 * (linear column-major indices r + c n, as topolow_cv_fold; their mirrors are held out too, the diagonal is eligible);
 * the device marks them in a fold mask of n^2 bits that lives in the handle and is empty again when either entry
 * returns, and derives from the masked matrix what topolow_cv_fold_pairs derives from the cell list.  Per fold the
 * picks go up and O(n) numbers come down; nothing of size n x n or O(cells) is touched on the host.  vals and codes are
 * never written: fetch(), optimize() and post_metrics() afterwards return what they returned before.
 * Both entries want a handle created with preserve_order (the fold's labels are the caller's; a handle that declined
 * or reordered: TOPOLOW_ERR_BAD_ARGUMENT, "create the handle with preserve_order") and a SYMMETRIC matrix -- every
 * off-diagonal cell has a mirror with the same value bits, the same NA-ness and the same code, decided on the device
 * at the first fold, once per handle; otherwise TOPOLOW_ERR_UNSUPPORTED with topolow_cv_fold_pairs' message.  A pick
 * outside 0 .. n^2 - 1: TOPOLOW_ERR_BAD_ARGUMENT.  The first fold adds n^2 / 8 bytes (the mask) and 24 n^2 / 64 bytes
 * (the partial sums) to what the handle holds.
 * ------------------------------------------------------------------------------------- */

/* topolow_cv_fold_pairs from the handle: the same outputs, computed on the device and downloaded.
 *   order        as topolow_cv_fold_pairs, from topolow_layout_order_from_sums on the masked sums, judged with the
 *                full matrix's exact_sums and negative / infinite counts (conservative for a subset of its cells).
 *                *order_route says how (TOPOLOW_ORDER_*).  On TOPOLOW_ORDER_DECLINED the entry still returns
 *                TOPOLOW_OK, order[0] = -1 and the scored cells are in the caller's numbering; degrees, numeric_max,
 *                n_edges and the pairs are valid, the caller orders the fold on the host.
 *   degrees, numeric_max, n_edges   equal to topolow_cv_fold_pairs'
 *   pair_i/_j    the same SET of unique held-out pairs i < j, sorted by (j, i) (up to n_picks entries)
 *   score_i/_j/_truth  equal to topolow_cv_fold_pairs' element for element: ascending column-major index of the
 *                cell, the truth read from the resident matrix (up to 2 n_picks entries)
 * TOPOLOW_ERR_BAD_ARGUMENT before any device call: a NULL argument (picks may be NULL when n_picks is 0), n_picks < 0. */
int topolow_layout_prep_fold(topolow_layout_prep* p, const int64_t* picks, int64_t n_picks, int32_t preserve_order,
                             int32_t named, int32_t* order, int32_t* degrees, double* numeric_max, int64_t* n_edges,
                             int32_t* pair_i, int32_t* pair_j, int64_t* n_pairs, int32_t* score_i, int32_t* score_j,
                             double* score_truth, int64_t* n_scored, int32_t* order_route, char* errbuf, size_t errlen);

/* topolow_cv_sweep_session with the handle in place of the cell list (the device is the handle's): the same grouping
 * by ndim, one session per group, relabelled from the group's first seed and loaded with
 * topolow_session_load_prepared; the same numbers, bit for bit, for every fold it runs.  Per fold: mark, masked sums,
 * order; the fold's checks and start positions along its order; compaction of the mask into held-out pairs and
 * scored cells; the hold-out (the pairs mapped to session labels on the device), the run, the score (the scored cells
 * gathered through the order and the session's labels on the device), restore with the handle's full degrees, the
 * mask cleared.  order_route[f]: TOPOLOW_ORDER_* of fold f.  A fold whose order was declined is not run:
 * error_code[f] = TOPOLOW_ERR_UNSUPPORTED, the session is not touched, the caller reruns that fold through
 * topolow_cv_sweep_session.  Other error_code[f] as topolow_cv_sweep_session.  In every case -- errors included --
 * the session is the full matrix again and the mask is empty before the next fold starts and when the call returns.
 * TOPOLOW_ERR_BAD_ARGUMENT before any device call: a NULL argument, n_folds < 0, an unknown schedule; n_folds == 0
 * is TOPOLOW_OK.  precision f64_exact: TOPOLOW_ERR_UNSUPPORTED, as topolow_cv_sweep_session. */
int topolow_layout_prep_cv_sweep(topolow_layout_prep* p, int32_t named, int32_t preserve_order, int32_t n_folds,
                                 const int32_t* ndim, const double* k0, const double* cooling_rate,
                                 const double* c_repulsion, const int64_t* picks, const int64_t* picks_offset,
                                 const double* unit_draws, const int64_t* draws_offset, const uint64_t* seeds,
                                 int32_t n_iter, double relative_epsilon, int32_t convergence_window,
                                 int32_t convergence_check_freq, int32_t precision, int32_t schedule,
                                 double* holdout_sum_abs, int64_t* holdout_count, int32_t* iterations, int32_t* converged,
                                 int32_t* error_code, int32_t* order_route, double* device_seconds, char* errbuf,
                                 size_t errlen);

/* A study entry (tests/study/cv_resident_cost.py): wall-clock seconds of this handle's last topolow_layout_prep_cv_sweep,
 * summed over its folds: {fold preparation (mark, sums, order, compaction), hold-out, score, restore}; 4 doubles out. */
int topolow_layout_prep_fold_seconds(const topolow_layout_prep* p, double* seconds);

/* ---------------------------------------------------------------------------------------
 * Connected subsamples of a resident matrix (reference R/utils.R:199-253 check_matrix_connectivity over the adjacency
 * of R/diagnostics.R:442-468, R/utils.R:321-463 subsample_dissimilarity_matrix): the components of the measurement
 * graph of a handle's matrix or of any subset of its points, and a child handle for parent[subset, subset], both from
 * what the parent keeps on the device.
 * subset: NULL for all n points (m is then ignored), or m distinct indices into the matrix as it was given to create(),
 * in any order.  Both entries take a handle that declined its ordering: it still holds the matrix.
 * TOPOLOW_ERR_BAD_ARGUMENT with a message, before any device call: a NULL handle or output; m < 2 or m > n; an index
 * out of range; a repeated index (and, for subsample, an order_in that is no permutation of 0..m-1).
 * ------------------------------------------------------------------------------------- */

/* The graph: the vertices are the points of the subset; {a, b}, a != b, is an edge iff cell (a, b) OR cell (b, a) is
 * not NaN (!is.na; igraph's mode = "undirected").  Threshold-coded cells and +Inf count as measured, the diagonal
 * never makes an edge; the same graph for either layout flag.
 *   n_cells       the non-NaN off-diagonal cells of the induced submatrix over both triangles (sum(adjacency));
 *                 n_measurements = n_cells / 2, completeness = n_cells / (m (m - 1))
 *   labels        m entries or NULL; labels[q] = the smallest position q' in `subset` whose point lies in the component
 *                 of subset[q] (canonical: any correct algorithm gives the same array)
 *   n_components  the number of q with labels[q] == q
 * One pass over the matrix leaves a packed bit adjacency of the subset (m^2 / 8 bytes) and n_cells; the component
 * rounds run on the bits, driven from the host until one changes nothing, at most m + 1 of them (TOPOLOW_ERR_HIP with
 * a message beyond that -- never a hang).  A failed device allocation: TOPOLOW_ERR_UNSUPPORTED with a message. */
int topolow_layout_prep_connectivity(topolow_layout_prep* p, const int32_t* subset, int32_t m, int32_t* n_components,
                                     int64_t* n_cells, int32_t* labels /* m, or NULL */, char* errbuf, size_t errlen);

/* A handle for the matrix parent[subset, subset]: rows and columns in the subset's given order, the parent's layout
 * flag, its codes if it has any, its device.  Values and codes are gathered device to device; then the child goes
 * through exactly what create() does after its upload (first pass, ordering rule, second pass), so `info`, fetch(),
 * order() and every other entry give, bit for bit, what a handle created from the host-gathered submatrix gives.
 * preserve_order and order_in as for create(), relative to the child's own m points.  The child owns its buffers
 * (21 m^2 bytes, as a fresh handle), outlives the parent and serves every handle entry, these two included; the parent
 * is not touched.  A failed device allocation: TOPOLOW_ERR_UNSUPPORTED with a message. */
int topolow_layout_prep_subsample(topolow_layout_prep* parent, const int32_t* subset, int32_t m,
                                  int32_t preserve_order, const int32_t* order_in, topolow_layout_prep** out,
                                  topolow_layout_prep_info* info, char* errbuf, size_t errlen);

/* A study entry (tests/study/subsample_timing.py): of this handle's last topolow_layout_prep_connectivity, the rounds
 * launched (the last one changed nothing) and the wall-clock seconds of {the bit pass, the rounds}; 2 doubles out. */
int topolow_layout_prep_graph_stats(const topolow_layout_prep* p, int32_t* rounds, double* seconds);

/* ---------------------------------------------------------------------------------------
 * Degrees and pruning of a resident matrix (reference R/diagnostics.R:434-475 analyze_network_structure,
 * R/data_preprocessing.R:1225-1503 prune_sparse_matrix).  Both entries count along MATRIX ROWS for either layout flag
 * -- cell (r, c) counts for point r -- and the matrix need not be symmetric.  A cell is measured when it is not NaN:
 * threshold-coded cells and +-Inf count, the diagonal never does.  Both serve a handle that declined its ordering, and
 * neither alters the handle.  One pass over the matrix leaves a packed bit adjacency (n^2 / 8 bytes; twice that while
 * the bits of a column-line layout are turned round, 64 x 64 bits at a time); everything after it reads the bits.
 * Transient device memory: those bits and O(n), freed before return; a failed allocation: TOPOLOW_ERR_UNSUPPORTED with
 * a message.
 * ------------------------------------------------------------------------------------- */

/* degrees[q] = the measured cells (subset[q], subset[c]), c != q, along the matrix row; *n_cells their sum (the n_cells
 * of topolow_layout_prep_connectivity).  subset as for that entry (NULL: all n points, m ignored).
 * TOPOLOW_ERR_BAD_ARGUMENT with a message, before any device call: a NULL handle, degrees or n_cells; the subset errors
 * of the connectivity entry. */
int topolow_layout_prep_degrees(topolow_layout_prep* p, const int32_t* subset, int32_t m, int32_t* degrees /* m */,
                                int64_t* n_cells, char* errbuf, size_t errlen);

#define TOPOLOW_PRUNE_CONVERGED 1       /* a round found every kept point at or above the threshold */
#define TOPOLOW_PRUNE_MIN_POINTS 2      /* removing the round's candidates would leave fewer than min_points: they stay */
#define TOPOLOW_PRUNE_MAX_ITERATIONS 3  /* max_iterations rounds, the last of which still removed points */
#define TOPOLOW_PRUNE_ALL_REMOVED 4     /* a round removed the last points ("All points removed during pruning") */
#define TOPOLOW_PRUNE_MAX_ATTEMPTS 10

typedef struct topolow_prune_info {
  int32_t original_size, final_size;
  int32_t iterations;            /* rounds of the last attempt, counted before the test: a run that converges reports the
                                  * round that found nothing to remove */
  int32_t min_connections_used;  /* the threshold of the last attempt */
  int32_t attempts;              /* 1 without a target */
  int32_t stop_reason;           /* TOPOLOW_PRUNE_* of the last attempt */
  int32_t target_reached;        /* 0 / 1; -1 when no target was given */
  int32_t last_remove;           /* the points the last decided round of the last attempt found below the threshold */
  int64_t original_cells, final_cells;   /* measured off-diagonal cells over both triangles, of the matrix / of kept x kept */
  double  seconds[3];            /* wall clock: the bit pass, the rounds, the rest */
  /* per attempt a (0-based), for the callers that repeat the reference's warnings: */
  int32_t attempt_iterations[TOPOLOW_PRUNE_MAX_ATTEMPTS], attempt_stop_reason[TOPOLOW_PRUNE_MAX_ATTEMPTS];
  int32_t attempt_last_remove[TOPOLOW_PRUNE_MAX_ATTEMPTS], attempt_final_size[TOPOLOW_PRUNE_MAX_ATTEMPTS];
  int64_t attempt_final_cells[TOPOLOW_PRUNE_MAX_ATTEMPTS];
  int64_t reserved[4];
} topolow_prune_info;

/* prune_sparse_matrix on the resident matrix: rounds that remove every kept point with fewer than min_connections
 * measured cells among the kept points of its row, until a round removes nothing (the reference's loop,
 * R/data_preprocessing.R:1371-1415, with the count its documentation describes: the measured off-diagonal cells).
 *   target_completeness NaN   one attempt at min_connections.
 *   target_completeness t     the reference's search as its code has it (:1288-1355): thresholds 4, 6, 8, ... for at
 *                             most TOPOLOW_PRUNE_MAX_ATTEMPTS attempts, each from the whole matrix, all inside this call
 *                             on one bit pass; min_connections is not used.  An attempt ends the search when
 *                             final_cells / (s (s - 1)) >= t in double, s its final_size (target_reached = 1), when
 *                             s <= min_points, or when it removed every point; running out of attempts is TOPOLOW_OK
 *                             with target_reached = 0 and attempts = TOPOLOW_PRUNE_MAX_ATTEMPTS.
 *   kept                      n flags of the last attempt: 1 where the point stays.
 * A round is two launches (count, decide); the host launches them in batches behind a device stop flag and reads one
 * small record per batch; at most min(max_iterations, n) + 1 count launches per attempt.
 * TOPOLOW_ERR_BAD_ARGUMENT with a message, before any device call: a NULL handle, kept or info; min_connections < 1;
 * a target that is not NaN and lies outside (0, 1]; n < min_points.  max_iterations <= 0 runs no round, as the
 * reference's loop does. */
int topolow_layout_prep_prune(topolow_layout_prep* p, int32_t min_connections,
                              double target_completeness /* NaN: fixed threshold */, int32_t max_iterations,
                              int32_t min_points, uint8_t* kept /* n flags */, topolow_prune_info* info, char* errbuf,
                              size_t errlen);

/* ---------------------------------------------------------------------------------------
 * Spectrum of a resident matrix: step 1 of the reference's Euclidify(), "Assessing data characteristics"
 * (R/core.R:983-1007) -- as.numeric, median fill, square, double-centre, all eigenvalues, deviation_score and
 * dims_90_percent -- and the symmetric eigenvalue path under it.  All f64, one GPU, no solver library.
 *   Householder tridiagonalisation, unblocked, one reflection per column applied as a rank-2 update of the trailing
 *   matrix: three launches per step on one stream (a one-workgroup step kernel; one streaming kernel that applies the
 *   pending update and accumulates the next A v in the same read, one partial per column and block of 64 lines; one
 *   kernel that adds the partials in block order), no grid barrier.  The matrix is held in full
 *   (both triangles, kept symmetric bit for bit): 8 n^2 bytes, read and written once per step.
 *   Eigenvalues of the tridiagonal by Sturm bisection on the Gershgorin interval, one index per thread, with LAPACK
 *   dstebz's pivmin guard; an interval ends at a width of 2 u max(|lo|, |hi|) + pivmin, u = 2^-52.  Descending order.
 *   No floating-point atomics: every reduction has fixed partitions added in fixed order, so two calls on the same
 *   input return the same bits.  The entries assume values whose squares stay inside the f64 range.
 * ------------------------------------------------------------------------------------- */

/* All eigenvalues of the symmetric tridiagonal matrix with diagonal d (n) and off-diagonal e (n - 1; not read when
 * n == 1), descending, into eigenvalues_out (n).  A zero in e needs no special treatment.
 * TOPOLOW_ERR_BAD_ARGUMENT with a message, before any device call: NULL d or eigenvalues_out; n < 1; NULL e with
 * n >= 2; an entry of d or e that is not finite. */
int topolow_tridiagonal_eigenvalues(const double* d, const double* e, int32_t n, int32_t device,
                                    double* eigenvalues_out, char* errbuf, size_t errlen);

/* a: host, n x n f64 column-major; only its lower triangle (row >= column) is read.  Each output may be NULL (not
 * wanted): d_out (n) and e_out (n - 1), the tridiagonal form Q^T A Q, and eigenvalues_out (n), descending.
 * Memory: the matrix on the device (8 n^2 bytes) and O(n) beside it; a failed allocation: TOPOLOW_ERR_UNSUPPORTED.
 * TOPOLOW_ERR_BAD_ARGUMENT with a message, before any device call: NULL a; n < 1; a cell of the lower triangle that
 * is not finite. */
int topolow_symmetric_eigenvalues(const double* a, int32_t n, int32_t device, double* d_out, double* e_out,
                                  double* eigenvalues_out, char* errbuf, size_t errlen);

typedef struct topolow_spectrum_info {
  double  median;             /* of the numeric cells (code 0, not NaN), diagonal and both triangles: np.median's value */
  int64_t n_numeric;          /* how many of them there are */
  int64_t n_filled;           /* n^2 - n_numeric: the cells that took the median (NaN, or a threshold code) */
  double  trace;              /* of the centred matrix B, its diagonal added in index order */
  int64_t n_positive, n_negative;       /* eigenvalues > 1e-12, < -1e-12 */
  double  sum_positive, sum_negative;   /* their sums, the negative ones by absolute value */
  double  deviation_score;    /* sum_negative / sum_positive; 1.0 when nothing is positive */
  int32_t dims_90;            /* max(1, first count of leading positive eigenvalues with >= 0.90 of sum_positive) */
  int32_t reserved32;
  double  seconds[4];         /* wall clock: median, centring, tridiagonalisation, bisection */
  int64_t reserved[4];
} topolow_spectrum_info;

/* The assessment of the handle's matrix, defined on the matrix in its INPUT order whatever the handle's ordering (a
 * handle that declined its ordering serves: only the matrix and the codes are read).  The matrix need not be symmetric.
 *   median   over every cell with code 0 that is not NaN, by a radix select over the order-preserving 64-bit key of
 *            the double, both middle ranks in the same 8 passes, integer atomics only; an even count gives
 *            (a + b) / 2 of the two middle values.  Equal to np.median of those cells (the sign of a zero aside).
 *   x_ij     the cell where it is numeric, otherwise the median (threshold-coded cells too: as.numeric makes them NA)
 *   B_ij     -0.5 (x_ij^2 - r_i - c_j + g), r / c / g the row / column / grand means of x^2.  The sums follow the first
 *            pass's rule ("Prepared layout" above: one partial per point and block of 64 cells added in index order, a
 *            point's partials in block order), g comes from the row sums in index order: the same bits whatever the
 *            grid and the layout flag.
 *   eigenvalues   of the symmetric matrix whose lower triangle (row >= column) is B's, as R's eigen(symmetric = TRUE)
 *            and NumPy's eigvalsh read it; descending
 *   info     deviation_score and dims_90 from the downloaded eigenvalues on the host, as R/core.R:994-1007
 * eigenvalues_out: n, or NULL.  centered_out: host, n x n laid out as the handle's inputs are, or NULL: B itself, both
 * triangles as computed.  The handle is neither consumed nor altered: fetch(), optimize() and the fold entries return
 * afterwards what they returned before.  B is 8 n^2 bytes of transient device memory, freed before return; a failed
 * allocation: TOPOLOW_ERR_UNSUPPORTED with a message.
 * TOPOLOW_ERR_BAD_ARGUMENT with a message: a NULL handle or info (before any device call); no numeric cell; a code-0
 * cell that is +-Inf ("infinite or missing values in 'x'", R's eigen). */
int topolow_layout_prep_spectrum(topolow_layout_prep* p, double* eigenvalues_out /* n, or NULL */,
                                 double* centered_out /* n x n, or NULL */, topolow_spectrum_info* info, char* errbuf,
                                 size_t errlen);

/* ---------------------------------------------------------------------------------------
 * Fit report of a resident embedding (reference R/error_metrics.R:55-202 error_calculator_comparison and
 * calculate_prediction_interval, R/visualization.R:2626-2648): the signed errors e = v - r of the handle's matrix
 * against a set of positions -- v the cell's value, r the distance of the two points with the bits of
 * topolow_est_distances -- their moments per series and their exact order statistics, from what the handle keeps on
 * the device.  Nothing of size n x n is allocated, downloaded or touched on the host; no buffer of errors exists.
 *   positions   n x ndim f64 column-major (host), row q for the q-th point of the ordered matrix, exactly as
 *               topolow_layout_prep_post_metrics; they must be finite
 *   picks       the held-out cells as linear column-major indices r + c n in the CALLER's numbering, as
 *               topolow_layout_prep_fold; their mirrors are held out too; NULL when n_picks is 0.  They are marked in
 *               the handle's fold mask, which is empty again on every return, errors included.  A pick outside
 *               0 .. n^2 - 1: TOPOLOW_ERR_BAD_ARGUMENT with the fold entries' message.
 * A cell belongs to zero or more of three series:
 *   TOPOLOW_FIT_IN    its value is finite, its code is 0 and it is not held out
 *   TOPOLOW_FIT_OUT   its value is finite, its code is 0 and it is held out
 *   TOPOLOW_FIT_ALL   its value is finite, whatever its code and whether held out or not (extract_numeric_values)
 * The diagonal counts, as in post-metrics.  DEVIATION from the reference: +-Inf cells are left out of every series, as
 * post-metrics leaves them out; in the reference they would turn every statistic into Inf or NaN.
 * Unlike the fold entries these need neither preserve_order nor a symmetric matrix: any handle that holds a second pass
 * serves (a handle that declined its ordering: TOPOLOW_ERR_BAD_ARGUMENT).  The handle is not altered: fetch(),
 * optimize(), post_metrics() and the fold entries return afterwards what they returned before.  The first call with
 * picks adds what the first fold adds (the mask, n^2 / 8 bytes, and the fold's O(n^2 / 64) partials).
 * Both entries: TOPOLOW_ERR_BAD_ARGUMENT with a message before any device call for a NULL handle, positions or output,
 * ndim < 1, n_picks < 0, picks NULL with n_picks > 0 (and, for the order statistics, an unknown series, n_ranks outside
 * 1 .. TOPOLOW_FIT_MAX_RANKS, a malformed negative rank).  A failed device allocation: TOPOLOW_ERR_UNSUPPORTED with
 * the handle as it was.
 * ------------------------------------------------------------------------------------- */
#define TOPOLOW_FIT_IN 0
#define TOPOLOW_FIT_OUT 1
#define TOPOLOW_FIT_ALL 2
#define TOPOLOW_FIT_MAX_RANKS 8
#define TOPOLOW_FIT_RANK_UPPER ((int64_t)1 << 32) /* see topolow_layout_prep_fit_order_stats: ranks */

typedef struct topolow_fit_series {
  int64_t count;              /* m: the cells of the series */
  double  sum_e, sum_abs_e;   /* sum of e, of |e| */
  double  min_e, max_e;       /* the bits of the smallest / largest e; NaN when count is 0 */
  int64_t pct_count;          /* IN, OUT: the cells of the series with v > 0 (R/error_metrics.R:116); ALL: 0 */
  double  sum_pct, sum_abs_pct;   /* IN, OUT: sum of p = e / v * 100 over them, of |p|; ALL: 0 */
  double  sum_v, sum_r;       /* ALL: sum of v, of r; IN, OUT: 0 */
  double  css_e;              /* sum of (e - mean e)^2, mean e = sum_e / count formed on the host between the passes */
  double  css_v, css_r, css_vr;   /* ALL: sum of (v - mean v)^2, (r - mean r)^2, (v - mean v)(r - mean r); IN, OUT: 0 */
} topolow_fit_series;

typedef struct topolow_fit_report {
  topolow_fit_series series[3];   /* [TOPOLOW_FIT_IN], [TOPOLOW_FIT_OUT], [TOPOLOW_FIT_ALL] */
  double  seconds[3];         /* wall clock: pass 1 (with the upload and the marking), pass 2, the whole call */
  int64_t reserved[4];
} topolow_fit_report;

/* Two passes over the resident matrix.  Every sum is reduced in topolow_post_metrics' fixed order -- each lane over its
 * indices in ascending order, the 64 lanes by a shuffle tree, the four waves in wave order, one partial per line of the
 * handle's buffer, the lines added in index order on the host -- with no floating-point atomic anywhere: the same bits
 * on every call.  The second pass takes the means the host formed from the first pass's totals. */
int topolow_layout_prep_fit_report(topolow_layout_prep* p, const double* positions, int32_t ndim,
                                   const int64_t* picks, int64_t n_picks, topolow_fit_report* out, char* errbuf,
                                   size_t errlen);

/* Exact order statistics of the signed errors of one series: a radix select over the order-preserving 64-bit key of the
 * double, one 8-bit digit per pass, all ranks at once -- exactly eight passes over the resident matrix whatever the
 * data, the errors recomputed in every pass; integer atomics only.
 *   series       TOPOLOW_FIT_IN, _OUT or _ALL
 *   ranks        n_ranks of them, 1 <= n_ranks <= TOPOLOW_FIT_MAX_RANKS.  A rank >= 0 is a 0-based rank of the ascending
 *                errors.  A negative rank -1 - q, q in 0 .. 1000000, is the rank floor((m - 1) q / 10^6): the lower
 *                neighbour of R's type-7 quantile at q / 10^6, for a caller that does not know m yet;
 *                -1 - (q + TOPOLOW_FIT_RANK_UPPER) is ceil((m - 1) q / 10^6), the upper neighbour.  (A caller that has
 *                the report knows m and passes plain ranks; topolow_amd.error_metrics does.)
 *   values_out   n_ranks doubles: values_out[k] has the bits of the ranks[k]-th smallest error (-0.0 sorts before 0.0)
 *   count_out    m
 * An empty series: TOPOLOW_OK, m = 0 and NaN values.  A rank >= m: TOPOLOW_ERR_BAD_ARGUMENT, reported after the first
 * pass (which counts m).  A rank whose key the eighth pass does not find: TOPOLOW_ERR_HIP with a message -- no pass is
 * ever added. */
int topolow_layout_prep_fit_order_stats(topolow_layout_prep* p, const double* positions, int32_t ndim,
                                        const int64_t* picks, int64_t n_picks, int32_t series,
                                        const int64_t* ranks, int32_t n_ranks, double* values_out, int64_t* count_out,
                                        char* errbuf, size_t errlen);

/* ---------------------------------------------------------------------------------------
 * The fit's diagnostic plots without their points (reference R/visualization.R:2616-2701 scatterplot_fitted_vs_true,
 * R/diagnostics.R:128-183 plot_embedding_quality): the extent of a series, exact 2-D bin counts and the mass
 * distribution of density()'s linear binning, one pass each over the resident matrix, integer atomics only -- the same
 * numbers on every call.  p, positions, ndim, picks, n_picks and series mean exactly what they mean for
 * topolow_layout_prep_fit_report: the same three series (the diagonal counts; +-Inf cells are left out of every series),
 * the same marking and clearing of the fold mask, the same handles served, the handle left as it was on every return,
 * and TOPOLOW_ERR_BAD_ARGUMENT with a message before any device call for a NULL handle, positions or output, ndim < 1,
 * n_picks < 0, picks NULL with n_picks > 0, an unknown series or axis and the limits stated below.
 * DEVIATION from plot_embedding_quality, which masks the diagonal: here the diagonal counts, as in the fit report.
 * A cell offers four quantities, v its value and r the distance with the bits of topolow_est_distances.  RESIDUAL is
 * there so that neither plot's sign convention needs reversed edges, which would move the closed side of a bin.
 * ------------------------------------------------------------------------------------- */
#define TOPOLOW_FIT_AXIS_TRUE 0      /* v */
#define TOPOLOW_FIT_AXIS_PREDICTED 1 /* r */
#define TOPOLOW_FIT_AXIS_ERROR 2     /* v - r */
#define TOPOLOW_FIT_AXIS_RESIDUAL 3  /* r - v */
#define TOPOLOW_FIT_MAX_BINS 8192    /* nx * ny of topolow_layout_prep_fit_hist2d */
#define TOPOLOW_FIT_MAX_GRID 4096    /* m of topolow_layout_prep_fit_linear_bins */

/* out[2 a], out[2 a + 1]: the bits of the smallest and the largest value of axis a (TOPOLOW_FIT_AXIS_*) over the
 * series; NaN when the series is empty.  count_out: the series' count. */
int topolow_layout_prep_fit_extent(topolow_layout_prep* p, const double* positions, int32_t ndim, const int64_t* picks,
                                   int64_t n_picks, int32_t series, double* out /* 8 */, int64_t* count_out,
                                   char* errbuf, size_t errlen);

/* Exact 2-D bin counts of (x_axis, y_axis) over the series.
 *   x_edges, y_edges   nx + 1 and ny + 1 finite, strictly increasing f64 (host); nx, ny >= 1, nx ny <= TOPOLOW_FIT_MAX_BINS
 *   counts_out         nx * ny, y fastest: counts_out[kx * ny + ky]
 * A value x lies in bin k iff edges[k] <= x < edges[k + 1]; the last bin also takes x == edges[nx] (NumPy's histogram2d
 * with explicit edges).  The bin is found by comparing against the edges themselves, never from a formula, so any
 * strictly increasing edges work and a host that compares the same doubles gets the same counts.  A cell of the series
 * outside either axis goes to outside_out: the sum of counts_out plus outside_out equals count_out. */
int topolow_layout_prep_fit_hist2d(topolow_layout_prep* p, const double* positions, int32_t ndim, const int64_t* picks,
                                   int64_t n_picks, int32_t series, int32_t x_axis, const double* x_edges, int32_t nx,
                                   int32_t y_axis, const double* y_edges, int32_t ny, int64_t* counts_out,
                                   int64_t* outside_out, int64_t* count_out, char* errbuf, size_t errlen);

/* The mass distribution of density()'s linear binning (R's BinDist) of one axis over the series, in integers:
 *   delta = (up - lo) / (m - 1); xpos = (x - lo) / delta; ix = floor(xpos); fx = xpos - ix
 * For 0 <= ix <= m - 2 the cell adds 1 to count_out[ix] and (uint64)(fx 2^32) to frac_out[ix]; every other cell of the
 * series goes to outside_out; total_out is the series' count.  The host forms mass[g] = (count[g] - S[g]) + S[g - 1]
 * with S = frac 2^-32.  Every operation is a plain IEEE f64 one, so a host doing the same gets the same integers.
 * DEVIATION from BinDist: the quantisation of fx moves a cell's mass by at most 2^-32 of itself.
 *   m        2 <= m <= TOPOLOW_FIT_MAX_GRID;  lo < up, both finite
 * TOPOLOW_ERR_UNSUPPORTED when n n >= 2^32: a bin's fraction sum must fit 64 bits. */
int topolow_layout_prep_fit_linear_bins(topolow_layout_prep* p, const double* positions, int32_t ndim,
                                        const int64_t* picks, int64_t n_picks, int32_t series, int32_t axis, double lo,
                                        double up, int32_t m, int64_t* count_out /* m */,
                                        uint64_t* frac_out /* m, units of 2^-32 */, int64_t* outside_out,
                                        int64_t* total_out, char* errbuf, size_t errlen);

/* ---------------------------------------------------------------------------------------
 * Device-resident session: the same relaxation with inputs kept in HBM, for callers that
 * run many iterations / many embeddings on data they already hold on the GPU (bench.py, the
 * row-sharded multi-GPU driver).  Pointers named d_* are DEVICE pointers.
 * ------------------------------------------------------------------------------------- */
typedef struct topolow_session topolow_session;

/* Creates a session for rows [row_begin, row_end) of an n-point problem (single GPU:
 * row_begin = 0, row_end = n).  The session owns an encoded fp32 target block of
 * (row_end-row_begin) x ld floats (see topolow_session_encoded_ld). */
int topolow_session_create(topolow_session** out, int32_t n, int32_t ndim, int32_t row_begin,
                           int32_t row_end, int32_t precision, int32_t device, char* errbuf,
                           size_t errlen);
void topolow_session_destroy(topolow_session* s);

/* Optional, before anything is loaded: store the points in a random order (a permutation drawn from
 * `seed`; 0 = the caller's order).  A slab -- a run of consecutive session labels -- is then a random
 * subset of the caller's points, not a run of points that lie next to each other on the reference's
 * random-walk start (R/core.R:407-415).  Every entry point that takes or returns HOST arrays keeps
 * speaking the caller's labels; device buffers handed to topolow_session_stage / _edge_error /
 * _check_partial are in session labels (topolow_session_labels gives the map).  Sessions that share
 * n and seed share the permutation (row-sharded runs). */
int topolow_session_set_relabel(topolow_session* s, uint64_t seed, char* errbuf, size_t errlen);
/* session label q holds the caller's point session_to_caller[q] (n entries). */
int topolow_session_labels(const topolow_session* s, int32_t* session_to_caller);

/* Encode the reference's dense inputs (host pointers, R layout) into the session's HBM
 * block.  Only rows [row_begin,row_end) are read. */
int topolow_session_load_dense(topolow_session* s, const double* dissimilarity_matrix,
                               const int32_t* threshold_matrix, const int32_t* degrees,
                               char* errbuf, size_t errlen);
/* COO entry for problems too large for dense host matrices (BASELINE config 4): edges are
 * the upper-triangle measured pairs (host pointers); degrees as above. */
int topolow_session_load_coo(topolow_session* s, const int32_t* edge_i, const int32_t* edge_j,
                             const double* edge_dist, const int32_t* edge_thresh,
                             int64_t n_edges, const int32_t* degrees, char* errbuf,
                             size_t errlen);
/* Device-side fill: the caller writes the session's encoded block itself (a device buffer of
 * (row_end-row_begin) x ld uint32 words, row-major: the word of (row r of the block, column c) sits at
 * topolow_encoded_index(r, c, ld) = r * ld + c; word = topolow_encode_target(); diagonal, padding
 * and unmeasured cells = topolow_encode_target(+Inf, 0)), then commits it with the degrees. */
void* topolow_session_encoded_ptr(topolow_session* s);
int32_t topolow_session_encoded_ld(const topolow_session* s);
int topolow_session_commit_encoded(topolow_session* s, const int32_t* degrees, char* errbuf,
                                   size_t errlen);
/* Edge list used by the convergence MAE (host pointers).  For a row-sharded session pass
 * only the edges this rank should reduce (e.g. those with edge_i in its row block). */
int topolow_session_set_edges(topolow_session* s, const int32_t* edge_i, const int32_t* edge_j,
                              const double* edge_dist, const int32_t* edge_thresh,
                              int64_t n_edges, char* errbuf, size_t errlen);
/* Positions: n x ndim float64 column-major host buffer. */
int topolow_session_set_positions(topolow_session* s, const double* positions, char* errbuf,
                                  size_t errlen);
int topolow_session_get_positions(topolow_session* s, double* positions, char* errbuf,
                                  size_t errlen);

/* Starts a run: resets the controller (best = DBL_MAX, k = k0, iteration 0). */
int topolow_session_begin(topolow_session* s, int32_t n_iter, double k0, double cooling_rate,
                          double c_repulsion, double relative_epsilon,
                          int32_t convergence_window, int32_t convergence_check_freq,
                          uint64_t seed, int32_t slab_stages, char* errbuf, size_t errlen);
/* Enqueues up to max_iters iterations (whole check intervals) on the session stream and
 * returns without waiting; *enqueued = iterations enqueued (0 when the run is over). */
int topolow_session_enqueue(topolow_session* s, int32_t max_iters, int32_t* enqueued,
                            char* errbuf, size_t errlen);
/* Waits for the launches enqueued so far on the session's streams and nothing else: a convergence check that is
 * waiting to ride on the next iteration's sweep (one-stage iterations reduce the pending check's MAE on the way) stays
 * pending, as it would in an uninterrupted run; no state is read back.  For callers that pace a run in slices
 * (bench.py) and go on enqueueing. */
int topolow_session_wait(topolow_session* s, char* errbuf, size_t errlen);
/* Waits for everything enqueued, a pending check included (it runs as a separate pass); reports progress. */
int topolow_session_sync(topolow_session* s, int32_t* iterations_run, int32_t* stopped,
                         double* last_mae, char* errbuf, size_t errlen);
/* Restores the best snapshot and returns the reference's result fields. */
int topolow_session_finish(topolow_session* s, double* positions_out, int32_t* converged,
                           int32_t* iterations, double* final_mae, double* final_k,
                           char* errbuf, size_t errlen);
/* The convergence checks of the current run so far: 3 doubles per check (iteration, MAE, k after
 * cooling) -- the values behind the reference's verbose lines (src/optimization.cpp:298-301).
 * Waits for the enqueued work.  *n_checks = checks recorded; at most max_checks are copied. */
int topolow_session_check_trace(topolow_session* s, double* out, int32_t max_checks, int32_t* n_checks);
/* A cross-validation fold on a loaded whole-problem session (row_begin = 0, row_end = n; edges set; slab or tile
 * Gauss-Seidel schedule, fp32 or f64), outside a run -- before topolow_session_begin or after topolow_session_finish.
 * A fold differs from the full matrix in at most floor(#nonNA / (2 folds)) cells: they are patched on the device and put
 * back afterwards; nothing of size n x n crosses PCIe.  Pairs are in the caller's labels.
 *   hold_out    the listed unordered pairs (any orientation; duplicates, unmeasured pairs and i == j are ignored) become
 *               unmeasured cells for the coming runs, `degrees` (n entries) the degrees.  Both mirrors of the encoded
 *               block, the symmetric sweep's tile-major copy and the f64 delta tiles are patched at those cells and what
 *               they held is saved; rowflags, the threshold bit and the cell count are recomputed on the device (the
 *               sweep's plan is rebuilt only when the threshold bit flips: another kernel instance); a session that
 *               gathers its edge list for the convergence MAE runs on a stable compaction of that list (the full one is
 *               parked on the device).  The session then is what a fresh session loaded with the fold's list would be:
 *               same block, same runs bit for bit.  A second hold_out without a restore: TOPOLOW_ERR_BAD_ARGUMENT;
 *               during a run: TOPOLOW_ERR_BAD_ARGUMENT; a row-block session: TOPOLOW_ERR_UNSUPPORTED.
 *   restore_held_out  puts the saved words, deltas and the full edge list back, with the full matrix's `degrees`: block,
 *               tile-major copy, flags and cell count are bit for bit what they were.
 *   score_pairs sum |truth - ||p_i - p_j||| and the number of pairs on the positions topolow_session_finish restores (the
 *               device's best snapshot: finish may be called with positions_out = NULL, nothing is downloaded).
 *               Distances and sums in f64 whatever the session's precision; deterministic (one partial per workgroup,
 *               summed in index order); i == j counts with distance 0, as the batch call's holdout_* fields. */
int topolow_session_hold_out(topolow_session* s, const int32_t* pair_i, const int32_t* pair_j, int64_t n_pairs,
                             const int32_t* degrees, char* errbuf, size_t errlen);
int topolow_session_restore_held_out(topolow_session* s, const int32_t* degrees, char* errbuf, size_t errlen);
int topolow_session_score_pairs(topolow_session* s, const int32_t* pair_i, const int32_t* pair_j, const double* truth,
                                int64_t n_pairs, double* sum_abs, int64_t* count, char* errbuf, size_t errlen);
/* Per-kernel timing for roofline accounting: while enabled, every slab-stage launch and
 * every convergence check is bracketed by HIP events on the session stream.
 * topolow_session_profile waits for the stream, returns the summed durations (ms) and launch
 * counts since profiling was enabled, and resets them. */
int topolow_session_set_profiling(topolow_session* s, int32_t enable);
/* Of the stage launches recorded so far, those that also reduced a convergence check's MAE (one-stage
 * iterations: the check is fused into the next iteration's sweep) -- summed duration (ms) and count.  Does
 * not reset anything: ask before topolow_session_profile, whose stage figures include these launches. */
int topolow_session_profile_fused(topolow_session* s, double* fused_ms, int64_t* fused_launches, char* errbuf,
                                  size_t errlen);
/* Iterations that ran as a symmetric sweep + apply (csrc/relax_symm.h) since profiling was enabled: their HIP-event
 * time, the plain ones and those whose sweep also reduced a check's MAE apart.  Not included in the two calls above. */
int topolow_session_profile_symmetric(topolow_session* s, double* plain_ms, int64_t* plain_iterations, double* fused_ms,
                                      int64_t* fused_iterations, char* errbuf, size_t errlen);
int topolow_session_profile(topolow_session* s, double* stage_ms, int64_t* stage_launches,
                            double* check_ms, int64_t* checks, char* errbuf, size_t errlen);
/* external != 0: the session launches on the caller's stream `hip_stream` (a hipStream_t; NULL
 * is the device's default stream, which is what torch uses unless told otherwise), so its
 * kernels are ordered with the caller's copies and collectives; the caller keeps ownership.
 * external == 0: back to the session's private non-blocking stream. */
int topolow_session_set_stream(topolow_session* s, void* hip_stream, int32_t external);
/* HIP stream (hipStream_t) the session launches on, for event timing by the caller. */
void* topolow_session_stream(topolow_session* s);
/* 1 when the convergence MAE is reduced from the encoded block (the edge list was verified to be
 * exactly its measured cells), 0 when it gathers the caller's edge list. */
int32_t topolow_session_uses_dense_mae(const topolow_session* s);
/* Number of slab-stage kernel launches so far, and the algorithmic bytes one iteration
 * moves (4*rows*n + 8*n*ndim + 4*n). */
int64_t topolow_session_stage_launches(const topolow_session* s);
/* Convergence checks of the current run whose controller step went out in a symmetric apply's launch instead of a
 * controller launch of its own (one-stage symmetric iterations; 0 under TOPOLOW_CHECK_IN_APPLY=0). */
int64_t topolow_session_checks_in_apply(const topolow_session* s);
int64_t topolow_session_bytes_per_iteration(const topolow_session* s);

/* ---------------------------------------------------------------------------------------
 * Row-sharded building blocks (one process per GPU; the all-gather between stages is the
 * caller's, e.g. torch.distributed/RCCL).  d_pos_* are device pointers to n x ndim
 * row-major positions in the session's precision.
 * ------------------------------------------------------------------------------------- */
/* Iteration body of the session: TOPOLOW_SCHEDULE_SLAB (default) or TOPOLOW_SCHEDULE_GS = exact
 * Gauss-Seidel across workgroups in tile-tournament order (whole-problem sessions only). */
int topolow_session_set_schedule(topolow_session* s, int32_t schedule);
/* Visiting order of the tile Gauss-Seidel schedule for iteration `iter` (as topolow_gs_pair_order). */
int64_t topolow_tilegs_pair_order(int32_t n, uint64_t seed, int32_t iter, int32_t* pairs_out);
/* Rows a caller-owned position buffer must hold: roundup4(n).  Rows [n, roundup4(n)) are the
 * phantom points of the padding columns and must be (1e18, 0, ..., 0) (1e150 in f64 sessions) in
 * BOTH ping-pong buffers; stages never write them. */
int32_t topolow_session_position_rows(const topolow_session* s);
/* Coordinates per point in such a buffer: ndim up to 10, 12 for ndim 11 and 12, 16 for ndim 13..16 (the
 * kernels are instantiated for 1..10, 12 and 16 coordinates; extra coordinates must be, and stay, zero). */
int32_t topolow_session_position_dim(const topolow_session* s);
/* Launches stage `stage` of iteration `iter` (0-based) for the session's row block: reads
 * all n positions from d_pos_in, writes rows [row_begin,row_end) of d_pos_out. */
int topolow_session_stage(topolow_session* s, const void* d_pos_in, void* d_pos_out,
                          int32_t iter, int32_t stage, int32_t n_stages, double k,
                          char* errbuf, size_t errlen);
/* The multi-process form of the convergence check (one process per GPU, the caller owns the
 * collectives): check_partial reduces this block's share of the measured pairs on d_pos into two
 * doubles (sum, count) at the DEVICE address d_out2; the caller all-reduces them (RCCL) and hands the
 * totals to controller_step, which runs the reference's controller (src/optimization.cpp:303-357) on
 * the device -- snapshot, counters, stop flag -- exactly as the session's own loop does.  Nothing
 * here waits for the device.  Valid between topolow_session_begin and topolow_session_finish. */
int topolow_session_check_partial(topolow_session* s, const void* d_pos, double* d_out2, char* errbuf,
                                  size_t errlen);
int topolow_session_controller_step(topolow_session* s, const double* d_total2, const void* d_pos,
                                    int32_t iter1, double k_after, char* errbuf, size_t errlen);
/* The fused form of a check for one-stage iterations: the ONE stage of iteration `iter` (0-based), which
 * also reduces this block's share of the convergence MAE of the positions it READS (d_pos_in: the previous
 * iteration's result, i.e. the previous iteration's check) into the two doubles at d_out2 -- no separate
 * pass over the block.  The caller all-reduces d_out2 and calls controller_step with d_pos_in and the
 * previous iteration's number.  topolow_session_can_fuse_checks: 1 when the session supports it (fp32,
 * MAE reduced from the block, even row count). */
int32_t topolow_session_can_fuse_checks(const topolow_session* s);
int topolow_session_stage_fused(topolow_session* s, const void* d_pos_in, void* d_pos_out, int32_t iter,
                                double k, double* d_out2, char* errbuf, size_t errlen);
/* ONE-stage iterations of a row-sharded run as the SYMMETRIC sweep sharded over the processes (one per GPU; fp32,
 * ndim 2..10, >= 7168 points: csrc/relax_symm.h, relax_symm_wide.h).  Every unordered pair is visited once instead of twice (reference
 * src/optimization.cpp:198-283 visits each pair once and moves both ends), so a rank reads half the bytes of its
 * row-owner sweep.  Rank r of P owns SEGMENT r of the tile list of the upper triangle (equal tile counts), not a
 * row block, so the caller first brings the rows that hold the segment's tiles together:
 *   topolow_symm_segment_rows   host only: rows [*row_first, *row_end) of the matrix hold segment `segment` of
 *                               `n_segments`; returns 0 when a problem of n points has too few tiles to cut
 *   topolow_session_degree_terms  device float[n]: degree + 1 per point (reference :137-140); a row-block session
 *                               knows its own rows' -- the caller completes the array over the ranks (all-gather)
 *   topolow_session_symm_segment_build  d_rows: device words of those rows, n_rows x topolow_session_encoded_ld(s),
 *                               row-major as in the owners' blocks (topolow_session_encoded_ptr; the caller moved
 *                               them, e.g. RCCL send/recv); any_threshold: some rank's block holds threshold codes.
 *                               Builds the tile-major copy of the segment and the sweep's buffers; d_rows may be
 *                               freed on return.  TOPOLOW_ERR_UNSUPPORTED when the session cannot take the path.
 * and then, per one-stage iteration `iter` (0-based), between topolow_session_begin and _finish:
 *   topolow_session_symm_segment_sweep  reads all n positions of d_pos_in, sweeps the segment and leaves the
 *                               segment's share of every point's move in the session's moves buffer
 *                               (topolow_session_symm_moves: device float[n][ndim]); d_out2 != NULL: also the
 *                               segment's share of the MAE of d_pos_in, as topolow_session_stage_fused does.  The
 *                               share is reduced over the block's measured cells, so d_out2 != NULL is refused
 *                               (TOPOLOW_ERR_UNSUPPORTED, nothing launched) unless
 *                               topolow_session_can_fuse_segment_checks: fp32, TOPOLOW_FUSE_CHECKS not 0, and the
 *                               edge list verified to be the block's measured cells
 *                               (topolow_session_uses_dense_mae) -- no even-rows rule, unlike
 *                               topolow_session_can_fuse_checks.  The ranks must agree (a collective minimum of the
 *                               query): a rank that cannot keeps topolow_session_check_partial, and then all do
 *   (the caller sums the moves buffer over the ranks in place -- ONE all-reduce of n x ndim floats, 600 KB at
 *    BASELINE config 4 -- and d_out2 as for stage_fused)
 *   topolow_session_symm_segment_apply  d_pos_out[i] = d_pos_in[i] + moves[i] for ALL n points: every rank holds
 *                               the same sums, so every rank holds the same positions and no gather follows.
 * Nothing here waits for the device (build does, once). */
int32_t topolow_symm_segment_rows(int32_t n, int32_t segment, int32_t n_segments, int32_t* row_first,
                                  int32_t* row_end);
/* 1 when the session can take the path cut into n_segments (fp32 slab schedule, ndim 2..10, size gate, targets loaded). */
int32_t topolow_session_symm_segment_eligible(const topolow_session* s, int32_t n_segments);
/* 1 when topolow_session_symm_segment_sweep may reduce a check (d_out2 != NULL) on this session. */
int32_t topolow_session_can_fuse_segment_checks(const topolow_session* s);
float* topolow_session_degree_terms(topolow_session* s);
/* 1 when some target of the session's block carries a threshold code ('>' / '<'): the any_threshold of the ranks is
 * the OR of these. */
int32_t topolow_session_has_thresholds(const topolow_session* s);
int topolow_session_symm_segment_build(topolow_session* s, int32_t segment, int32_t n_segments, const void* d_rows,
                                       int32_t row_first, int32_t n_rows, int32_t any_threshold, char* errbuf,
                                       size_t errlen);
float* topolow_session_symm_moves(topolow_session* s);
int topolow_session_symm_segment_sweep(topolow_session* s, const void* d_pos_in, int32_t iter, double k,
                                       double* d_out2, char* errbuf, size_t errlen);
int topolow_session_symm_segment_apply(topolow_session* s, const void* d_pos_in, void* d_pos_out, int32_t iter,
                                       char* errbuf, size_t errlen);
/* First iteration (1-based) at which one of this block's rows became non-finite, 0 = none. Waits. */
int topolow_session_first_nonfinite(topolow_session* s, int32_t* iteration);
/* Partial edge error of this session's edge list on d_pos: (sum, count). Synchronous. */
int topolow_session_edge_error(topolow_session* s, const void* d_pos, double* sum,
                               int64_t* count, char* errbuf, size_t errlen);

/* ---------------------------------------------------------------------------------------
 * ONE embedding row-sharded over several GPUs from ONE process (BASELINE config 4: the R host is a
 * single process, reference src/RcppExports.cpp:16-39).  Block b owns a contiguous row block of the
 * encoded matrix and moves its own points; a stage kernel stores its updated rows straight into the
 * position buffers of all blocks (peer stores over xGMI), blocks meet at HIP-event barriers, and the
 * convergence controller is replicated from per-block (sum, count) partials -- no host round trip
 * per stage or per check (the engine: csrc/topolow_relax.hip; its sharded sweep: csrc/topolow_symm.hip).  Results equal the one-session run of the
 * same seed: positions bit for bit, the MAE to rounding (its partial sums are grouped by block) -- on
 * the multi-stage iterations and wherever the row-owner kernel runs.  ONE-stage iterations of fp32 runs with
 * ndim 2..10 and >= 7168 points run as the symmetric sweep sharded over the sessions (csrc/relax_symm.h): session b
 * sweeps segment b of the tile list of the upper triangle (equal tile counts; gathered once from all row blocks),
 * folds its partials per point and stores them into the inbox of the session that owns the point; behind the
 * barrier the owners move their points and store them into every session's positions (two barriers per
 * iteration).  Against one block: positions to the fp32 summation band (2e-5 of the coordinate scale per iteration),
 * every check's MAE to 2e-6, same verdicts (tests/test_gpu_sharded_native.py); TOPOLOW_SHARD_SYMMETRIC=0 keeps
 * the row-owner sweeps.
 * ------------------------------------------------------------------------------------- */
typedef struct topolow_shard_stats {
  int32_t blocks, iterations_run, n_checks;
  int32_t groups;                /* host threads / streams: blocks that share a GPU share one */
  double loop_seconds;           /* host wall time of the relaxation loop, all blocks */
  double total_seconds;          /* including session creation, upload, encode, download */
  double stage_kernel_seconds;   /* first GPU: summed durations of its blocks' stage kernels (HIP events) */
  double check_kernel_seconds;   /* first GPU: error passes + partial exchange + controllers */
  int64_t stage_launches;        /* block 0 */
  int64_t exchanges;             /* stage and check boundaries (an event barrier when groups > 1) */
  /* Measurement aid, IN and out (topolow_sessions_run_sharded only): when > 0 on entry, the GPUs are
   * drained once these iterations have run and `timed_seconds` covers the rest of the loop -- the
   * steady state without the 16-stage iterations of the unfolding phase. */
  int32_t warmup_iterations;
  int32_t symmetric_segments;    /* > 0: one-stage iterations ran as the symmetric sweep sharded over this many sessions */
  double timed_seconds;
  int64_t reserved[2];
} topolow_shard_stats;

/* Row block `block` of `blocks` over n rows: contiguous, whole 8-row workgroups; returns how many
 * blocks hold at least one row (<= blocks; trailing blocks of a small problem are empty and
 * dropped).  block < 0: only the count. */
int32_t topolow_shard_rows(int32_t n, int32_t blocks, int32_t block, int32_t* row_begin, int32_t* row_end);

/* The `.Call` payload row-sharded over opt->devices[0 .. n_devices) (an ordinal may repeat: several
 * row blocks on one GPU).  Arguments and outputs as topolow_optimize_layout_exact;
 * dissimilarity_matrix and threshold_matrix may both be NULL: the edge list then IS the matrix (large
 * problems never build the dense n x n host matrices).  Slab schedule only. */
int topolow_optimize_layout_exact_sharded(
    const double* initial_positions, int32_t n, int32_t ndim,
    const double* dissimilarity_matrix, const int32_t* threshold_matrix,
    const int32_t* degrees,
    const int32_t* edge_i, const int32_t* edge_j, const double* edge_dist,
    const int32_t* edge_thresh, int64_t n_edges,
    int32_t n_iter, double k0, double cooling_rate, double c_repulsion,
    double relative_epsilon, int32_t convergence_window, int32_t convergence_check_freq,
    int32_t verbose, const topolow_options* opt,
    double* positions_out, int32_t* converged, int32_t* iterations, double* final_mae,
    double* final_k, topolow_shard_stats* stats, char* errbuf, size_t errlen);

/* The same run over sessions the caller has created and loaded itself (targets, degrees and each
 * block's share of the MAE edges -- pair {lo, hi} belongs to the block that owns lo when lo + hi is
 * even and hi when it is odd): row blocks that tile [0, n) in order, slab schedule, one precision.
 * profile != 0: block 0's kernels are bracketed by timing events (fills the *_kernel_seconds). */
int topolow_sessions_run_sharded(topolow_session** sessions, int32_t count, const double* initial_positions,
                                 int32_t n_iter, double k0, double cooling_rate, double c_repulsion,
                                 double relative_epsilon, int32_t convergence_window,
                                 int32_t convergence_check_freq, uint64_t seed, int32_t slab_stages,
                                 int32_t (*interrupt_cb)(void* user), void* interrupt_user, int32_t profile,
                                 double* positions_out, int32_t* converged, int32_t* iterations,
                                 double* final_mae, double* final_k, topolow_shard_stats* stats,
                                 char* errbuf, size_t errlen);

/* ---------------------------------------------------------------------------------------
 * Host-side helpers exported for tests and integrators (no GPU needed).
 * ------------------------------------------------------------------------------------- */
/* Slab plan of iteration `iter`: writes n_stages x 4 int32 (r0_begin, r0_end, r1_begin,
 * r1_end; second range empty unless the slab wraps) in execution order; returns n_stages. */
int32_t topolow_slab_plan(int32_t n, int32_t slab_stages, uint64_t seed, int32_t iter,
                          int32_t* ranges_out, int32_t max_stages);
/* Stage count the adaptive policy picks for spring constant k in ndim dimensions: the smallest power of two
 * with k / stages <= min(3, ndim) (a stage is a Jacobi step, stable for k / stages < 2 ndim). */
int32_t topolow_slab_stages_for_k(double k, int32_t ndim);
/* 2-, 4- and 8-stage iterations of sessions that take the symmetric sweep (slab schedule, ndim 2..10 in fp32, 2..6 in f64, >= 7168
 * points, whole matrix) run as symmetric sweeps that split the PAIRS: the (randomly labelled) points are cut into S slabs
 * of labels [first_label[q], first_label[q + 1]) and stage st sweeps the pairs between slabs a and b with
 * (a + b) mod S == st, so every point meets one slab of partners per stage, as in the row-owner form, and both ends of a
 * pair move in the same stage, as in the reference.  topolow_symm_stage_bounds: the S + 1 slab boundaries (0 when the
 * problem is too small or S is not 2, 4, 8); topolow_symm_stage_order: the order of the stages in iteration `iter`.
 * TOPOLOW_SYMMETRIC_TWO_STAGE=0 keeps the row-owner stages. */
int32_t topolow_symm_stage_bounds(int32_t n, int32_t stages, int32_t* first_label);
int32_t topolow_symm_stage_order(uint64_t seed, int32_t iter, int32_t stages, int32_t* order);
/* Host only: per tile-row R (64 points) of an n-point problem, what stage `stage` of a `stages`-stage iteration sweeps
 * and sums -- rows_out[4 R ..] = (j0, j1, rp0, rp1): the column blocks [j0, j1) of 32 points that the stage sweeps in
 * tile-row R (empty when j0 >= j1), and the tile-rows [rp0, rp1) whose column sums of that stage belong to the points
 * of tile-row R.  Returns the number of tile-rows (rows_out may be NULL), -1 where topolow_symm_stage_bounds gives 0. */
int32_t topolow_symm_stage_rows(int32_t n, int32_t stages, int32_t stage, int32_t* rows_out);
/* Host only: the plan the symmetric sweep of an n-point problem loads for a grid of n_waves waves (4 per workgroup) --
 *   stages == 0, n_segments <= 1   the whole upper triangle;
 *   stages in {2, 4, 8}            the tiles of stage `stage` (n_segments <= 1);
 *   n_segments >= 2                segment `segment` of the sharded sweep: tiles [total b / P, total (b + 1) / P).
 * units_out: 4 int32 per unit (tile_row, j0, j1, tile0): the column blocks [j0, j1) of tile-row tile_row, the first of
 * them at index tile0 of the plan's tile-major copy; at most max_units units are written.  wave_first_out: n_waves + 1
 * entries, wave w sweeps the units [wave_first[w], wave_first[w + 1]).  Either may be NULL (to size the other).
 * Returns the number of units, -1 for arguments no session would plan with. */
int32_t topolow_symm_plan(int32_t n, int32_t n_waves, int32_t stages, int32_t stage, int32_t segment, int32_t n_segments,
                          int32_t* units_out, int32_t max_units, int32_t* wave_first_out);
/* Workgroups of the symmetric sweep this session has built (whole triangle or segment), 0 if none: one resident round
 * of the device, or fewer under TOPOLOW_SYMMETRIC_GRID (a test knob). */
int32_t topolow_session_symm_grid(const topolow_session* s);
/* Stage count of iteration `iter` (0-based) when slab_stages = 0: the policy above, and at least 16 stages
 * during the first 8 iterations, while the layout unfolds from its start. */
int32_t topolow_slab_stages_at(int32_t iter, double k, int32_t ndim);
/* Visiting order of the GS tournament schedule for iteration `iter`: n(n-1)/2 pairs
 * (a,b) as 2 int32 each, in an order equivalent to what the kernel executes. */
int64_t topolow_gs_pair_order(int32_t n, uint64_t seed, int32_t iter, int32_t* pairs_out);
/* fp32 target encoding used in HBM: value with the 2 low mantissa bits replaced by the
 * threshold code (0 exact, 1 ">", 2 "<", 3 skip); +Inf = unmeasured. */
uint32_t topolow_encode_target(double dissimilarity, int32_t threshold_code);
int64_t topolow_encoded_index(int32_t row_in_block, int32_t column, int32_t ld);
double topolow_decode_target(uint32_t bits, int32_t* threshold_code);
/* Convergence controller (reference src/optimization.cpp:303-357) on a scripted MAE
 * sequence; same code the device runs. */
int topolow_controller_script(const double* mae_seq, const int32_t* iter_seq,
                              const double* k_seq, int32_t n_obs, double k0, int32_t window,
                              double eps, int32_t* stopped_at_obs, int32_t* snapshot_flags,
                              double* best_mae, double* best_k, int32_t* best_iter);
const char* topolow_relax_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TOPOLOW_RELAX_H */
