// topolow_amd/csrc/topolow_prep.h -- the prepared handle as the library's sources see it: struct topolow_layout_prep
// and what it is made of, the pinned staging and the stream pipe the post-metrics share with the handle's entries, and
// the functions that cross a source boundary: between the handle's five sources (topolow_prep.hip: create, fetch and
// the entries that run from a handle; topolow_prep_graph.hip: connectivity, sub-handles, degrees, pruning;
// topolow_spectrum.hip; topolow_prep_fold.hip: folds, CV sweep, fit report; topolow_fit_bins.hip: the fit's binned
// diagnostics) and to topolow_relax.hip and
// topolow_post.hip.  Types, declarations and a few host helpers; the kernels live in the sources.
#pragma once

#include "topolow_session.h"
#include "relax_prep_types.h"

namespace {

// layout prep: an allocation that fails is "this problem is too large for the dense form", not a HIP error
template <typename T>
void prep_alloc(DevBuf<T>& buf, size_t count, const char* what) {
  try {
    buf.alloc(count);
  } catch (const HipError& e) {
    (void)hipGetLastError();
    throw HipError{TOPOLOW_ERR_UNSUPPORTED, "layout prep: no device memory for " + std::string(what) + " (" +
                                                std::to_string(count * sizeof(T)) + " bytes): " + e.msg};
  }
}

// Counts per column -> exclusive offsets, off[0 .. n]; returns the total.
int64_t prep_offsets(const int32_t* per_col, size_t n, int64_t* off) {
  off[0] = 0;
  for (size_t j = 0; j < n; ++j) off[j + 1] = off[j] + per_col[j];
  return off[n];
}

// The host's side of a radix select over prep_order_key (the median of the spectrum, the fit report's order statistics).
// Rank `rank` (0-based) among the keys counted in hist: its digit; rank becomes the rank within that digit.
unsigned spec_pick_digit(const unsigned long long* hist, unsigned long long& rank) {
  unsigned digit = 0;
  while (digit < 255 && rank >= hist[digit]) rank -= hist[digit++];
  return digit;
}

double spec_key_value(unsigned long long key) {
  const unsigned long long bits = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
  double v;
  std::memcpy(&v, &bits, 8);
  return v;
}

constexpr size_t kPrepChunkBytes = (size_t)32 << 20;
constexpr int kPrepSlots = 3;

constexpr int kPostSlots = 3;
constexpr int kPostDefaultStaging = TOPOLOW_POST_STAGING_PINNED;

// pageable <-> pinned on up to 16 host threads (one per MB)
void post_host_copy(void* dst, const void* src, size_t bytes) {
  host_parallel(bytes, (size_t)1 << 20, [&](size_t lo, size_t hi) {
    memcpy(static_cast<char*>(dst) + lo, static_cast<const char*>(src) + lo, hi - lo);
  });
}

}  // namespace

#pragma GCC visibility push(hidden)

struct PinBuf {
  void* p = nullptr;
  void alloc(size_t bytes) { HIP_TRY(hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault)); }
  ~PinBuf() { if (p) (void)hipHostFree(p); }
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
};

// The three streams and the events that order the slots.  Destroyed before the buffers it worked on (declare it after
// them): the destructor waits for the streams first, so nothing is in flight when a buffer goes.
struct PostPipe {
  hipStream_t up = nullptr, run = nullptr, down = nullptr;
  hipEvent_t up_done[kPostSlots] = {}, run_done[kPostSlots] = {}, down_done[kPostSlots] = {};
  std::vector<hipEvent_t> timing;   // per tile: begin and end of upload, kernel, download (only when asked for)
  void create(int slots, int timed_tiles) {
    HIP_TRY(hipStreamCreateWithFlags(&up, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&run, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&down, hipStreamNonBlocking));
    for (int b = 0; b < slots; ++b) {
      HIP_TRY(hipEventCreateWithFlags(&up_done[b], hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&run_done[b], hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&down_done[b], hipEventDisableTiming));
    }
    timing.assign((size_t)timed_tiles * 6, nullptr);
    for (hipEvent_t& e : timing) HIP_TRY(hipEventCreate(&e));
  }
  void mark(int tile, int which, hipStream_t s) {
    if (!timing.empty()) HIP_TRY(hipEventRecord(timing[(size_t)tile * 6 + which], s));
  }
  void sync() {
    HIP_TRY(hipStreamSynchronize(up));
    HIP_TRY(hipStreamSynchronize(run));
    HIP_TRY(hipStreamSynchronize(down));
  }
  ~PostPipe() {
    for (hipStream_t s : {up, run, down})
      if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
    for (int b = 0; b < kPostSlots; ++b)
      for (hipEvent_t e : {up_done[b], run_done[b], down_done[b]})
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : timing)
      if (e) (void)hipEventDestroy(e);
  }
  PostPipe() = default;
  PostPipe(const PostPipe&) = delete;
  PostPipe& operator=(const PostPipe&) = delete;
};

// The matrix of a post-metrics pass when it is resident on the device already (topolow_layout_prep_post_metrics): the
// handle's buffers; a tile is then a run of the buffer's lines and nothing is uploaded.
struct PostResident {
  const double* vals;
  const int8_t* codes;   // nullable
  const int32_t* ord;    // nullable: the input order is kept
};

// topolow_post.hip: the pipeline of topolow_post_metrics_ex, and of topolow_layout_prep_post_metrics when `resident` is given.
int post_metrics_run(const double* positions, int32_t n, int32_t ndim, const double* values, const int32_t* codes,
                     const PostResident* resident, double* est_distances, double* sum_abs, int64_t* count,
                     int32_t device, int32_t staging, double* phase_seconds, char* errbuf, size_t errlen);

// The host's side of a sums pass (prep_tile_sums), of the full matrix (prep_passes) or a fold's masked one
// (prep_fold_prepare): the buffers the tile kernels write, and what the host reads of them.
template <typename Totals>
struct PrepSums {
  DevBuf<double> part_slow_sum, part_fast_sum, line_sum;
  DevBuf<int32_t> part_slow_cnt, part_fast_cnt, line_cnt;
  DevBuf<uint8_t> diag;
  DevBuf<Totals> totals;
  std::vector<double> sums;      // after fetch(), 2 n each: the slow lines, then the fast lines
  std::vector<int32_t> cnts;
  std::vector<uint8_t> on_diag;  // n: is the diagonal cell counted?
  Totals tot;
  void alloc(int n) {
    const size_t N = (size_t)n, nb = (N + kPrepTile - 1) / kPrepTile;
    for (auto* b : {&part_slow_sum, &part_fast_sum}) prep_alloc(*b, nb * N, "the partial sums");
    for (auto* b : {&part_slow_cnt, &part_fast_cnt}) prep_alloc(*b, nb * N, "the partial counts");
    prep_alloc(line_sum, 2 * N, "the sums");
    prep_alloc(line_cnt, 2 * N, "the counts");
    prep_alloc(diag, N, "the diagonal flags");
    prep_alloc(totals, 1, "the totals");
  }
  // Behind the tile kernels on `stream`: the partials added per point, all of it sent down; the caller synchronises.
  // Defined in topolow_prep.hip, for PrepTotals and FoldTotals: it launches a kernel of relax_prep.h.
  void fetch(int n, hipStream_t stream);
  // topolow_layout_order_from_sums on the fetched sums, the counts less the diagonal; rows at row_at, columns at col_at.
  int32_t order(int n, size_t row_at, size_t col_at, bool exact_sums, bool negative_or_infinite, int32_t* order_out) const {
    std::vector<int64_t> row_cnt((size_t)n), col_cnt((size_t)n);
    for (size_t q = 0; q < (size_t)n; ++q) {
      row_cnt[q] = (int64_t)cnts[row_at + q] - on_diag[q];
      col_cnt[q] = (int64_t)cnts[col_at + q] - on_diag[q];
    }
    return topolow_layout_order_from_sums(n, sums.data() + row_at, row_cnt.data(), sums.data() + col_at, col_cnt.data(),
                                          exact_sums ? 1 : (negative_or_infinite ? -1 : 0), order_out);
  }
  double numeric_max() const {   // from the totals' max_key (prep_order_key); NaN: there is no non-NA code-0 value
    const uint64_t key = tot.max_key, bits = (key >> 63) ? key & 0x7fffffffffffffffull : ~key;
    double v = NAN;
    if (key != 0) memcpy(&v, &bits, 8);
    return v;
  }
};

// ---- layout prep: order, degrees, edge list and dense fill on the device (R/core.R:269-436) ----
// create(): the matrix goes up in chunks of whole 64-line blocks through pinned staging while the first pass runs on
// the chunks that have arrived; the host applies the ordering rule to the sums; the second pass fills the dense
// matrices and counts the edges per column.  fetch(): the compaction, the reordered copy when asked for, and the
// downloads, through the same pinned staging.  The matrix stays on the device between the two.
struct topolow_layout_prep {
  int n = 0, device = 0;                 // n first: the subset checks of the graph entries read nothing else of a handle
  bool transposed = false, has_codes = false, declined = false;
  DevBuf<double> vals, dense;
  DevBuf<int8_t> codes;
  DevBuf<int32_t> tdense, ord;
  DevBuf<int64_t> edge_off;
  std::vector<int32_t> order, degrees;   // order[0] == -1: the input order is kept
  int64_t n_edges = 0;
  double phase_seconds[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  // What the resident entries add (topolow_session_load_prepared, topolow_layout_prep_optimize, _post_metrics):
  DevBuf<int32_t> ddeg;                  // `degrees` on the device: a session gathers its degree terms from it
  bool compacted = false;                // the edge list below is written (prep_compact_edges: at most once per handle)
  DevBuf<int32_t> edge_i, edge_j, edge_thresh;
  DevBuf<double> edge_dist;
  double resident_seconds[3] = {0.0, 0.0, 0.0};   // last load_prepared, last optimize (whole call), last post_metrics
  // What the ordering rule needs to know of the data (create()'s first pass): conservative for any subset of the cells,
  // so a fold's masked sums are judged with them (topolow_layout_prep_fold).
  bool exact_sums = false;
  bool negative_or_infinite = false;
  // The last topolow_layout_prep_connectivity (relax_prep_graph.h): rounds launched; seconds of the bit pass, the rounds.
  int graph_rounds = 0;
  double graph_seconds[2] = {0.0, 0.0};
  // Cross-validation folds prepared from the handle (relax_prep_fold.h), allocated by the first fold.
  struct Fold {
    bool ready = false;
    bool symmetry_known = false, symmetric = false;   // fold_symmetry_kernel ran / what it found
    hipStream_t stream = nullptr;          // topolow_layout_prep_fold's own; a sweep works on its session's stream
    size_t mask_words = 0;
    DevBuf<uint32_t> mask;                 // one bit per cell; all zero between folds
    PrepSums<FoldTotals> sums;             // of the masked matrix; its totals serve fold_symmetry_kernel too
    DevBuf<int32_t> col_counts;            // 2 n: held-out pairs per column, then scored cells per column
    DevBuf<int64_t> offsets;               // 2 (n + 1): their prefix sums
    DevBuf<long long> picks;
    DevBuf<int32_t> order;                 // the fold's order, where the scored cells are gathered through it
    DevBuf<int32_t> pair_i, pair_j, score_r, score_c;   // caller's labels; the scored cells as (row, column)
    DevBuf<int> score_i, score_j;          // the points the scored cells are scored against (topolow_layout_prep_fold)
    DevBuf<double> score_truth;
    double seconds[4] = {0.0, 0.0, 0.0, 0.0};   // last sweep, summed over its folds: prepare, hold out, score, restore
  } fold;
  ~topolow_layout_prep() {
    if (fold.stream) (void)hipStreamDestroy(fold.stream);
  }
};

// ---- defined in topolow_prep.hip, called by topolow_session_load_prepared (topolow_relax.hip) and the fit report ----
void prep_compact_edges(topolow_layout_prep* p, hipStream_t stream);
int prep_check_usable(const topolow_layout_prep* p, char* errbuf, size_t errlen);

// How the lines of an n x n matrix arrive on the device: in chunks of whole 64-line blocks of about kPrepChunkBytes.
struct PrepChunks {
  int chunk_lines, n_chunks, slots;
  size_t chunk_cells;
  explicit PrepChunks(int n) {
    const size_t N = (size_t)n;
    const int nb = (n + kPrepTile - 1) / kPrepTile;
    chunk_lines = (int)std::min<size_t>(
        (size_t)nb * kPrepTile, std::max<size_t>(kPrepTile, kPrepChunkBytes / (N * 8) / kPrepTile * kPrepTile));
    n_chunks = (n + chunk_lines - 1) / chunk_lines;
    slots = std::min(kPrepSlots, n_chunks);
    chunk_cells = (size_t)std::min(chunk_lines, n) * N;
  }
};

// ---- defined in topolow_prep.hip, called by topolow_layout_prep_subsample (topolow_prep_graph.hip) as well ----
bool prep_order_in_ok(int32_t preserve_order, const int32_t* order_in, int n, char* errbuf, size_t errlen);
void prep_passes(topolow_layout_prep* p, int32_t preserve_order, const int32_t* order_in, topolow_layout_prep_info* info,
                 double t0, const PrepChunks& g, const std::function<void(PostPipe&, int, int, int)>& arrive);

// ---- defined in topolow_prep_fold.hip with the fit report, called by the binned diagnostics (topolow_fit_bins.hip) as well ----
// What the fit kernels read: the handle's buffers, the positions one row per point, the fold mask where picks were given.
struct FitInputs {
  const double* pos;
  const double* vals;
  const int8_t* codes;
  const int32_t* ord;
  const uint32_t* mask;
  hipStream_t stream;
};
int fit_check_arguments(const char* entry, const topolow_layout_prep* p, const double* positions, int32_t ndim,
                        const int64_t* picks, int64_t n_picks, const void* out, char* errbuf, size_t errlen);
int fit_check_series(const char* entry, int32_t series, char* errbuf, size_t errlen);
// The positions go up, the picks are marked in the handle's fold mask, body(inputs) runs, and the mask is empty again
// when this returns, whatever body threw.
int fit_run(topolow_layout_prep* p, const double* positions, int32_t ndim, const int64_t* picks, int64_t n_picks,
            char* errbuf, size_t errlen, const std::function<void(const FitInputs&)>& body);

#pragma GCC visibility pop
