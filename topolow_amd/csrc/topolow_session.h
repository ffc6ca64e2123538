// topolow_amd/csrc/topolow_session.h -- the session as the library's sources see it: struct topolow_session, the
// device buffer it is made of, and the few session functions another source calls.  Types, declarations and small
// stateless helpers only; the kernels and what launches them live in the session's four sources: topolow_relax.hip (the
// session, its loop, the stage and check kernels, the row-sharded engine), topolow_symm.hip (the symmetric sweep),
// topolow_tilegs.hip (tile Gauss-Seidel) and topolow_cv.hip (hold-out and scoring).  What is defined once and called
// from another source has hidden visibility, so the library exports the C ABI of include/topolow_relax.h and nothing else.
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <cstdlib>
#include <array>
#include <atomic>
#include <deque>
#include <functional>
#include <future>
#include <limits>
#include <mutex>
#include <string>
#include <memory>
#include <thread>
#include <vector>

#include "../../include/topolow_relax.h"
#include "relax_common.h"
#include "relax_host.h"
#include "relax_symm_plan.h"

using namespace topolow;

#pragma GCC visibility push(hidden)

// The types below are members of the two structs the C ABI hands out, so they are ONE type in every source.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  void alloc(size_t count) {
    release();
    if (count == 0) count = 1;
    HIP_TRY(hipMalloc((void**)&p, count * sizeof(T)));
    n = count;
  }
  void release() {
    if (p) { (void)hipFree(p); p = nullptr; n = 0; }
  }
  ~DevBuf() { release(); }
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
};

// Small stateless helpers, defined here with internal linkage (as relax_host.h's).
namespace {

constexpr int kMaxDim = 64;        // 1..16: the tuned kernels; 17..64: the plain stage kernel (relax_kernels.h: slab_stage_wide_kernel)
constexpr int kMaxTunedDim = 16;
// kernels are instantiated for 1..10, 12, 16, 32 and 64 coordinates; 11 runs as 12, 13..15 as 16, 17..31 as 32 and
// 33..63 as 64 with the extra coordinates held at exactly zero (a zero coordinate adds 0 to every distance and
// receives 0 of every move)
constexpr int kernel_dim(int ndim) { return ndim <= 10 ? ndim : (ndim <= 12 ? 12 : (ndim <= 16 ? 16 : (ndim <= 32 ? 32 : 64))); }

// The symmetric sweep's size gate (topolow_symm.hip: sym_shape_ok; a session reads TOPOLOW_SYMMETRIC_MIN_N over it at creation).
constexpr int kSymMinPoints = 7168;   // below ~7000 points a resident wave gets fewer than 8 tiles and the row-owner sweep is faster (tests/study/symm_crossover.py; at ndim 10 the two meet near 4 100 points and the sweep leads by 1.11 at 6 144, 1.27 at 7 168: the gate stays, profiles/r05_symm_wide.txt)

int select_device(int device) {
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    throw HipError{TOPOLOW_ERR_NO_DEVICE,
                   "no HIP device available (libtopolow_relax has no CPU fallback)"};
  if (device < 0) {
    HIP_TRY(hipGetDevice(&device));
  } else {
    if (device >= count) throw HipError{TOPOLOW_ERR_NO_DEVICE, "HIP device ordinal out of range"};
    HIP_TRY(hipSetDevice(device));
  }
  return device;
}

double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

template <typename T>
void grow_buf(DevBuf<T>& b, size_t count) { if (b.p == nullptr || b.n < count) b.alloc(count); }

}  // namespace

// A convergence check whose error pass has not been launched yet: when the NEXT iteration is a single
// stage, that stage's kernel reduces the MAE of the positions it reads (exactly this check's positions)
// on its way (slab_stage_pipe_kernel<..., ERR = true>) and the separate 2 N^2-byte pass is dropped.
// beside: the session's own loop runs it on the check stream (launch_check).
// in_apply: the check rides on a one-stage symmetric sweep and its controller step runs in that iteration's apply launch
// (relax_symm.h: SymApplyCheck): no check stream, no stream marker, no held buffer.
struct PendingCheck {
  bool active = false; int iter1 = 0; double k_after = 0.0; int buf = -1; bool beside = false; bool in_apply = false;
};

struct topolow_session {
  int n = 0, dim = 0, udim = 0, row_begin = 0, row_end = 0, ld = 0;   // dim: coordinates the kernels carry, udim: the caller's ndim
  int precision = TOPOLOW_PRECISION_F32;
  bool exact = false;           // TOPOLOW_PRECISION_F64_EXACT: an F64 session whose kernels read word + delta (denc)
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t own_stream = nullptr;
  // Convergence checks run beside the next iteration (slab schedule, own stream, not profiling):
  // the error pass and the controller go to `check_stream` and read the position buffer the
  // iteration ended in, which the stage kernels leave alone (`held`) until the next check.
  hipStream_t check_stream = nullptr;
  hipEvent_t ev_iter_done = nullptr, ev_check_done = nullptr;
  int held = -1;
  PendingCheck pcheck;
  bool fuse_checks = true;      // TOPOLOW_FUSE_CHECKS=0: always the separate pass
  bool serial_checks = false;   // TOPOLOW_SERIAL_CHECKS=1: keep every check on the main stream
  bool check_in_apply = true;   // TOPOLOW_CHECK_IN_APPLY=0: a check fused into a symmetric sweep keeps the separate controller
  int checks_launched = 0;      // checks of the current run enqueued so far (the mailbox's n_checks counts those that ran)
  long long checks_in_apply = 0;   // ... those of them whose controller step went out in an apply's launch

  // Session labels.  With a relabelling (topolow_session_set_relabel) the session stores point
  // perm[q] of the caller as its point q, so that a slab -- a run of consecutive session labels -- is
  // a random subset of the caller's points instead of a run of consecutive ones (which lie next to
  // each other on the reference's random-walk start, R/core.R:407-415, and often in the data's own
  // order).  Every entry point that takes or returns host arrays speaks the CALLER's labels.
  std::vector<int> perm, inv;      // session -> caller, caller -> session; empty = identity
  DevBuf<int> d_perm, d_inv;
  DevBuf<uint32_t> enc;
  DevBuf<float> denc;          // exact sessions: fp32 (target - decoded word) per cell of enc, same layout, 0 where unmeasured
  DevBuf<float> gplus;
  DevBuf<unsigned char> rowflags;
  bool any_threshold = true;   // does any row of the block hold a ">" / "<" target?
  unsigned long long block_gen = 0;     // counts the fills of enc (compute_row_flags): enc.p itself never changes
  unsigned long long block_cells = 0;   // measured (ordered) cells of the block: 2 x the measured pairs of a whole problem
  int schedule = TOPOLOW_SCHEDULE_SLAB;   // SLAB, or GS = exact tile Gauss-Seidel (relax_tilegs.h)
  DevBuf<int> bperm;
  DevBuf<unsigned char> pos[3];   // stage ping-pong + the buffer a running check reads
  // The two snapshot buffers: the run state names the one that holds the best positions (RunState::best_buf).  A check
  // that rides in an apply's launch has the column blocks copy its positions into the other one (relax_symm.h).
  DevBuf<unsigned char> best[2];
  static int best_index(const RunState& st) { return st.best_buf[st.best_entry & 1] & 1; }
  // ... as the pinned mailbox has it, which every controller step mirrors the run state to: for a caller that has
  // waited for the session's streams
  void* best_now() const { return best[mailbox != nullptr ? best_index(*mailbox) : 0].p; }
  DevBuf<int> ei, ej;
  DevBuf<unsigned char> et;
  DevBuf<int8_t> ec;
  long long n_edges = 0;
  int n_parts = 0;
  bool dense_mae = false;   // edge list verified == measured cells of the encoded block
  bool list_is_block = false;   // ... the verification itself (dense_mae also wants fp32 and ndim <= 16)
  bool dense_parity = false;
  int dense_blocks = 0, dense_grid_x = 0, dense_grid_y = 0;
  DevBuf<double> part_sum;
  DevBuf<unsigned long long> part_cnt;
  DevBuf<RunState> state;
  RunState* mailbox = nullptr;      // pinned host memory
  RunState* mailbox_dev = nullptr;  // device alias of mailbox
  double* trace = nullptr;          // pinned: (iteration, MAE, k) of every check of the current run
  double* trace_dev = nullptr;
  int trace_cap = 0;

  // run parameters
  int n_iter = 0, check_freq = 3, window = 5, fixed_stages = 0;
  double k0 = 0, cooling = 0, c_rep = 0, eps = 1e-4;
  uint64_t seed = 0;
  // host-side progress
  int iters_enqueued = 0;
  double k_host = 0;
  int cur = 0;
  bool host_seen_stop = false;
  bool began = false;
  bool in_run = false;          // between topolow_session_begin and _finish
  long long stage_launches = 0;
  std::deque<hipEvent_t> pending;
  std::vector<hipEvent_t> event_pool;
  // row-sharded engine (topolow_sessions_run_sharded): this block's view of the other blocks
  DevBuf<void*> push_tab[3];           // [b]: the other blocks' position buffer b (device pointers)
  int n_push = 0;
  DevBuf<double> rank_sum;             // one (sum, count) slot per block, written by every block
  DevBuf<unsigned long long> rank_cnt;
  DevBuf<double*> rsum_tab;            // every block's rank_sum / rank_cnt (self included)
  DevBuf<unsigned long long*> rcnt_tab;
  int n_ranks = 0, rank = 0;
  // Symmetric sweep (relax_symm.h, relax_symm64.h): one-stage iterations of a whole-matrix session.
  struct SymState {
    bool allowed = false;          // TOPOLOW_SYMMETRIC != 0 (session creation)
    bool forced = false;           // TOPOLOW_SYMMETRIC=1: also at an ndim whose default is off (sym_dim_default)
    int min_n = 0;                 // size gate (TOPOLOW_SYMMETRIC_MIN_N at session creation; default kSymMinPoints)
    // What the buffers below describe, all of them at once.  hold() enters a state, once a build is complete; invalidate()
    // (the memory stays for the next build) and release() (a build failed: the memory goes too) leave it for kNothing.
    enum class Holds {
      kNothing,
      kTriangle,        // the whole upper triangle of the session's own block (sym_prepare): stage plans may be cut from it
      kRunSegment,      // this session's segment of a run over several row-block sessions (sym_sharded_prepare)
      kCallerSegment,   // topolow_session_symm_segment_build's: one slot, one owner, the caller sums the inbox over the processes
    };
    Holds holds = Holds::kNothing;
    int npad = 0, tiles = 0, grid = 0;   // npad = roundup(n, 64): whole 64-row tiles
    DevBuf<uint32_t> tenc;
    // records, row and column partials in the session's precision (SymRec<DIM> floats or SymRec64<DIM> doubles)
    DevBuf<unsigned char> rec[2], rowpart, colpart;
    int rec_cur = 0, rec_iter = -1;   // rec[rec_cur] holds the records of iteration rec_iter (sym_iteration's cursor; -1 per run)
    DevBuf<float> tdelta;          // f64: exact target - decoded word per cell of tenc: the fused check's MAE is exact
    bool delta_ready = false;      // tdelta is built for what the buffers hold
    int generation = 0;            // counts the builds of the copy: a patch of it is only put back into the build it was made on
    // A sweep plan on the device (relax_symm.h: SymPlan): units, every wave's run of them, per tile-row its units.
    struct Plan {
      DevBuf<SymUnit> units;
      DevBuf<SymRun> runs;
      DevBuf<int2> row_units;
      int n_units = 0;
      void load(const SymPlan& hp) {
        const std::vector<SymRun> hr = hp.runs();
        n_units = (int)hp.units.size();
        units.alloc(std::max<size_t>(hp.units.size(), 1));
        runs.alloc(hr.size());
        row_units.alloc(std::max<size_t>(hp.row_units.size(), 1));
        if (!hp.units.empty())
          HIP_TRY(hipMemcpy(units.p, hp.units.data(), hp.units.size() * sizeof(SymUnit), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(runs.p, hr.data(), hr.size() * sizeof(SymRun), hipMemcpyHostToDevice));
        if (!hp.row_units.empty())
          HIP_TRY(hipMemcpy(row_units.p, hp.row_units.data(), hp.row_units.size() * sizeof(int2), hipMemcpyHostToDevice));
      }
      void release() { units.release(); runs.release(); row_units.release(); n_units = 0; }
    };
    Plan plan;                     // the whole triangle, or this session's segment
    // multi-stage iterations (2, 4, 8 stages) as symmetric sweeps over the tiles of one stage each (relax_symm.h:
    // sym_rr_*): rr[log2 S] holds the S plans, built when an iteration first needs them
    std::vector<Plan> rr[4];
    bool two_stage = true;         // TOPOLOW_SYMMETRIC_TWO_STAGE=0: multi-stage iterations stay on the row-owner kernel
    bool prio = true;              // TOPOLOW_SYM_PRIO=0: the fp32 sweep's waves all stay at issue priority 0
    int rr_min_tiles = 5;          // tiles per resident wave a stage must have (TOPOLOW_SYMMETRIC_STAGE_MIN_TILES; tests: 0)
    int grid_cap = 0;              // > 0: at most this many workgroups (TOPOLOW_SYMMETRIC_GRID; tests: long runs on small problems)
    DevBuf<const uint32_t*> src_tab;   // the row blocks the tile-major copy is gathered from (one: the session's own)
    DevBuf<int> src_row0;
    // the sweep sharded over the row-block sessions of a run (topolow_symm.hip: sym_sharded_*; the engine: topolow_relax.hip): this session's segment
    bool seg_thr = false;          // some session of the run holds threshold targets: the classifying instance
    int seg_first = 0, seg_last = -1;   // tile-rows that hold a tile of the segment
    int seg_slots = 0;             // sessions of the run (slots of an inbox)
    int seg_slot = 0;              // the slot this session's folded partials go to
    DevBuf<float> inbox;           // [seg_slots][npad][ndim]: every session's folded partials of this session's points
    DevBuf<float*> inbox_tab;      // every session's inbox (self included)
    DevBuf<int> own0;              // first row of every session, then n
    // what a run segment was gathered from: every session's enc.p (refilled in place: it never changes) and block_gen
    using Sources = std::vector<std::pair<const void*, unsigned long long>>;
    Sources seg_from;

    void hold(Holds what) { holds = what; }
    // The buffers no longer describe the block: whatever reads them builds them again first.
    void invalidate() {
      holds = Holds::kNothing;
      delta_ready = false;
      rec_iter = -1;
      seg_from.clear();
    }
    // Frees every sweep buffer (a build that failed: the session keeps the row-owner sweep).
    void release() {
      tenc.release(); rec[0].release(); rec[1].release(); rowpart.release(); colpart.release();
      tdelta.release();
      plan.release();
      for (auto& v : rr) v.clear();
      src_tab.release(); src_row0.release();
      inbox.release(); inbox_tab.release(); own0.release();
      invalidate();
    }
  } sym;
  // A fold held out of the resident block (topolow_session_hold_out, relax_cv.h): the pairs in session labels, what
  // their cells held, and -- sessions that gather their edge list -- the full list, parked while the fold's compacted
  // copy takes its place.
  struct CvHold {
    bool active = false;
    long long n_pairs = 0;
    DevBuf<int> lo, hi;
    DevBuf<uint32_t> words;        // 2 per pair: the mirrors (lo, hi) and (hi, lo)
    DevBuf<float> deltas;          // f64 delta tiles: 1 per pair
    bool tiles_patched = false;    // the tile-major copy of build `generation` carries the patch
    int generation = 0;
    bool list_compacted = false;
    DevBuf<int> ei, ej;            // the spare edge list: the compacted copy is written here, then swapped in
    DevBuf<unsigned char> et;
    DevBuf<int8_t> ec;
    long long full_edges = 0;
    int full_parts = 0;
    DevBuf<int> blk_count;
    DevBuf<long long> blk_offset;
    DevBuf<int> sc_i, sc_j;        // topolow_session_score_pairs: the pairs, their truths, the partial sums
    DevBuf<double> sc_t, sc_part;
  } cv;
  int fused_parts = 0;             // partial sums the last ERR launch wrote (stage kernel: workgroups; sweep: units)
  // profiling (roofline accounting)
  bool profiling = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_stage, prof_stage_err, prof_check;   // _err: launches that also reduce the MAE
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_sym, prof_sym_err;                   // symmetric sweep + apply of one iteration

  size_t real_size() const { return precision == TOPOLOW_PRECISION_F64 ? 8 : 4; }
  int rows() const { return row_end - row_begin; }
  int pos_rows() const { return (n + 3) & ~3; }  // position buffers hold the padding points too

  ~topolow_session() {
    for (auto& pr : prof_stage) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (auto& pr : prof_stage_err) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (auto& pr : prof_check) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (auto& pr : prof_sym) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (auto& pr : prof_sym_err) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (hipEvent_t e : pending) (void)hipEventDestroy(e);
    for (hipEvent_t e : event_pool) (void)hipEventDestroy(e);
    if (mailbox) (void)hipHostFree(mailbox);
    if (trace) (void)hipHostFree(trace);
    if (ev_iter_done) (void)hipEventDestroy(ev_iter_done);
    if (ev_check_done) (void)hipEventDestroy(ev_check_done);
    if (check_stream) (void)hipStreamDestroy(check_stream);
    if (own_stream) (void)hipStreamDestroy(own_stream);
  }
};

// ---- FN<DIM>(...) at the coordinates a session's kernels carry (kernel_dim): the launch helpers of topolow_relax.hip
// and topolow_tilegs.hip.  The symmetric sweep has a switch of its own, over its dims (topolow_symm.hip) ----
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

using SymHolds = topolow_session::SymState::Holds;

namespace {

// Profiling sessions: a pair of timing events around what is enqueued on the session's stream while the scope lives.
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

}  // namespace

// ---- defined in topolow_relax.hip ----
int edge_error_blocks(long long n_edges);
void scan_row_flags(topolow_session* s);
void upload_degrees(topolow_session* s, const int32_t* degrees);
// part_sum / part_cnt [0, n_parts) folded into d_out2 (sum, count), on the session's stream (reduce_total_kernel)
void reduce_total(topolow_session* s, int n_parts, double* d_out2);

// ---- defined in topolow_symm.hip: the symmetric sweep as the session's loop and the row-sharded engine see it ----
enum class SymForm { kRowOwner, kSweep, kStages };
bool sym_eligible(const topolow_session* s);
bool sym_available(topolow_session* s);
bool sym_fused_ok(const topolow_session* s);
SymForm sym_form(topolow_session* s, int n_stages);
// sym_iteration<DIM>, sym_sharded_sweep<DIM> and sym_owner_apply<DIM> at the session's ndim
void sym_run_iteration(topolow_session* s, const void* pin, void* pout, int iter, double k, bool err, int S, int st, bool last,
                       const PendingCheck* in_apply);
bool sym_sharded_eligible(const std::vector<topolow_session*>& ss);
void sym_sharded_prepare(std::vector<topolow_session*>& ss);
void sym_run_sharded_sweep(topolow_session* s, const void* pin, int iter, double k, bool err);
void sym_run_owner_apply(topolow_session* s, const void* pin, void* pout, int row_begin, int row_end, const void* push,
                         int n_push, int iter);

// ---- defined in topolow_tilegs.hip ----
void tilegs_run_iteration(topolow_session* s, void* pos, int iter, double k);   // launch_tilegs_iteration<DIM> at the session's ndim
void launch_tilegs_finite(topolow_session* s, const void* pos, int iter1);

// ---- defined in topolow_cv.hip, called by the folds of a prepared handle too (topolow_prep_fold.hip: HandleFolds) ----
int cv_check_hold_out(const topolow_session* s, char* errbuf, size_t errlen);
void cv_hold_out_pairs(topolow_session* s, long long np, const int32_t* degrees, const std::function<void(int*, int*)>& fill);
void cv_score_device(topolow_session* s, const int* d_i, const int* d_j, const double* d_truth, long long n_pairs,
                     double* sum_abs, int64_t* count);

#pragma GCC visibility pop
