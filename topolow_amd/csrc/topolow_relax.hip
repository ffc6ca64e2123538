// topolow_amd/csrc/topolow_relax.hip -- host side of libtopolow_relax.so: the C ABI of
// include/topolow_relax.h over the HIP kernels in relax_kernels.h / relax_gs.h.
//
// Replaces the native half of the reference's euclidean_embedding():
//   .Call(`_topolow_optimize_layout_exact_cpp`, ...)  (reference R/RcppExports.R:4-6)
//   -> optimize_layout_exact_cpp                       (reference src/optimization.cpp:109-382)
// There is no CPU fallback in this library: without a HIP device every entry point that
// computes returns TOPOLOW_ERR_NO_DEVICE.

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
#include "relax_kernels.h"
#include "relax_exact.h"
#include "relax_fold.h"
#include "relax_gs.h"
#include "relax_tilegs.h"
#include "relax_symm.h"
#include "relax_symm64.h"
#include "relax_symm_wide.h"
#include "relax_cv.h"
#include "relax_post.h"
#include "relax_prep.h"
#include "relax_prep_fold.h"
#include "relax_prep_graph.h"
#include "relax_prep_prune.h"
#include "relax_spectrum.h"
#include "relax_fit.h"

using namespace topolow;

namespace {

constexpr int kMaxDim = 64;        // 1..16: the tuned kernels; 17..64: the plain stage kernel (relax_kernels.h: slab_stage_wide_kernel)
constexpr int kMaxTunedDim = 16;
// kernels are instantiated for 1..10, 12, 16, 32 and 64 coordinates; 11 runs as 12, 13..15 as 16, 17..31 as 32 and
// 33..63 as 64 with the extra coordinates held at exactly zero (a zero coordinate adds 0 to every distance and
// receives 0 of every move)
constexpr int kernel_dim(int ndim) { return ndim <= 10 ? ndim : (ndim <= 12 ? 12 : (ndim <= 16 ? 16 : (ndim <= 32 ? 32 : 64))); }
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

double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

}  // namespace

// =========================================================================================
// Session (slab path)
// =========================================================================================
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
  DevBuf<unsigned char> best;
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
    // the sweep sharded over the row-block sessions of a run (relax_sharded_engine.h): this session's segment
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
                       (const double*)pos, (double*)s->best.p, nv, iter1, k_after, s->trace_dev, s->trace_cap, total2);
  } else {
    hipLaunchKernelGGL((controller_kernel<float>), dim3(1), dim3(kCtlThreads), 0, s->stream,
                       s->state.p, s->mailbox_dev, psum, pcnt, nparts,
                       (const float*)pos, (float*)s->best.p, nv, iter1, k_after, s->trace_dev, s->trace_cap, total2);
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
    ac.best = s->best.p;
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

// ---- the symmetric sweep sharded over the row-block sessions of one run (relax_symm.h, relax_sharded_engine.h) ----
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
  s->part_sum.alloc(std::max({s->n_parts, s->dense_blocks, stage_blocks}));
  s->part_cnt.alloc(std::max({s->n_parts, s->dense_blocks, stage_blocks}));
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

template <typename T>
void grow_buf(DevBuf<T>& b, size_t count) { if (b.p == nullptr || b.n < count) b.alloc(count); }

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

// The device half of a hold-out, shared by topolow_session_hold_out and the folds prepared on the device
// (topolow_layout_prep_cv_sweep).  fill(lo, hi) enqueues on s->stream whatever writes the n_pairs held-out pairs into
// the two device arrays: session labels, lo < hi, every pair once, in ANY order -- the mask, tile and compaction
// kernels of relax_cv.h need the pairs unique, not sorted.  degrees: the fold's, per caller's point (host).
template <typename Fill>
void cv_hold_out_pairs(topolow_session* s, long long np, const int32_t* degrees, Fill&& fill) {
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
    hipLaunchKernelGGL((cv_score_kernel<double>), dim3(blocks), dim3(kThreads), 0, s->stream, (const double*)s->best.p,
                       s->dim, d_i, d_j, d_truth, n_pairs, h.sc_part.p);
  else
    hipLaunchKernelGGL((cv_score_kernel<float>), dim3(blocks), dim3(kThreads), 0, s->stream, (const float*)s->best.p,
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

#include "relax_sharded_engine.h"

}  // namespace

// =========================================================================================
// C ABI
// =========================================================================================
extern "C" {

const char* topolow_relax_version(void) { return "topolow_relax 0.1 (gfx950)"; }

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

int64_t topolow_gs_pair_order(int32_t n, uint64_t seed, int32_t iter, int32_t* pairs_out) {
  return gs_pair_order(n, seed, iter, pairs_out);
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
    s->best.alloc(pos_bytes);
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
    // best snapshot starts as the initial positions (reference :171)
    HIP_TRY(hipMemcpyAsync(s->best.p, s->pos[s->cur].p,
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
    if (positions_out) download_positions(s, s->best.p, positions_out);
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

int topolow_session_symm_segment_sweep(topolow_session* s, const void* d_pos_in, int32_t iter, double k,
                                       double* d_out2, char* errbuf, size_t errlen) {
  if (!s || !d_pos_in || !s->began) return TOPOLOW_ERR_BAD_ARGUMENT;
  if (s->sym.holds != SymHolds::kCallerSegment) {
    set_err(errbuf, errlen, "no segment built (topolow_session_symm_segment_build)");
    return TOPOLOW_ERR_BAD_ARGUMENT;
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

// ---- batch of independent embeddings (GS kernel, one workgroup each) --------------------
int topolow_optimize_layout_exact_batch(const topolow_problem* problems, topolow_result* results,
                                        int32_t count, int32_t precision, int32_t device,
                                        double* device_seconds, char* errbuf, size_t errlen) {
  if (count < 0 || (count > 0 && (!problems || !results))) return TOPOLOW_ERR_BAD_ARGUMENT;
  if (device_seconds) *device_seconds = 0.0;
  if (count == 0) return TOPOLOW_OK;
  return guarded(errbuf, errlen, [&] {
    select_device(device);
    for (int b = 0; b < count; ++b)
      if (problems[b].n < 2) throw HipError{TOPOLOW_ERR_TOO_FEW_POINTS, "Need at least 2 points for embedding"};
    if (precision == TOPOLOW_PRECISION_F32) gs_relax<float>(problems, results, count, device_seconds);
    else gs_relax<double>(problems, results, count, device_seconds);
  });
}

// ---- post metric -----------------------------------------------------------------------
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

namespace {

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

}  // namespace

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

int32_t topolow_batch_problem_fits(int32_t n, int32_t ndim, int32_t precision, int64_t n_edges) {
  if (n < 2 || ndim < 1 || ndim > kMaxTunedDim) return 0;
  const int dim = kernel_dim(ndim);
  const size_t rs = precision == TOPOLOW_PRECISION_F32 ? 4 : 8;   // AUTO: f64, as the batch call
  // GsBatch::stage: the LDS-resident edge table when it fits its budget, the dense form otherwise
  const bool sparse = n <= 2048 && n_edges > 0 && n_edges < 65535 && gs_lds_bytes(n, dim, rs, n_edges) <= kGsSparseLdsBudget;
  return gs_lds_bytes(n, dim, rs, sparse ? n_edges : 0) <= kGsLdsLimit ? 1 : 0;
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

namespace {

// Schedule gs is tuned up to kMaxTunedDim dimensions: the one place that says so to a caller.
int check_gs_dim(int ndim, char* errbuf, size_t errlen) {
  if (ndim <= kMaxTunedDim) return TOPOLOW_OK;
  set_err(errbuf, errlen, "schedule gs: ndim must be between 1 and %d (wider embeddings run the slab schedule)", kMaxTunedDim);
  return TOPOLOW_ERR_UNSUPPORTED;
}

// Targets, degrees and the convergence edge list into a fresh whole-problem session (relabelled already).
using SessionLoader = std::function<int(topolow_session*, char*, size_t)>;

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
extern "C++" template <typename Folds>
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

// rows [row_begin, row_end) of as.matrix(dist(positions)): out is (row_end - row_begin) x n, row-major.
// Device memory is bounded: the rows are produced in tiles of at most 256 MB.
int topolow_est_distances_rows(const double* positions, int32_t n, int32_t ndim, int32_t row_begin,
                               int32_t row_end, double* out, int32_t device, char* errbuf, size_t errlen) {
  if (!positions || !out || n < 1 || ndim < 1 || row_begin < 0 || row_end > n || row_begin > row_end)
    return TOPOLOW_ERR_BAD_ARGUMENT;
  return guarded(errbuf, errlen, [&] {
    select_device(device);
    std::vector<double> rowmajor((size_t)n * ndim);
    for (int i = 0; i < n; ++i)
      for (int d = 0; d < ndim; ++d) rowmajor[(size_t)i * ndim + d] = positions[i + (size_t)d * n];
    DevBuf<double> dp, dout;
    dp.alloc(rowmajor.size());
    HIP_TRY(hipMemcpy(dp.p, rowmajor.data(), rowmajor.size() * 8, hipMemcpyHostToDevice));
    const int tile = std::max(1, std::min(row_end - row_begin, (int)((256ll << 20) / (8ll * n))));
    dout.alloc((size_t)tile * n);
    for (int r0 = row_begin; r0 < row_end; r0 += tile) {
      const int rows = std::min(tile, row_end - r0);
      dim3 grid(rows, (n + kThreads - 1) / kThreads);
      hipLaunchKernelGGL(pdist_kernel, grid, dim3(kThreads), 0, 0, dp.p, n, ndim, r0, rows, dout.p);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpy(out + (size_t)(r0 - row_begin) * n, dout.p, (size_t)rows * n * 8, hipMemcpyDeviceToHost));
    }
  });
}

int topolow_est_distances(const double* positions, int32_t n, int32_t ndim,
                          double* est_distances, int32_t device, char* errbuf, size_t errlen) {
  return topolow_est_distances_rows(positions, n, ndim, 0, n, est_distances, device, errbuf, errlen);
}

// ---- post-metrics: est_distances and the terms of mae in one pass (R/core.R:474-481) ----
// The caller's matrices travel in tiles of whole columns (contiguous in column-major storage).  A tile's upload, the
// kernel of the tile before it and the download of the est tile before that run on three streams and overlap; kPostSlots
// sets of buffers go round, ordered by events.  What is allocated is bounded whatever n is: per slot one tile of values,
// of codes and of est on the device (<= kPostTileBytes each while a column fits in that), and as much pinned memory when
// the staging is PINNED.
namespace {

constexpr int kPostSlots = 3;
constexpr size_t kPostTileBytes = (size_t)32 << 20;   // of `values` per tile
constexpr int kPostDefaultStaging = TOPOLOW_POST_STAGING_PINNED;

struct PinBuf {
  void* p = nullptr;
  void alloc(size_t bytes) { HIP_TRY(hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault)); }
  ~PinBuf() { if (p) (void)hipHostFree(p); }
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
};

// hipHostRegister on a range of the caller's memory for as long as this object lives
struct HostRegistration {
  void* p = nullptr;
  void pin(const void* q, size_t bytes) {
    HIP_TRY(hipHostRegister(const_cast<void*>(q), bytes, hipHostRegisterDefault));
    p = const_cast<void*>(q);
  }
  ~HostRegistration() { if (p) (void)hipHostUnregister(p); }
  HostRegistration() = default;
  HostRegistration(const HostRegistration&) = delete;
  HostRegistration& operator=(const HostRegistration&) = delete;
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

// pageable <-> pinned on up to 16 host threads (one per MB)
void post_host_copy(void* dst, const void* src, size_t bytes) {
  host_parallel(bytes, (size_t)1 << 20, [&](size_t lo, size_t hi) {
    memcpy(static_cast<char*>(dst) + lo, static_cast<const char*>(src) + lo, hi - lo);
  });
}

// The matrix of a post-metrics pass when it is resident on the device already (topolow_layout_prep_post_metrics): the
// handle's buffers; a tile is then a run of the buffer's lines and nothing is uploaded.
struct PostResident {
  const double* vals;
  const int8_t* codes;   // nullable
  const int32_t* ord;    // nullable: the input order is kept
};

// The pipeline of topolow_post_metrics_ex, and of topolow_layout_prep_post_metrics when `resident` is given (values
// and codes are then NULL and the device is the current one).  The arguments are checked by the callers.
int post_metrics_run(const double* positions, int32_t n, int32_t ndim, const double* values, const int32_t* codes,
                     const PostResident* resident, double* est_distances, double* sum_abs, int64_t* count,
                     int32_t device, int32_t staging, double* phase_seconds, char* errbuf, size_t errlen) {
  return guarded(errbuf, errlen, [&] {
    if (!resident) select_device(device);
    const bool pinned = staging == TOPOLOW_POST_STAGING_PINNED, want_est = est_distances != nullptr;
    int tile = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, kPostTileBytes / ((size_t)n * 8)));
    if (const char* e = getenv("TOPOLOW_POST_TILE_COLS")) {
      const int cap = atoi(e);
      if (cap >= 1) tile = std::min(tile, cap);
    }
    const int n_tiles = (n + tile - 1) / tile, slots = std::min(kPostSlots, n_tiles);
    const size_t tile_cells = (size_t)tile * n;

    std::vector<double> rowmajor((size_t)n * ndim);
    for (int i = 0; i < n; ++i)
      for (int d = 0; d < ndim; ++d) rowmajor[(size_t)i * ndim + d] = positions[i + (size_t)d * n];
    DevBuf<double> dp, dsum, dvals[kPostSlots], dest[kPostSlots];
    DevBuf<uint32_t> dcnt;
    DevBuf<int32_t> dcodes[kPostSlots];
    PinBuf pvals[kPostSlots], pcodes[kPostSlots], pest[kPostSlots];
    HostRegistration reg_values, reg_codes, reg_est;
    PostPipe P;
    dp.alloc(rowmajor.size());
    HIP_TRY(hipMemcpy(dp.p, rowmajor.data(), rowmajor.size() * 8, hipMemcpyHostToDevice));
    dsum.alloc((size_t)n);
    dcnt.alloc((size_t)n);
    for (int b = 0; b < slots; ++b) {
      if (!resident) dvals[b].alloc(tile_cells);
      if (codes) dcodes[b].alloc(tile_cells);
      if (want_est) dest[b].alloc(tile_cells);
      if (pinned) {
        if (!resident) pvals[b].alloc(tile_cells * 8);
        if (codes) pcodes[b].alloc(tile_cells * 4);
        if (want_est) pest[b].alloc(tile_cells * 8);
      }
    }
    if (staging == TOPOLOW_POST_STAGING_REGISTER && !resident) {
      const size_t cells = (size_t)n * n;
      reg_values.pin(values, cells * 8);
      if (codes) reg_codes.pin(codes, cells * 4);
      if (want_est) reg_est.pin(est_distances, cells * 8);
    }
    P.create(slots, phase_seconds ? n_tiles : 0);

    // est tile `t` has arrived in its pinned buffer: hand it to the caller
    auto drain = [&](int t) {
      const int b = t % slots, c0 = t * tile, cols = std::min(tile, n - c0);
      HIP_TRY(hipEventSynchronize(P.down_done[b]));
      post_host_copy(est_distances + (size_t)c0 * n, pest[b].p, (size_t)cols * n * 8);
    };
    for (int t = 0; t < n_tiles; ++t) {
      const int b = t % slots, c0 = t * tile, cols = std::min(tile, n - c0);
      const size_t off = (size_t)c0 * n, cells = (size_t)cols * n;
      const bool reused = t >= slots;   // tile t - slots went through this slot
      if (resident) {   // nothing to upload: the kernel reads the handle's buffers
        if (want_est && reused) HIP_TRY(hipStreamWaitEvent(P.run, P.down_done[b], 0));   // its est tile has left the device
        P.mark(t, 0, P.run);
        P.mark(t, 1, P.run);
        P.mark(t, 2, P.run);
        hipLaunchKernelGGL(post_metrics_resident_kernel, dim3(cols), dim3(kPostThreads), 0, P.run, dp.p, n, ndim, c0, cols,
                           resident->vals, resident->codes, resident->ord, want_est ? dest[b].p : nullptr, dsum.p, dcnt.p);
        HIP_TRY(hipGetLastError());
        P.mark(t, 3, P.run);
        HIP_TRY(hipEventRecord(P.run_done[b], P.run));
      } else {
        const double* src_v = values + off;
        const int32_t* src_c = codes ? codes + off : nullptr;
        if (pinned) {
          if (reused) HIP_TRY(hipEventSynchronize(P.up_done[b]));   // its upload has left the staging buffers
          post_host_copy(pvals[b].p, src_v, cells * 8);
          src_v = static_cast<const double*>(pvals[b].p);
          if (codes) {
            post_host_copy(pcodes[b].p, src_c, cells * 4);
            src_c = static_cast<const int32_t*>(pcodes[b].p);
          }
        }
        if (reused) HIP_TRY(hipStreamWaitEvent(P.up, P.run_done[b], 0));   // its kernel has read the device tile
        P.mark(t, 0, P.up);
        HIP_TRY(hipMemcpyAsync(dvals[b].p, src_v, cells * 8, hipMemcpyHostToDevice, P.up));
        if (codes) HIP_TRY(hipMemcpyAsync(dcodes[b].p, src_c, cells * 4, hipMemcpyHostToDevice, P.up));
        P.mark(t, 1, P.up);
        HIP_TRY(hipEventRecord(P.up_done[b], P.up));

        HIP_TRY(hipStreamWaitEvent(P.run, P.up_done[b], 0));
        if (want_est && reused) HIP_TRY(hipStreamWaitEvent(P.run, P.down_done[b], 0));   // its est tile has left the device
        P.mark(t, 2, P.run);
        hipLaunchKernelGGL(post_metrics_kernel, dim3(cols), dim3(kPostThreads), 0, P.run, dp.p, n, ndim, c0, cols,
                           dvals[b].p, codes ? dcodes[b].p : nullptr, want_est ? dest[b].p : nullptr, dsum.p, dcnt.p);
        HIP_TRY(hipGetLastError());
        P.mark(t, 3, P.run);
        HIP_TRY(hipEventRecord(P.run_done[b], P.run));
      }

      if (want_est) {
        HIP_TRY(hipStreamWaitEvent(P.down, P.run_done[b], 0));
        P.mark(t, 4, P.down);
        HIP_TRY(hipMemcpyAsync(pinned ? pest[b].p : (void*)(est_distances + off), dest[b].p, cells * 8,
                               hipMemcpyDeviceToHost, P.down));
        P.mark(t, 5, P.down);
        HIP_TRY(hipEventRecord(P.down_done[b], P.down));
        // the tile before this one is drained while this one is on its way: with two slots or more its pinned
        // buffer is not the one just handed to the download above
        if (pinned && t >= 1) drain(t - 1);
      }
    }
    if (pinned && want_est) drain(n_tiles - 1);
    P.sync();

    std::vector<double> col_sum((size_t)n);
    std::vector<uint32_t> col_cnt((size_t)n);
    HIP_TRY(hipMemcpy(col_sum.data(), dsum.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(col_cnt.data(), dcnt.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    double total = 0.0;
    int64_t cells = 0;
    for (int j = 0; j < n; ++j) { total += col_sum[(size_t)j]; cells += col_cnt[(size_t)j]; }   // columns in index order
    *sum_abs = total;
    *count = cells;
    if (phase_seconds) {
      for (int q = 0; q < 3; ++q) phase_seconds[q] = 0.0;
      for (int t = 0; t < n_tiles; ++t)
        for (int q = 0; q < (want_est ? 3 : 2); ++q) {
          float ms = 0.0f;
          HIP_TRY(hipEventElapsedTime(&ms, P.timing[(size_t)t * 6 + 2 * q], P.timing[(size_t)t * 6 + 2 * q + 1]));
          phase_seconds[q] += 1e-3 * ms;
        }
    }
  });
}

}  // namespace

int topolow_post_metrics_ex(const double* positions, int32_t n, int32_t ndim, const double* values,
                            const int32_t* codes, double* est_distances, double* sum_abs, int64_t* count,
                            int32_t device, int32_t staging, double* phase_seconds, char* errbuf, size_t errlen) {
  if (!positions || !values || !sum_abs || !count || n < 1 || ndim < 1 || staging < TOPOLOW_POST_STAGING_DEFAULT ||
      staging > TOPOLOW_POST_STAGING_PAGEABLE)
    return TOPOLOW_ERR_BAD_ARGUMENT;
  if (staging == TOPOLOW_POST_STAGING_DEFAULT) staging = kPostDefaultStaging;
  return post_metrics_run(positions, n, ndim, values, codes, nullptr, est_distances, sum_abs, count, device, staging,
                          phase_seconds, errbuf, errlen);
}

int topolow_post_metrics(const double* positions, int32_t n, int32_t ndim, const double* values,
                         const int32_t* codes, double* est_distances, double* sum_abs, int64_t* count,
                         int32_t device, char* errbuf, size_t errlen) {
  return topolow_post_metrics_ex(positions, n, ndim, values, codes, est_distances, sum_abs, count, device,
                                 TOPOLOW_POST_STAGING_DEFAULT, nullptr, errbuf, errlen);
}

namespace {

// The host's side of a sums pass (prep_tile_sums), of the full matrix (prep_passes) or a fold's masked one
// (prep_fold_prepare): the buffers the tile kernels write, and what the host reads of them.
extern "C++" template <typename Totals>
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
  void fetch(int n, hipStream_t stream) {
    const size_t N = (size_t)n;
    hipLaunchKernelGGL(prep_finish_sums_kernel, dim3((n + kPrepThreads - 1) / kPrepThreads), dim3(kPrepThreads), 0, stream,
                       n, (n + kPrepTile - 1) / kPrepTile, part_slow_sum.p, part_slow_cnt.p, part_fast_sum.p,
                       part_fast_cnt.p, line_sum.p, line_cnt.p);
    HIP_TRY(hipGetLastError());
    sums.resize(2 * N); cnts.resize(2 * N); on_diag.resize(N);
    HIP_TRY(hipMemcpyAsync(sums.data(), line_sum.p, 2 * N * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(cnts.data(), line_cnt.p, 2 * N * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(on_diag.data(), diag.p, N, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(&tot, totals.p, sizeof tot, hipMemcpyDeviceToHost, stream));
  }
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

// Counts per column -> exclusive offsets, off[0 .. n]; returns the total.
int64_t prep_offsets(const int32_t* per_col, size_t n, int64_t* off) {
  off[0] = 0;
  for (size_t j = 0; j < n; ++j) off[j + 1] = off[j] + per_col[j];
  return off[n];
}

}  // namespace

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

namespace {

constexpr size_t kPrepChunkBytes = (size_t)32 << 20;
constexpr int kPrepSlots = 3;

// device -> pinned slot -> the caller's pageable memory, the slots going round: chunk t is on its way while the host
// threads drain chunk t - 1.  Everything before it on `stream` has run when a chunk leaves.
void prep_download(hipStream_t stream, hipEvent_t* done, PinBuf* pin, size_t slot_bytes, void* dst, const void* src,
                   size_t bytes) {
  if (bytes == 0) return;
  const size_t n_chunks = (bytes + slot_bytes - 1) / slot_bytes;
  auto drain = [&](size_t t) {
    const size_t off = t * slot_bytes, len = std::min(slot_bytes, bytes - off);
    HIP_TRY(hipEventSynchronize(done[t % kPrepSlots]));
    post_host_copy(static_cast<char*>(dst) + off, pin[t % kPrepSlots].p, len);
  };
  for (size_t t = 0; t < n_chunks; ++t) {
    const size_t off = t * slot_bytes, len = std::min(slot_bytes, bytes - off);
    HIP_TRY(hipMemcpyAsync(pin[t % kPrepSlots].p, static_cast<const char*>(src) + off, len, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipEventRecord(done[t % kPrepSlots], stream));
    if (t >= 1) drain(t - 1);
  }
  drain(n_chunks - 1);
}

// The stable compaction of the dense fill into the handle's edge list (relax_prep.h: prep_edge_write_kernel), on
// `stream`; the caller orders its reads after it.  fetch() and topolow_session_load_prepared share it: it runs at most
// once per handle, the list stays until destroy().
void prep_compact_edges(topolow_layout_prep* p, hipStream_t stream) {
  if (p->compacted) return;
  const size_t E = (size_t)p->n_edges;
  prep_alloc(p->edge_i, E, "the edge list");
  prep_alloc(p->edge_j, E, "the edge list");
  prep_alloc(p->edge_thresh, E, "the edge list");
  prep_alloc(p->edge_dist, E, "the edge list");
  hipLaunchKernelGGL(prep_edge_write_kernel, dim3(p->n), dim3(kPrepThreads), 0, stream, p->dense.p, p->tdense.p, p->n,
                     p->edge_off.p, p->edge_i.p, p->edge_j.p, p->edge_dist.p, p->edge_thresh.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(stream));   // the list is complete before the flag says so
  p->compacted = true;
}

// A handle whose ordering was declined went through no second pass: every entry that reads one refuses it here.
int prep_check_usable(const topolow_layout_prep* p, char* errbuf, size_t errlen) {
  if (!p->declined) return TOPOLOW_OK;
  set_err(errbuf, errlen, "the ordering was declined (order_route 3): create the handle again with order_in");
  return TOPOLOW_ERR_BAD_ARGUMENT;
}

bool prep_is_permutation(const int32_t* order, int n) {
  std::vector<char> seen((size_t)n, 0);
  for (int q = 0; q < n; ++q) {
    if (order[q] < 0 || order[q] >= n || seen[(size_t)order[q]]) return false;
    seen[(size_t)order[q]] = 1;
  }
  return true;
}

}  // namespace

int32_t topolow_layout_order_from_sums(int32_t n, const double* row_sum, const int64_t* row_cnt,
                                       const double* col_sum, const int64_t* col_cnt, int32_t exact_sums,
                                       int32_t* order_out) {
  if (order_out && n >= 1) order_out[0] = -1;
  if (n < 1 || !row_sum || !row_cnt || !col_sum || !col_cnt || !order_out) return TOPOLOW_ORDER_DECLINED;
  std::vector<double> key((size_t)n);
  int64_t positive = 0;
  for (int p = 0; p < n; ++p) {
    const double rm = row_cnt[p] > 0 ? row_sum[p] / (double)row_cnt[p] : NAN;
    const double cm = col_cnt[p] > 0 ? col_sum[p] / (double)col_cnt[p] : NAN;
    double k = (rm + cm) / 2.0;
    if (std::isnan(k)) k = 0.0;
    key[(size_t)p] = k;
    positive += k > 0.0 ? 1 : 0;
  }
  const bool exact = exact_sums > 0 && n <= (1 << 23);
  if (!exact && exact_sums < 0) return TOPOLOW_ORDER_DECLINED;
  std::vector<int32_t> idx((size_t)n);
  for (int p = 0; p < n; ++p) idx[(size_t)p] = p;
  std::stable_sort(idx.begin(), idx.end(), [&](int32_t x, int32_t y) { return key[(size_t)x] < key[(size_t)y]; });
  if (!exact) {
    // no negative and no infinite cell: either implementation's key is within (n + 2) * 2^-53 relative of the true
    // one, so neighbours further apart than 8 n 2^-53 of the larger sort alike in both.  Two keys of exactly 0 are
    // a tie in both (a sum of non-negative terms is 0 only when every term is).
    const double rel = 8.0 * (double)n * 0x1p-53;
    for (int q = 0; q + 1 < n; ++q) {
      const double lo = key[(size_t)idx[(size_t)q]], hi = key[(size_t)idx[(size_t)q + 1]];
      if (lo == 0.0 && hi == 0.0) continue;
      if (!std::isfinite(hi) || lo < 0.0 || hi < 0x1p-1000 || !(hi - lo > rel * hi)) return TOPOLOW_ORDER_DECLINED;
    }
    if (n == 1 && !(key[0] == 0.0 || (std::isfinite(key[0]) && key[0] >= 0x1p-1000))) return TOPOLOW_ORDER_DECLINED;
  }
  if (positive > 1) std::copy(idx.begin(), idx.end(), order_out);
  return exact ? TOPOLOW_ORDER_DEVICE_EXACT : TOPOLOW_ORDER_DEVICE_GAP;
}

namespace {

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

bool prep_order_in_ok(int32_t preserve_order, const int32_t* order_in, int n, char* errbuf, size_t errlen) {
  if (!preserve_order && order_in != nullptr && order_in[0] != -1 && !prep_is_permutation(order_in, n)) {
    set_err(errbuf, errlen, "order_in must be a permutation of 0..n-1, or start with -1");
    return false;
  }
  return true;
}

// Everything a handle goes through once its matrix is on the device -- the ONE copy of the passes, reached by
// topolow_layout_prep_create (the matrix arrives by upload) and topolow_layout_prep_subsample (it arrives by a gather
// from another handle).  p holds n, device, transposed, has_codes and the allocated vals / codes; arrive(P, t, a0,
// lines) enqueues the arrival of lines [a0, a0 + lines) -- chunk t of `g` -- so that P.run is ordered after it.  The
// first pass runs on each chunk as it arrives (the same bits whatever the chunking), then the ordering rule, then --
// unless the rule declines -- the second pass.  t0: when the caller began (phase_seconds[0] counts from it).
void prep_passes(topolow_layout_prep* p, int32_t preserve_order, const int32_t* order_in, topolow_layout_prep_info* info,
                 double t0, const PrepChunks& g, const std::function<void(PostPipe&, int, int, int)>& arrive) {
  const int n = p->n;
  const bool given = !preserve_order && order_in != nullptr;
  const int8_t* codes = p->has_codes ? p->codes.p : nullptr;
  const size_t N = (size_t)n, cells = N * N;
  const int nb = (n + kPrepTile - 1) / kPrepTile;

  // -- arrival and first pass, overlapped
  PrepSums<PrepTotals> S;
  S.alloc(n);
  PostPipe P;
  P.create(g.slots, 0);
  HIP_TRY(hipMemsetAsync(S.totals.p, 0, sizeof(PrepTotals), P.run));
  for (int t = 0; t < g.n_chunks; ++t) {
    const int a0 = t * g.chunk_lines, lines = std::min(g.chunk_lines, n - a0);
    arrive(P, t, a0, lines);
    hipLaunchKernelGGL(prep_sums_kernel, dim3(nb, (lines + kPrepTile - 1) / kPrepTile), dim3(kPrepThreads), 0, P.run,
                       p->vals.p, codes, n, a0, S.part_slow_sum.p, S.part_slow_cnt.p, S.part_fast_sum.p,
                       S.part_fast_cnt.p, S.diag.p, S.totals.p);
    HIP_TRY(hipGetLastError());
  }
  S.fetch(n, P.run);
  P.sync();
  const PrepTotals& tot = S.tot;
  const double t1 = now_s();

  // -- the quantities of the info struct and the order
  const size_t row_at = p->transposed ? 0 : N, col_at = p->transposed ? N : 0;   // slow lines are rows when transposed
  *info = topolow_layout_prep_info();
  info->n_edges = -1;
  info->n_finite_nonzero = (int64_t)tot.n_finite_nonzero;
  info->n_infinite = (int64_t)tot.n_infinite;
  info->n_negative = (int64_t)tot.n_negative;
  info->exact_sums = tot.n_inexact == 0 ? 1 : 0;
  p->exact_sums = tot.n_inexact == 0;
  p->negative_or_infinite = tot.n_negative + tot.n_infinite > 0;
  info->numeric_max = S.numeric_max();
  p->order.assign(N, 0);
  p->order[0] = -1;
  if (preserve_order) {
    info->order_route = TOPOLOW_ORDER_PRESERVED;
  } else if (given) {
    info->order_route = TOPOLOW_ORDER_DECLINED;
    std::copy(order_in, order_in + (order_in[0] == -1 ? 1 : n), p->order.begin());
  } else {
    info->order_route = S.order(n, row_at, col_at, p->exact_sums, p->negative_or_infinite, p->order.data());
    if (info->order_route == TOPOLOW_ORDER_DECLINED) {
      p->declined = true;
      p->phase_seconds[0] = t1 - t0;
      return;
    }
  }
  const bool reordered = p->order[0] != -1;
  info->reordered = reordered ? 1 : 0;
  std::vector<int32_t> ord(N);
  for (size_t q = 0; q < N; ++q) ord[q] = reordered ? p->order[q] : (int32_t)q;
  p->degrees.resize(N);
  for (size_t q = 0; q < N; ++q) p->degrees[q] = S.cnts[row_at + (size_t)ord[q]];
  const double t2 = now_s();

  // -- second pass: dense fill, edges per column
  prep_alloc(p->ord, N, "the order");
  prep_alloc(p->dense, cells, "the dense distances");
  prep_alloc(p->tdense, cells, "the dense thresholds");
  prep_alloc(p->edge_off, N + 1, "the edge offsets");
  prep_alloc(p->ddeg, N, "the degrees");
  HIP_TRY(hipMemcpyAsync(p->ddeg.p, p->degrees.data(), N * 4, hipMemcpyHostToDevice, P.run));
  DevBuf<int32_t> col_edges;
  prep_alloc(col_edges, N, "the edge counts");
  HIP_TRY(hipMemcpyAsync(p->ord.p, ord.data(), N * 4, hipMemcpyHostToDevice, P.run));
  hipLaunchKernelGGL(prep_dense_kernel, dim3(nb, nb), dim3(kPrepThreads), 0, P.run, p->vals.p, codes, n, p->ord.p,
                     p->transposed ? 1 : 0, p->dense.p, p->tdense.p);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(prep_edge_count_kernel, dim3(n), dim3(kPrepThreads), 0, P.run, p->dense.p, n, col_edges.p);
  HIP_TRY(hipGetLastError());
  std::vector<int32_t> per_col(N);
  HIP_TRY(hipMemcpyAsync(per_col.data(), col_edges.p, N * 4, hipMemcpyDeviceToHost, P.run));
  HIP_TRY(hipStreamSynchronize(P.run));
  std::vector<int64_t> off(N + 1);
  p->n_edges = prep_offsets(per_col.data(), N, off.data());
  HIP_TRY(hipMemcpy(p->edge_off.p, off.data(), (N + 1) * 8, hipMemcpyHostToDevice));
  info->n_edges = p->n_edges;
  p->phase_seconds[0] = t1 - t0;
  p->phase_seconds[1] = t2 - t1;
  p->phase_seconds[2] = now_s() - t2;
}

}  // namespace

int topolow_layout_prep_create(topolow_layout_prep** out, const double* values, const int8_t* codes, int32_t n,
                               int32_t transposed, int32_t preserve_order, const int32_t* order_in, int32_t device,
                               topolow_layout_prep_info* info, char* errbuf, size_t errlen) {
  if (!out || !values || !info || n < 2) return TOPOLOW_ERR_BAD_ARGUMENT;
  *out = nullptr;
  if (!prep_order_in_ok(preserve_order, order_in, n, errbuf, errlen)) return TOPOLOW_ERR_BAD_ARGUMENT;
  std::unique_ptr<topolow_layout_prep> p(new topolow_layout_prep());
  const int rc = guarded(errbuf, errlen, [&] {
    p->device = select_device(device);
    p->n = n;
    p->transposed = transposed != 0;
    p->has_codes = codes != nullptr;
    const size_t N = (size_t)n, cells = N * N;
    const double t0 = now_s();
    prep_alloc(p->vals, cells, "the matrix");
    if (codes) prep_alloc(p->codes, cells, "the codes");
    // the matrix goes up in chunks through pinned staging, the slots going round
    const PrepChunks g(n);
    PinBuf pvals[kPrepSlots], pcodes[kPrepSlots];
    for (int b = 0; b < g.slots; ++b) {
      pvals[b].alloc(g.chunk_cells * 8);
      if (codes) pcodes[b].alloc(g.chunk_cells);
    }
    prep_passes(p.get(), preserve_order, order_in, info, t0, g, [&](PostPipe& P, int t, int a0, int lines) {
      const int b = t % g.slots;
      const size_t off = (size_t)a0 * N, len = (size_t)lines * N;
      if (t >= g.slots) HIP_TRY(hipEventSynchronize(P.up_done[b]));   // chunk t - slots has left the staging buffers
      post_host_copy(pvals[b].p, values + off, len * 8);
      if (codes) post_host_copy(pcodes[b].p, codes + off, len);
      HIP_TRY(hipMemcpyAsync(p->vals.p + off, pvals[b].p, len * 8, hipMemcpyHostToDevice, P.up));
      if (codes) HIP_TRY(hipMemcpyAsync(p->codes.p + off, pcodes[b].p, len, hipMemcpyHostToDevice, P.up));
      HIP_TRY(hipEventRecord(P.up_done[b], P.up));
      HIP_TRY(hipStreamWaitEvent(P.run, P.up_done[b], 0));
    });
  });
  if (rc != TOPOLOW_OK) return rc;
  *out = p.release();
  return TOPOLOW_OK;
}

int topolow_layout_prep_fetch(topolow_layout_prep* p, int32_t* order, int32_t* degrees, int32_t* edge_i,
                              int32_t* edge_j, double* edge_dist, int32_t* edge_thresh, double* dense, int32_t* tdense,
                              double* values_reordered, int8_t* codes_reordered, char* errbuf, size_t errlen) {
  if (!p || !order || !degrees || !edge_i || !edge_j || !edge_dist || !edge_thresh) return TOPOLOW_ERR_BAD_ARGUMENT;
  if (const int rcu = prep_check_usable(p, errbuf, errlen)) return rcu;
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(p->device));
    const double t0 = now_s();
    const int n = p->n;
    const size_t N = (size_t)n, cells = N * N, E = (size_t)p->n_edges;
    std::copy(p->order.begin(), p->order.end(), order);
    std::copy(p->degrees.begin(), p->degrees.end(), degrees);

    const bool want_codes = codes_reordered != nullptr && p->has_codes;
    size_t largest = std::max<size_t>(E * 8, 4096);
    if (dense || values_reordered) largest = std::max(largest, cells * 8);
    if (tdense) largest = std::max(largest, cells * 4);
    if (want_codes) largest = std::max(largest, cells);
    const size_t slot_bytes = std::min(kPrepChunkBytes, largest);
    PinBuf pin[kPrepSlots];
    PostPipe P;
    for (int b = 0; b < kPrepSlots; ++b) pin[b].alloc(slot_bytes);
    P.create(kPrepSlots, 0);

    prep_compact_edges(p, P.down);
    DevBuf<double> rvals;
    DevBuf<int8_t> rcodes;
    if (values_reordered || want_codes) {
      if (values_reordered) prep_alloc(rvals, cells, "the reordered matrix");
      if (want_codes) prep_alloc(rcodes, cells, "the reordered codes");
      hipLaunchKernelGGL(prep_reorder_kernel, dim3(n), dim3(kPrepThreads), 0, P.down, p->vals.p,
                         want_codes ? p->codes.p : nullptr, n, p->ord.p, values_reordered ? rvals.p : nullptr,
                         want_codes ? rcodes.p : nullptr);
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(P.down));   // the compaction and the gather end here, the downloads begin
    const double t1 = now_s();
    prep_download(P.down, P.down_done, pin, slot_bytes, edge_i, p->edge_i.p, E * 4);
    prep_download(P.down, P.down_done, pin, slot_bytes, edge_j, p->edge_j.p, E * 4);
    prep_download(P.down, P.down_done, pin, slot_bytes, edge_dist, p->edge_dist.p, E * 8);
    prep_download(P.down, P.down_done, pin, slot_bytes, edge_thresh, p->edge_thresh.p, E * 4);
    if (dense) prep_download(P.down, P.down_done, pin, slot_bytes, dense, p->dense.p, cells * 8);
    if (tdense) prep_download(P.down, P.down_done, pin, slot_bytes, tdense, p->tdense.p, cells * 4);
    if (values_reordered) prep_download(P.down, P.down_done, pin, slot_bytes, values_reordered, rvals.p, cells * 8);
    if (want_codes) prep_download(P.down, P.down_done, pin, slot_bytes, codes_reordered, rcodes.p, cells);
    else if (codes_reordered) memset(codes_reordered, 0, cells);   // no codes came in: all zero
    P.sync();
    p->phase_seconds[3] = t1 - t0;
    p->phase_seconds[4] = now_s() - t1;
  });
}

int topolow_layout_prep_phase_seconds(const topolow_layout_prep* p, double* seconds) {
  if (!p || !seconds) return TOPOLOW_ERR_BAD_ARGUMENT;
  for (int q = 0; q < 5; ++q) seconds[q] = p->phase_seconds[q];
  return TOPOLOW_OK;
}

void topolow_layout_prep_destroy(topolow_layout_prep* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  delete p;
}

// ---- the measurement graph of a handle and its sub-handles (relax_prep_graph.h) ----
namespace {

// The rules both graph entries share for `subset` (NULL: all n points); no device call.  n is the handle's.
int prep_check_subset(int n, const int32_t* subset, int32_t m, char* errbuf, size_t errlen) {
  if (subset == nullptr) return TOPOLOW_OK;
  if (m < 2 || m > n) {
    set_err(errbuf, errlen, "subset: m = %d must be between 2 and the handle's n = %d", (int)m, n);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  std::vector<char> seen((size_t)n, 0);
  for (int q = 0; q < m; ++q) {
    const int32_t x = subset[q];
    if (x < 0 || x >= n) {
      set_err(errbuf, errlen, "subset[%d] = %d is out of range (0 .. %d)", q, (int)x, n - 1);
      return TOPOLOW_ERR_BAD_ARGUMENT;
    }
    if (seen[(size_t)x]) {
      set_err(errbuf, errlen, "subset[%d] = %d is a repeated index", q, (int)x);
      return TOPOLOW_ERR_BAD_ARGUMENT;
    }
    seen[(size_t)x] = 1;
  }
  return TOPOLOW_OK;
}

}  // namespace

int topolow_layout_prep_connectivity(topolow_layout_prep* p, const int32_t* subset, int32_t m, int32_t* n_components,
                                     int64_t* n_cells, int32_t* labels, char* errbuf, size_t errlen) {
  if (!p || !n_components || !n_cells) {
    set_err(errbuf, errlen, "topolow_layout_prep_connectivity: the handle, n_components and n_cells must not be NULL");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  const int rcs = prep_check_subset(p->n, subset, m, errbuf, errlen);
  if (rcs != TOPOLOW_OK) return rcs;
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(p->device));
    const double t0 = now_s();
    const int M = subset != nullptr ? m : p->n;
    const int words = (M + 63) / 64;
    DevBuf<int32_t> sub, parent, changed;
    DevBuf<unsigned long long> bits, cells;
    if (subset != nullptr) prep_alloc(sub, (size_t)M, "the subset");
    prep_alloc(parent, (size_t)M, "the component labels");
    prep_alloc(changed, 1, "the round flag");
    prep_alloc(bits, (size_t)M * (size_t)words, "the bit adjacency");
    prep_alloc(cells, 1, "the cell count");
    PostPipe P;
    P.create(0, 0);
    if (subset != nullptr) HIP_TRY(hipMemcpyAsync(sub.p, subset, (size_t)M * 4, hipMemcpyHostToDevice, P.run));
    HIP_TRY(hipMemsetAsync(cells.p, 0, sizeof(unsigned long long), P.run));
    hipLaunchKernelGGL(graph_bits_kernel, dim3(M), dim3(kGraphThreads), 0, P.run, p->vals.p, p->n,
                       subset != nullptr ? sub.p : nullptr, M, words, bits.p, parent.p, cells.p);
    HIP_TRY(hipGetLastError());
    unsigned long long set_bits = 0;
    HIP_TRY(hipMemcpyAsync(&set_bits, cells.p, sizeof set_bits, hipMemcpyDeviceToHost, P.run));
    HIP_TRY(hipStreamSynchronize(P.run));
    const double t1 = now_s();
    // the rounds: flatten, hook, ask whether anything was hooked; the round that hooks nothing leaves the labels
    int rounds = 0;
    for (;;) {
      if (rounds > M)   // a round that hooks lowers a label; this many cannot happen
        throw HipError{TOPOLOW_ERR_HIP, "connectivity: the component rounds did not settle within m + 1 rounds"};
      ++rounds;
      int32_t any = 0;
      HIP_TRY(hipMemsetAsync(changed.p, 0, sizeof(int32_t), P.run));
      hipLaunchKernelGGL(graph_jump_kernel, dim3((M + kGraphThreads - 1) / kGraphThreads), dim3(kGraphThreads), 0, P.run,
                         parent.p, M);
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(graph_hook_kernel, dim3((M + kGraphWaves - 1) / kGraphWaves), dim3(kGraphThreads), 0, P.run,
                         bits.p, M, words, parent.p, changed.p);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(&any, changed.p, sizeof any, hipMemcpyDeviceToHost, P.run));
      HIP_TRY(hipStreamSynchronize(P.run));
      if (!any) break;
    }
    std::vector<int32_t> lab((size_t)M);
    HIP_TRY(hipMemcpyAsync(lab.data(), parent.p, (size_t)M * 4, hipMemcpyDeviceToHost, P.run));
    HIP_TRY(hipStreamSynchronize(P.run));
    int32_t roots = 0;
    for (int q = 0; q < M; ++q) roots += lab[(size_t)q] == q ? 1 : 0;
    *n_components = roots;
    *n_cells = (int64_t)set_bits;
    if (labels != nullptr) std::copy(lab.begin(), lab.end(), labels);
    p->graph_rounds = rounds;
    p->graph_seconds[0] = t1 - t0;
    p->graph_seconds[1] = now_s() - t1;
  });
}

int topolow_layout_prep_subsample(topolow_layout_prep* parent, const int32_t* subset, int32_t m,
                                  int32_t preserve_order, const int32_t* order_in, topolow_layout_prep** out,
                                  topolow_layout_prep_info* info, char* errbuf, size_t errlen) {
  if (!parent || !out || !info) {
    set_err(errbuf, errlen, "topolow_layout_prep_subsample: the parent, out and info must not be NULL");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  *out = nullptr;
  const int rcs = prep_check_subset(parent->n, subset, m, errbuf, errlen);
  if (rcs != TOPOLOW_OK) return rcs;
  const int M = subset != nullptr ? m : parent->n;
  if (!prep_order_in_ok(preserve_order, order_in, M, errbuf, errlen)) return TOPOLOW_ERR_BAD_ARGUMENT;
  std::unique_ptr<topolow_layout_prep> p(new topolow_layout_prep());
  const int rc = guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(parent->device));
    p->device = parent->device;
    p->n = M;
    p->transposed = parent->transposed;
    p->has_codes = parent->has_codes;
    const size_t cells = (size_t)M * (size_t)M;
    const double t0 = now_s();
    prep_alloc(p->vals, cells, "the matrix");
    if (p->has_codes) prep_alloc(p->codes, cells, "the codes");
    DevBuf<int32_t> sub;
    if (subset != nullptr) {
      prep_alloc(sub, (size_t)M, "the subset");
      HIP_TRY(hipMemcpy(sub.p, subset, (size_t)M * 4, hipMemcpyHostToDevice));
    }
    // the matrix arrives from the parent, a chunk of lines per launch on the stream of the passes
    const PrepChunks g(M);
    prep_passes(p.get(), preserve_order, order_in, info, t0, g, [&](PostPipe& P, int, int a0, int lines) {
      hipLaunchKernelGGL(graph_gather_kernel, dim3(lines), dim3(kGraphThreads), 0, P.run, parent->vals.p,
                         parent->has_codes ? parent->codes.p : nullptr, parent->n, subset != nullptr ? sub.p : nullptr, M,
                         a0, p->vals.p, p->has_codes ? p->codes.p : nullptr);
      HIP_TRY(hipGetLastError());
    });
  });
  if (rc != TOPOLOW_OK) return rc;
  *out = p.release();
  return TOPOLOW_OK;
}

int topolow_layout_prep_graph_stats(const topolow_layout_prep* p, int32_t* rounds, double* seconds) {
  if (!p || !rounds || !seconds) return TOPOLOW_ERR_BAD_ARGUMENT;
  *rounds = p->graph_rounds;
  seconds[0] = p->graph_seconds[0];
  seconds[1] = p->graph_seconds[1];
  return TOPOLOW_OK;
}

// ---- degrees and pruning of a resident matrix (relax_prep_prune.h) ----
namespace {

static_assert(kPruneConverged == TOPOLOW_PRUNE_CONVERGED && kPruneMinPoints == TOPOLOW_PRUNE_MIN_POINTS &&
                  kPruneMaxIterations == TOPOLOW_PRUNE_MAX_ITERATIONS && kPruneAllRemoved == TOPOLOW_PRUNE_ALL_REMOVED,
              "the kernels' stop reasons are the header's");

constexpr int kPruneBatch = 8;   // rounds launched between two reads of the state

// The row-oriented bits of parent[subset, subset] (M x words; bit (r, c): cell (r, c) is measured) into `bits`, on
// `stream`; returns the set bits.  Where a buffer line is a matrix column the line bits are turned round and freed.
unsigned long long prune_row_bits(const topolow_layout_prep* p, const int32_t* subset, int M, int words, hipStream_t stream,
                                  DevBuf<unsigned long long>& bits) {
  DevBuf<int32_t> sub, first;
  DevBuf<unsigned long long> cells, line_bits;
  const size_t count = (size_t)M * (size_t)words;
  if (subset != nullptr) prep_alloc(sub, (size_t)M, "the subset");
  prep_alloc(first, (size_t)M, "the first neighbours");
  prep_alloc(cells, 1, "the cell count");
  DevBuf<unsigned long long>& by_line = p->transposed ? bits : line_bits;
  prep_alloc(by_line, count, "the bit adjacency");
  if (subset != nullptr) HIP_TRY(hipMemcpyAsync(sub.p, subset, (size_t)M * 4, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemsetAsync(cells.p, 0, sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(graph_bits_kernel, dim3(M), dim3(kGraphThreads), 0, stream, p->vals.p, p->n,
                     subset != nullptr ? sub.p : nullptr, M, words, by_line.p, first.p, cells.p);
  HIP_TRY(hipGetLastError());
  if (!p->transposed) {
    prep_alloc(bits, count, "the transposed bit adjacency");
    const long long tiles = (long long)words * (long long)words;
    hipLaunchKernelGGL(prune_bits_transpose_kernel, dim3((unsigned)((tiles + kGraphWaves - 1) / kGraphWaves)),
                       dim3(kGraphThreads), 0, stream, line_bits.p, M, words, bits.p);
    HIP_TRY(hipGetLastError());
  }
  unsigned long long set_bits = 0;
  HIP_TRY(hipMemcpyAsync(&set_bits, cells.p, sizeof set_bits, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return set_bits;
}

// `words` words with the bits 0 .. M - 1 set: every point alive.
void prune_all_alive(int M, int words, std::vector<unsigned long long>& all) {
  all.assign((size_t)words, ~0ull);
  if (M & 63) all[(size_t)words - 1] = (1ull << (M & 63)) - 1ull;
}

void prune_launch_count(hipStream_t stream, const unsigned long long* bits, int M, int words, const unsigned long long* alive,
                        int min_connections, uint8_t* flag, int32_t* counts, PruneState* st) {
  hipLaunchKernelGGL(prune_count_kernel, dim3((M + kGraphWaves - 1) / kGraphWaves), dim3(kGraphThreads), 0, stream, bits, M,
                     words, alive, min_connections, flag, counts, st);
  HIP_TRY(hipGetLastError());
}

}  // namespace

int topolow_layout_prep_degrees(topolow_layout_prep* p, const int32_t* subset, int32_t m, int32_t* degrees,
                                int64_t* n_cells, char* errbuf, size_t errlen) {
  if (!p || !degrees || !n_cells) {
    set_err(errbuf, errlen, "topolow_layout_prep_degrees: the handle, degrees and n_cells must not be NULL");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  const int rcs = prep_check_subset(p->n, subset, m, errbuf, errlen);
  if (rcs != TOPOLOW_OK) return rcs;
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(p->device));
    const int M = subset != nullptr ? m : p->n;
    const int words = (M + 63) / 64;
    DevBuf<unsigned long long> bits, alive;
    DevBuf<uint8_t> flag;
    DevBuf<int32_t> counts;
    DevBuf<PruneState> st;
    PostPipe P;
    P.create(0, 0);
    prune_row_bits(p, subset, M, words, P.run, bits);
    prep_alloc(alive, (size_t)words, "the mask of kept points");
    prep_alloc(flag, (size_t)M, "the round's flags");
    prep_alloc(counts, (size_t)M, "the degrees");
    prep_alloc(st, 1, "the pruning state");
    std::vector<unsigned long long> all;
    prune_all_alive(M, words, all);
    PruneState state = PruneState();
    state.size = M;
    HIP_TRY(hipMemcpy(alive.p, all.data(), (size_t)words * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(st.p, &state, sizeof state, hipMemcpyHostToDevice));
    prune_launch_count(P.run, bits.p, M, words, alive.p, 0, flag.p, counts.p, st.p);
    HIP_TRY(hipMemcpyAsync(degrees, counts.p, (size_t)M * 4, hipMemcpyDeviceToHost, P.run));
    HIP_TRY(hipMemcpyAsync(&state, st.p, sizeof state, hipMemcpyDeviceToHost, P.run));
    HIP_TRY(hipStreamSynchronize(P.run));
    *n_cells = (int64_t)state.cells;
  });
}

int topolow_layout_prep_prune(topolow_layout_prep* p, int32_t min_connections, double target_completeness,
                              int32_t max_iterations, int32_t min_points, uint8_t* kept, topolow_prune_info* info,
                              char* errbuf, size_t errlen) {
  if (!p || !kept || !info) {
    set_err(errbuf, errlen, "topolow_layout_prep_prune: the handle, kept and info must not be NULL");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  const bool search = !std::isnan(target_completeness);
  if (p->n < min_points) {
    set_err(errbuf, errlen, "Matrix size (%d) is smaller than min_points (%d)", p->n, (int)min_points);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (min_connections < 1) {
    set_err(errbuf, errlen, "min_connections must be a positive integer");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (search && !(target_completeness > 0.0 && target_completeness <= 1.0)) {
    set_err(errbuf, errlen, "target_completeness must be between 0 and 1");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(p->device));
    const double t0 = now_s();
    const int n = p->n, words = (n + 63) / 64;
    const int rounds_asked = std::max<int32_t>(max_iterations, 0), limit = std::min(rounds_asked, n);
    DevBuf<unsigned long long> bits, alive;
    DevBuf<uint8_t> flag;
    DevBuf<PruneState> st;
    PostPipe P;
    P.create(0, 0);
    const unsigned long long set_bits = prune_row_bits(p, nullptr, n, words, P.run, bits);
    const double t1 = now_s();
    prep_alloc(alive, (size_t)words, "the mask of kept points");
    prep_alloc(flag, (size_t)n, "the round's flags");
    prep_alloc(st, 1, "the pruning state");
    std::vector<unsigned long long> all;
    prune_all_alive(n, words, all);
    PruneState fresh = PruneState();
    fresh.size = n;
    *info = topolow_prune_info();
    info->original_size = n;
    info->original_cells = (int64_t)set_bits;
    info->target_reached = search ? 0 : -1;
    for (int a = 0; a < (search ? TOPOLOW_PRUNE_MAX_ATTEMPTS : 1); ++a) {
      const int threshold = search ? 4 + 2 * a : (int)min_connections;
      // every attempt starts from the whole matrix; `all` and `fresh` stay as they are while the copies are under way
      HIP_TRY(hipMemcpyAsync(alive.p, all.data(), (size_t)words * 8, hipMemcpyHostToDevice, P.run));
      HIP_TRY(hipMemcpyAsync(st.p, &fresh, sizeof fresh, hipMemcpyHostToDevice, P.run));
      PruneState state = fresh;
      int launched = 0;
      while (launched < limit && state.stopped == 0) {
        const int batch = std::min(kPruneBatch, limit - launched);
        for (int b = 0; b < batch; ++b) {
          prune_launch_count(P.run, bits.p, n, words, alive.p, threshold, flag.p, nullptr, st.p);
          hipLaunchKernelGGL(prune_decide_kernel, dim3(1), dim3(kGraphThreads), 0, P.run, n, words, (int)min_points, flag.p,
                             alive.p, st.p);
          HIP_TRY(hipGetLastError());
        }
        launched += batch;
        HIP_TRY(hipMemcpyAsync(&state, st.p, sizeof state, hipMemcpyDeviceToHost, P.run));
        HIP_TRY(hipStreamSynchronize(P.run));
      }
      int reason = state.stopped;
      unsigned long long final_cells = state.final_cells;
      if (reason == 0) {
        // no round stopped: max_iterations rounds each removed points.  (Fewer than that cannot be: a round that does
        // not stop removes a point, so n of them leave none.)  One more count gives the cells of what is left.
        if (launched < rounds_asked)
          throw HipError{TOPOLOW_ERR_HIP, "prune: the rounds did not stop within n rounds"};
        prune_launch_count(P.run, bits.p, n, words, alive.p, threshold, flag.p, nullptr, st.p);
        HIP_TRY(hipMemcpyAsync(&state, st.p, sizeof state, hipMemcpyDeviceToHost, P.run));
        HIP_TRY(hipStreamSynchronize(P.run));
        reason = kPruneMaxIterations;
        final_cells = state.cells;
      }
      info->attempts = a + 1;
      info->min_connections_used = threshold;
      info->iterations = info->attempt_iterations[a] = state.iteration;
      info->stop_reason = info->attempt_stop_reason[a] = reason;
      info->last_remove = info->attempt_last_remove[a] = state.last_remove;
      info->final_size = info->attempt_final_size[a] = state.size;
      info->final_cells = info->attempt_final_cells[a] = (int64_t)final_cells;
      if (!search || reason == kPruneAllRemoved) break;
      const double s = (double)state.size;
      const double completeness = state.size >= 2 ? (double)final_cells / (s * (s - 1.0)) : NAN;
      if (completeness >= target_completeness) {
        info->target_reached = 1;
        break;
      }
      if (state.size <= min_points) break;
    }
    const double t2 = now_s();
    std::vector<unsigned long long> mask((size_t)words);
    HIP_TRY(hipMemcpyAsync(mask.data(), alive.p, (size_t)words * 8, hipMemcpyDeviceToHost, P.run));
    HIP_TRY(hipStreamSynchronize(P.run));
    for (int q = 0; q < n; ++q) kept[q] = (uint8_t)((mask[(size_t)q >> 6] >> (q & 63)) & 1ull);
    info->seconds[0] = t1 - t0;
    info->seconds[1] = t2 - t1;
    info->seconds[2] = now_s() - t2;
  });
}

// ---- spectrum of a resident matrix (relax_spectrum.h; reference R/core.R:983-1007) ----
namespace {

bool spec_all_finite(const double* x, size_t count) {
  for (size_t q = 0; q < count; ++q)
    if (!std::isfinite(x[q])) return false;
  return true;
}

// d (n) and e (n - 1) of the tridiagonal form of the symmetric matrix A (device, n x n, both triangles; overwritten).
void spec_tridiagonalize(double* A, int n, hipStream_t stream, double* d_host, double* e_host) {
  const size_t N = (size_t)n;
  if (n == 1) {
    HIP_TRY(hipMemcpyAsync(d_host, A, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return;
  }
  const int lb = kSpecLineBlock, n_blocks = (n - 1) / lb + 1;
  DevBuf<double> v[2], w, y, part, scal, d, e;
  prep_alloc(v[0], N, "the reflections");
  prep_alloc(v[1], N, "the reflections");
  prep_alloc(w, N, "the reflections");
  prep_alloc(y, N, "the reflections");
  prep_alloc(part, N * (size_t)n_blocks, "the partial sums");
  prep_alloc(scal, 1, "the step scalars");
  prep_alloc(d, N, "the tridiagonal");
  prep_alloc(e, N, "the tridiagonal");
  HIP_TRY(hipMemsetAsync(v[0].p, 0, N * 8, stream));
  HIP_TRY(hipMemsetAsync(v[1].p, 0, N * 8, stream));
  HIP_TRY(hipMemsetAsync(w.p, 0, N * 8, stream));
  HIP_TRY(hipMemsetAsync(y.p, 0, N * 8, stream));
  HIP_TRY(hipMemsetAsync(scal.p, 0, 8, stream));
  for (int k = 0; k + 1 < n; ++k) {
    const double* v_prev = v[k & 1].p;
    double* v_new = v[(k + 1) & 1].p;
    hipLaunchKernelGGL(spec_step_kernel, dim3(1), dim3(kSpecStepThreads), 0, stream, A, n, k, v_prev, v_new, w.p, y.p,
                       scal.p, d.p, e.p);
    HIP_TRY(hipGetLastError());
    if (k + 2 < n) {   // a trailing matrix of at least 2 x 2 is left
      const int first = k + 1;
      const dim3 grid((n - 1) / kSpecThreads - first / kSpecThreads + 1, (n - 1) / lb - first / lb + 1);
      hipLaunchKernelGGL(spec_stream_kernel, grid, dim3(kSpecThreads), 0, stream, A, n, k, v_prev, w.p, v_new, part.p);
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(spec_sum_kernel, dim3((n - first + kSpecSumThreads - 1) / kSpecSumThreads), dim3(kSpecSumThreads),
                         0, stream, n, k, part.p, y.p);
      HIP_TRY(hipGetLastError());
    }
  }
  HIP_TRY(hipMemcpyAsync(d_host, d.p, N * 8, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(e_host, e.p, (N - 1) * 8, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
}

// The eigenvalues of the tridiagonal (d, e), all finite, descending into out (host, n).
void spec_bisect(const double* d, const double* e, int n, hipStream_t stream, double* out) {
  const size_t N = (size_t)n;
  std::vector<double> e2(N, 0.0);
  double lo = d[0], hi = d[0], e2max = 0.0;
  for (int i = 0; i < n; ++i) {
    const double r = (i > 0 ? std::fabs(e[i - 1]) : 0.0) + (i + 1 < n ? std::fabs(e[i]) : 0.0);
    lo = std::min(lo, d[i] - r);
    hi = std::max(hi, d[i] + r);
    if (i + 1 < n) {
      e2[(size_t)i] = e[i] * e[i];
      e2max = std::max(e2max, e2[(size_t)i]);
    }
  }
  // dstebz: pivmin = safmin max(1, max e^2); the Gershgorin interval widened by 2.1 (n ulp |T| + 2 pivmin)
  const double pivmin = std::numeric_limits<double>::min() * std::max(1.0, e2max);
  const double tnorm = std::max(std::fabs(lo), std::fabs(hi));
  const double widen = 2.1 * tnorm * 0x1p-52 * (double)n + 2.1 * 2.0 * pivmin;
  DevBuf<double> dd, de2, dout;
  prep_alloc(dd, N, "the tridiagonal");
  prep_alloc(de2, N, "the tridiagonal");
  prep_alloc(dout, N, "the eigenvalues");
  HIP_TRY(hipMemcpyAsync(dd.p, d, N * 8, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(de2.p, e2.data(), N * 8, hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(spec_bisect_kernel, dim3((n + kSpecBisectThreads - 1) / kSpecBisectThreads), dim3(kSpecBisectThreads),
                     0, stream, dd.p, de2.p, n, lo - widen, hi + widen, pivmin, dout.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, dout.p, N * 8, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
}

// R/core.R:994-1007 on eigenvalues in descending order.
void spec_characteristics(const double* lam, int n, topolow_spectrum_info* info) {
  int64_t n_pos = 0, n_neg = 0;
  double sum_pos = 0.0, sum_neg = 0.0;
  for (int q = 0; q < n; ++q) {
    if (lam[q] > 1e-12) { ++n_pos; sum_pos += lam[q]; }
    else if (lam[q] < -1e-12) { ++n_neg; sum_neg += std::fabs(lam[q]); }
  }
  int64_t dims = n_pos;   // which(...)[1] is NA: the positive count
  double cum = 0.0;
  for (int q = 0, seen = 0; q < n; ++q) {
    if (!(lam[q] > 1e-12)) continue;
    cum += lam[q];
    ++seen;
    if (cum / sum_pos >= 0.90) { dims = seen; break; }
  }
  info->n_positive = n_pos;
  info->n_negative = n_neg;
  info->sum_positive = sum_pos;
  info->sum_negative = sum_neg;
  info->deviation_score = n_pos > 0 ? sum_neg / sum_pos : 1.0;
  info->dims_90 = (int32_t)std::max<int64_t>(1, dims);
}

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

}  // namespace

int topolow_tridiagonal_eigenvalues(const double* d, const double* e, int32_t n, int32_t device,
                                    double* eigenvalues_out, char* errbuf, size_t errlen) {
  if (!d || !eigenvalues_out || n < 1 || (n >= 2 && !e)) {
    set_err(errbuf, errlen, "topolow_tridiagonal_eigenvalues: d, e (n >= 2) and eigenvalues_out must not be NULL, n >= 1");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (!spec_all_finite(d, (size_t)n) || !spec_all_finite(e, (size_t)n - 1)) {
    set_err(errbuf, errlen, "infinite or missing values in the tridiagonal matrix");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  return guarded(errbuf, errlen, [&] {
    select_device(device);
    PostPipe P;
    P.create(0, 0);
    spec_bisect(d, e, n, P.run, eigenvalues_out);
  });
}

int topolow_symmetric_eigenvalues(const double* a, int32_t n, int32_t device, double* d_out, double* e_out,
                                  double* eigenvalues_out, char* errbuf, size_t errlen) {
  if (!a || n < 1) {
    set_err(errbuf, errlen, "topolow_symmetric_eigenvalues: a must not be NULL, n >= 1");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  for (int32_t c = 0; c < n; ++c)
    if (!spec_all_finite(a + (size_t)c * (size_t)n + (size_t)c, (size_t)(n - c))) {
      set_err(errbuf, errlen, "infinite or missing values in 'x' (column %d of the lower triangle)", (int)c);
      return TOPOLOW_ERR_BAD_ARGUMENT;
    }
  return guarded(errbuf, errlen, [&] {
    select_device(device);
    const size_t N = (size_t)n;
    DevBuf<double> A;
    prep_alloc(A, N * N, "the matrix");
    PostPipe P;
    P.create(0, 0);
    HIP_TRY(hipMemcpyAsync(A.p, a, N * N * 8, hipMemcpyHostToDevice, P.run));
    HIP_TRY(hipStreamSynchronize(P.run));   // the caller's memory is pageable
    hipLaunchKernelGGL(spec_mirror_kernel, dim3(n, (n + kSpecThreads - 1) / kSpecThreads), dim3(kSpecThreads), 0, P.run,
                       A.p, n, 0);
    HIP_TRY(hipGetLastError());
    std::vector<double> d(N), e(N);
    spec_tridiagonalize(A.p, n, P.run, d.data(), e.data());
    if (d_out) std::copy(d.begin(), d.end(), d_out);
    if (e_out) std::copy(e.begin(), e.begin() + (n - 1), e_out);
    if (eigenvalues_out) spec_bisect(d.data(), e.data(), n, P.run, eigenvalues_out);
  });
}

int topolow_layout_prep_spectrum(topolow_layout_prep* p, double* eigenvalues_out, double* centered_out,
                                 topolow_spectrum_info* info, char* errbuf, size_t errlen) {
  if (!p || !info) {
    set_err(errbuf, errlen, "topolow_layout_prep_spectrum: the handle and info must not be NULL");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  return guarded(errbuf, errlen, [&] {
    HIP_TRY(hipSetDevice(p->device));
    *info = topolow_spectrum_info();
    const int n = p->n;
    const size_t N = (size_t)n, cells = N * N;
    const int8_t* codes = p->has_codes ? p->codes.p : nullptr;
    PostPipe P;
    P.create(0, 0);
    const double t0 = now_s();

    // -- the median: 8 passes of 8 bits, both middle ranks at once
    DevBuf<SpecSelect> sel;
    prep_alloc(sel, 1, "the select histograms");
    const int sel_grid = (int)std::min<size_t>((cells + kSpecThreads - 1) / kSpecThreads, 2048);
    unsigned long long prefix[2] = {0, 0}, rank[2] = {0, 0}, n_numeric = 0;
    SpecSelect h;
    for (int shift = 56; shift >= 0; shift -= 8) {
      HIP_TRY(hipMemsetAsync(sel.p, 0, sizeof(SpecSelect), P.run));
      hipLaunchKernelGGL(spec_select_kernel, dim3(sel_grid), dim3(kSpecThreads), 0, P.run, p->vals.p, codes, cells, shift,
                         prefix[0], prefix[1], sel.p);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(&h, sel.p, sizeof(SpecSelect), hipMemcpyDeviceToHost, P.run));
      HIP_TRY(hipStreamSynchronize(P.run));
      if (shift == 56) {
        for (int q = 0; q < 256; ++q) n_numeric += h.hist[0][q];
        if (n_numeric == 0)
          throw HipError{TOPOLOW_ERR_BAD_ARGUMENT, "infinite or missing values in 'x': the matrix holds no numeric cell"};
        if (h.n_infinite > 0)
          throw HipError{TOPOLOW_ERR_BAD_ARGUMENT, "infinite or missing values in 'x': " + std::to_string(h.n_infinite) +
                                                       " numeric cell(s) are infinite"};
        rank[0] = (n_numeric - 1) / 2;
        rank[1] = n_numeric / 2;
      }
      for (int r = 0; r < 2; ++r) prefix[r] |= (unsigned long long)spec_pick_digit(h.hist[r], rank[r]) << shift;
    }
    const double lo_mid = spec_key_value(prefix[0]), hi_mid = spec_key_value(prefix[1]);
    const double median = (n_numeric & 1) ? lo_mid : (lo_mid + hi_mid) / 2.0;
    info->median = median;
    info->n_numeric = (int64_t)n_numeric;
    info->n_filled = (int64_t)(cells - n_numeric);
    const double t1 = now_s();

    // -- the centred matrix
    const int nb = (n + kPrepTile - 1) / kPrepTile;
    DevBuf<double> part_slow, part_fast, sums, B;
    prep_alloc(part_slow, N * (size_t)nb, "the partial sums");
    prep_alloc(part_fast, N * (size_t)nb, "the partial sums");
    prep_alloc(sums, 2 * N, "the sums");
    prep_alloc(B, cells, "the centred matrix");
    hipLaunchKernelGGL(spec_square_sums_kernel, dim3(nb, nb), dim3(kPrepThreads), 0, P.run, p->vals.p, codes, n, median,
                       part_slow.p, part_fast.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(spec_finish_sums_kernel, dim3((n + kPrepThreads - 1) / kPrepThreads), dim3(kPrepThreads), 0, P.run,
                       n, nb, part_slow.p, part_fast.p, sums.p);
    HIP_TRY(hipGetLastError());
    std::vector<double> means(2 * N);
    HIP_TRY(hipMemcpyAsync(means.data(), sums.p, 2 * N * 8, hipMemcpyDeviceToHost, P.run));
    HIP_TRY(hipStreamSynchronize(P.run));
    const size_t row_at = p->transposed ? 0 : N;   // slow lines are rows when transposed
    double grand = 0.0;
    for (size_t i = 0; i < N; ++i) grand += means[row_at + i];
    grand /= (double)n * (double)n;
    for (double& m : means) m /= (double)n;
    HIP_TRY(hipMemcpyAsync(sums.p, means.data(), 2 * N * 8, hipMemcpyHostToDevice, P.run));
    const dim3 lines_grid(n, (n + kSpecThreads - 1) / kSpecThreads);
    hipLaunchKernelGGL(spec_center_kernel, lines_grid, dim3(kSpecThreads), 0, P.run, p->vals.p, codes, n, median, sums.p,
                       grand, p->transposed ? 1 : 0, B.p);
    HIP_TRY(hipGetLastError());
    std::vector<double> diag(N);
    hipLaunchKernelGGL(spec_diagonal_kernel, dim3((n + kSpecThreads - 1) / kSpecThreads), dim3(kSpecThreads), 0, P.run,
                       B.p, n, part_slow.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(diag.data(), part_slow.p, N * 8, hipMemcpyDeviceToHost, P.run));
    if (centered_out) HIP_TRY(hipMemcpyAsync(centered_out, B.p, cells * 8, hipMemcpyDeviceToHost, P.run));
    HIP_TRY(hipStreamSynchronize(P.run));
    for (size_t i = 0; i < N; ++i) info->trace += diag[i];
    hipLaunchKernelGGL(spec_mirror_kernel, lines_grid, dim3(kSpecThreads), 0, P.run, B.p, n, p->transposed ? 1 : 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(P.run));
    const double t2 = now_s();

    // -- the eigenvalues
    std::vector<double> d(N), e(N), lam(N);
    spec_tridiagonalize(B.p, n, P.run, d.data(), e.data());
    const double t3 = now_s();
    if (!spec_all_finite(d.data(), N) || !spec_all_finite(e.data(), N - 1))
      throw HipError{TOPOLOW_ERR_BAD_ARGUMENT, "infinite or missing values in 'x': the squared matrix overflows"};
    spec_bisect(d.data(), e.data(), n, P.run, lam.data());
    const double t4 = now_s();
    if (eigenvalues_out) std::copy(lam.begin(), lam.end(), eigenvalues_out);
    spec_characteristics(lam.data(), n, info);
    info->seconds[0] = t1 - t0;
    info->seconds[1] = t2 - t1;
    info->seconds[2] = t3 - t2;
    info->seconds[3] = t4 - t3;
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
        if (positions_out) download_positions(s0, s0->best.p, positions_out);
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

namespace {

// Which device path an embedding of n points in ndim dimensions takes under `opt`: the decision of
// topolow_optimize_layout_exact, shared with topolow_layout_prep_optimize.
struct LayoutRoute {
  int schedule = TOPOLOW_SCHEDULE_SLAB;   // AUTO resolved
  bool tile_gs = false;                   // schedule gs beyond one workgroup: the session runs tile Gauss-Seidel
};

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

}  // namespace

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
      std::vector<double>* trace_out = verbose ? &trace : nullptr;
      if (precision == TOPOLOW_PRECISION_F32)
        gs_relax<float>(&pb, &res, 1, &dev_s, opt.interrupt_cb, opt.interrupt_user, trace_out);
      else
        gs_relax<double>(&pb, &res, 1, &dev_s, opt.interrupt_cb, opt.interrupt_user, trace_out);
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

int topolow_layout_prep_optimize(topolow_layout_prep* p, const double* initial_positions, int32_t ndim,
                                 int32_t n_iter, double k0, double cooling_rate, double c_repulsion,
                                 double relative_epsilon, int32_t convergence_window, int32_t convergence_check_freq,
                                 int32_t verbose, const topolow_options* opt_in, double* positions_out,
                                 int32_t* converged, int32_t* iterations, double* final_mae, double* final_k,
                                 topolow_run_stats* stats, char* errbuf, size_t errlen) {
  if (!p || !initial_positions || !positions_out || !converged || !iterations || !final_mae || !final_k) {
    set_err(errbuf, errlen, "null argument");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (const int rcu = prep_check_usable(p, errbuf, errlen)) return rcu;
  topolow_options opt;
  if (opt_in) opt = *opt_in; else topolow_default_options(&opt);
  if (opt.n_devices > 1 || opt.devices != nullptr) {
    set_err(errbuf, errlen, "a prepared handle lives on one device: a run sharded over devices takes the arrays "
            "(topolow_layout_prep_fetch, then topolow_optimize_layout_exact)");
    return TOPOLOW_ERR_UNSUPPORTED;
  }
  if (opt.device >= 0 && opt.device != p->device) {
    set_err(errbuf, errlen, "the handle lives on device %d, the options ask for device %d", p->device, opt.device);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  opt.device = p->device;
  const double t_start = now_s();
  const int n = p->n;
  LayoutRoute route;
  if (const int rcr = layout_route(n, ndim, opt, &route, errbuf, errlen)) return rcr;
  int rc = TOPOLOW_OK;
  if (route.schedule == TOPOLOW_SCHEDULE_GS && !route.tile_gs) {
    // one workgroup: the kernel reads the caller-form arrays.  These problems are small (n <= 2048): fetched into
    // temporaries, and the 16-argument entry does the rest -- the same route, the same run.
    const size_t N = (size_t)n, E = (size_t)std::max<int64_t>(p->n_edges, 0);
    const size_t Ea = std::max<size_t>(E, 1);   // fetch() refuses NULL outputs
    std::vector<int32_t> order(N), degrees(N), ei(Ea), ej(Ea), et(Ea), tdense(N * N);
    std::vector<double> ed(Ea), dense(N * N);
    rc = topolow_layout_prep_fetch(p, order.data(), degrees.data(), ei.data(), ej.data(), ed.data(), et.data(),
                                   dense.data(), tdense.data(), nullptr, nullptr, errbuf, errlen);
    if (rc == TOPOLOW_OK)
      rc = topolow_optimize_layout_exact(initial_positions, n, ndim, dense.data(), tdense.data(), degrees.data(),
                                         ei.data(), ej.data(), ed.data(), et.data(), (int64_t)E, n_iter, k0, cooling_rate,
                                         c_repulsion, relative_epsilon, convergence_window, convergence_check_freq,
                                         verbose, &opt, positions_out, converged, iterations, final_mae, final_k, stats,
                                         errbuf, errlen);
  } else {
    rc = run_session_layout(n, ndim, route.tile_gs, opt, [&](topolow_session* s, char* eb, size_t el) -> int {
      return topolow_session_load_prepared(s, p, eb, el);
    }, initial_positions, n_iter, k0, cooling_rate, c_repulsion, relative_epsilon, convergence_window,
    convergence_check_freq, verbose, positions_out, converged, iterations, final_mae, final_k, stats, t_start, errbuf,
    errlen);
  }
  p->resident_seconds[1] = now_s() - t_start;
  return rc;
}

int topolow_layout_prep_post_metrics(topolow_layout_prep* p, const double* positions, int32_t ndim,
                                     double* est_distances, double* sum_abs, int64_t* count, char* errbuf,
                                     size_t errlen) {
  if (!p || !positions || !sum_abs || !count || ndim < 1) {
    set_err(errbuf, errlen, "null argument, or ndim < 1");
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (const int rcu = prep_check_usable(p, errbuf, errlen)) return rcu;
  const double t0 = now_s();
  (void)hipSetDevice(p->device);
  const PostResident resident = {p->vals.p, p->has_codes ? p->codes.p : nullptr, p->order[0] != -1 ? p->ord.p : nullptr};
  const int rc = post_metrics_run(positions, p->n, ndim, nullptr, nullptr, &resident, est_distances, sum_abs, count,
                                  p->device, kPostDefaultStaging, nullptr, errbuf, errlen);
  p->resident_seconds[2] = now_s() - t0;
  return rc;
}

int topolow_layout_prep_order(const topolow_layout_prep* p, int32_t* order, int32_t* degrees) {
  if (!p || p->declined || (!order && !degrees)) return TOPOLOW_ERR_BAD_ARGUMENT;
  if (order) std::copy(p->order.begin(), p->order.end(), order);
  if (degrees) std::copy(p->degrees.begin(), p->degrees.end(), degrees);
  return TOPOLOW_OK;
}

int topolow_layout_prep_resident_seconds(const topolow_layout_prep* p, double* seconds) {
  if (!p || !seconds) return TOPOLOW_ERR_BAD_ARGUMENT;
  for (int q = 0; q < 3; ++q) seconds[q] = p->resident_seconds[q];
  return TOPOLOW_OK;
}

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

}  // namespace

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

namespace {

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

// ---- the fit report of a resident embedding (relax_fit.h) ---------------------------------------------------------------
namespace {

static_assert(kFitMaxRanks == TOPOLOW_FIT_MAX_RANKS, "relax_fit.h and the header disagree");

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

}  // namespace

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
  if (series != TOPOLOW_FIT_IN && series != TOPOLOW_FIT_OUT && series != TOPOLOW_FIT_ALL) {
    set_err(errbuf, errlen, "%s: unknown series %d (TOPOLOW_FIT_IN, _OUT or _ALL)", entry, series);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
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
