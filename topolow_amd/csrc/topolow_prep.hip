// topolow_amd/csrc/topolow_prep.hip -- the prepared handle of libtopolow_relax.so: create, fetch and destroy,
// connectivity, subsample, degrees, prune and spectrum of a resident matrix, and the entries that run from a handle:
// optimize, post-metrics, the folds, the CV sweep and the fit report.  One source, because relax_prep_fold.h and
// relax_fit.h build on the device functions of relax_prep.h and both halves fetch their sums through PrepSums.

#include "topolow_prep.h"
#include "topolow_drivers.h"
#include "relax_fold.h"
#include "relax_prep.h"
#include "relax_prep_fold.h"
#include "relax_prep_graph.h"
#include "relax_prep_prune.h"
#include "relax_spectrum.h"
#include "relax_fit.h"

// PrepSums (topolow_prep.h).  Behind the tile kernels on `stream`: the partials added per point, all of it sent down;
// the caller synchronises.
template <typename Totals>
void PrepSums<Totals>::fetch(int n, hipStream_t stream) {
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

namespace {

// Counts per column -> exclusive offsets, off[0 .. n]; returns the total.
int64_t prep_offsets(const int32_t* per_col, size_t n, int64_t* off) {
  off[0] = 0;
  for (size_t j = 0; j < n; ++j) off[j + 1] = off[j] + per_col[j];
  return off[n];
}

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

}  // namespace

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

extern "C" {

namespace {

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
