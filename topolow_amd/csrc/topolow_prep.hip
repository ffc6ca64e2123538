// topolow_amd/csrc/topolow_prep.hip -- the prepared handle of libtopolow_relax.so: create, fetch and destroy, the two
// passes a handle goes through (prep_passes, which a sub-handle of topolow_prep_graph.hip goes through as well), and
// optimize and post-metrics from a handle.  It owns the kernels of relax_prep.h, so PrepSums<>::fetch is defined here
// for both kinds of totals.  The handle's other entries: topolow_prep_graph.hip, topolow_spectrum.hip,
// topolow_prep_fold.hip.

#include "topolow_prep.h"
#include "topolow_drivers.h"
#include "relax_prep.h"

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
template void PrepSums<PrepTotals>::fetch(int, hipStream_t);   // the full matrix (prep_passes)
template void PrepSums<FoldTotals>::fetch(int, hipStream_t);   // a fold's masked one (topolow_prep_fold.hip)

namespace {

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

bool prep_is_permutation(const int32_t* order, int n) {
  std::vector<char> seen((size_t)n, 0);
  for (int q = 0; q < n; ++q) {
    if (order[q] < 0 || order[q] >= n || seen[(size_t)order[q]]) return false;
    seen[(size_t)order[q]] = 1;
  }
  return true;
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

extern "C" {

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

}  // extern "C"
