// topolow_amd/csrc/topolow_prep_graph.hip -- the measurement graph of a prepared handle: connectivity and sub-handles
// (relax_prep_graph.h), degrees and pruning (relax_prep_prune.h).  One source, because both halves start from the
// bits graph_bits_kernel leaves (graph_line_bits).  A sub-handle goes through prep_passes of topolow_prep.hip.

#include "topolow_prep.h"
#include "relax_prep_graph.h"
#include "relax_prep_prune.h"

namespace {

// The rules the graph entries share for `subset` (NULL: all n points); no device call.  n is the handle's.
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

// The bit-adjacency pass of p[subset, subset] (NULL: all of it, M = n) on `stream`: the subset goes up, then
// graph_bits_kernel leaves the bits in buffer coordinates (M x words; bit (l, c): cell (l, c) of the buffer is
// measured) and every line's first neighbour in `first`; returns the set bits.  `then` enqueues what the caller has
// behind the kernel, before the count is read back; `stream` is idle when this returns.
unsigned long long graph_line_bits(const topolow_layout_prep* p, const int32_t* subset, int M, int words, hipStream_t stream,
                                   unsigned long long* bits, int32_t* first, const std::function<void()>& then = nullptr) {
  DevBuf<int32_t> sub;
  DevBuf<unsigned long long> cells;
  if (subset != nullptr) prep_alloc(sub, (size_t)M, "the subset");
  prep_alloc(cells, 1, "the cell count");
  if (subset != nullptr) HIP_TRY(hipMemcpyAsync(sub.p, subset, (size_t)M * 4, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemsetAsync(cells.p, 0, sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(graph_bits_kernel, dim3(M), dim3(kGraphThreads), 0, stream, p->vals.p, p->n,
                     subset != nullptr ? sub.p : nullptr, M, words, bits, first, cells.p);
  HIP_TRY(hipGetLastError());
  if (then) then();
  unsigned long long set_bits = 0;
  HIP_TRY(hipMemcpyAsync(&set_bits, cells.p, sizeof set_bits, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return set_bits;
}

static_assert(kPruneConverged == TOPOLOW_PRUNE_CONVERGED && kPruneMinPoints == TOPOLOW_PRUNE_MIN_POINTS &&
                  kPruneMaxIterations == TOPOLOW_PRUNE_MAX_ITERATIONS && kPruneAllRemoved == TOPOLOW_PRUNE_ALL_REMOVED,
              "the kernels' stop reasons are the header's");

constexpr int kPruneBatch = 8;   // rounds launched between two reads of the state

// The row-oriented bits of parent[subset, subset] (M x words; bit (r, c): cell (r, c) is measured) into `bits`, on
// `stream`; returns the set bits.  Where a buffer line is a matrix column the line bits are turned round and freed.
unsigned long long prune_row_bits(const topolow_layout_prep* p, const int32_t* subset, int M, int words, hipStream_t stream,
                                  DevBuf<unsigned long long>& bits) {
  DevBuf<int32_t> first;
  DevBuf<unsigned long long> line_bits;
  const size_t count = (size_t)M * (size_t)words;
  prep_alloc(first, (size_t)M, "the first neighbours");
  DevBuf<unsigned long long>& by_line = p->transposed ? bits : line_bits;
  prep_alloc(by_line, count, "the bit adjacency");
  return graph_line_bits(p, subset, M, words, stream, by_line.p, first.p, [&] {
    if (p->transposed) return;
    prep_alloc(bits, count, "the transposed bit adjacency");
    const long long tiles = (long long)words * (long long)words;
    hipLaunchKernelGGL(prune_bits_transpose_kernel, dim3((unsigned)((tiles + kGraphWaves - 1) / kGraphWaves)),
                       dim3(kGraphThreads), 0, stream, line_bits.p, M, words, bits.p);
    HIP_TRY(hipGetLastError());
  });
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

extern "C" {

// ---- the measurement graph of a handle and its sub-handles (relax_prep_graph.h) ----

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
    DevBuf<int32_t> parent, changed;
    DevBuf<unsigned long long> bits;
    prep_alloc(parent, (size_t)M, "the component labels");
    prep_alloc(changed, 1, "the round flag");
    prep_alloc(bits, (size_t)M * (size_t)words, "the bit adjacency");
    PostPipe P;
    P.create(0, 0);
    const unsigned long long set_bits = graph_line_bits(p, subset, M, words, P.run, bits.p, parent.p);
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

}  // extern "C"
