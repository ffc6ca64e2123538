// topolow_amd/csrc/topolow_cv.hip -- a cross-validation fold on a resident session (relax_cv.h): holding a fold's
// pairs out of the encoded block and of what was derived from it, putting them back, and scoring held-out pairs on the
// positions a run left: topolow_session_hold_out / _restore_held_out / _score_pairs of include/topolow_relax.h, and the
// device halves the folds of a prepared handle (topolow_prep_fold.hip) share with them.

#include "topolow_session.h"
#include "relax_cv.h"

namespace {

template <typename T>
void swap_buf(DevBuf<T>& a, DevBuf<T>& b) { std::swap(a.p, b.p); std::swap(a.n, b.n); }

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

}  // namespace

// ---- the three functions topolow_prep_fold.hip calls as well (declared in topolow_session.h) ----

// The device half of a hold-out, shared by topolow_session_hold_out and the folds prepared on the device
// (topolow_layout_prep_cv_sweep).  fill(lo, hi) enqueues on s->stream whatever writes the n_pairs held-out pairs into
// the two device arrays: session labels, lo < hi, every pair once, in ANY order -- the mask, tile and compaction
// kernels of relax_cv.h need the pairs unique, not sorted.  degrees: the fold's, per caller's point (host).
void cv_hold_out_pairs(topolow_session* s, long long np, const int32_t* degrees, const std::function<void(int*, int*)>& fill) {
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
    hipLaunchKernelGGL((cv_score_kernel<double>), dim3(blocks), dim3(kThreads), 0, s->stream, (const double*)s->best_now(),
                       s->dim, d_i, d_j, d_truth, n_pairs, h.sc_part.p);
  else
    hipLaunchKernelGGL((cv_score_kernel<float>), dim3(blocks), dim3(kThreads), 0, s->stream, (const float*)s->best_now(),
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

extern "C" {

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

}  // extern "C"
