// topolow_amd/csrc/topolow_spectrum.hip -- the spectrum entries of libtopolow_relax.so (relax_spectrum.h; reference
// R/core.R:983-1007): all eigenvalues of a tridiagonal and of a symmetric matrix, and the data assessment of a
// prepared handle's resident matrix.

#include "topolow_prep.h"
#include "relax_spectrum.h"

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

}  // namespace

extern "C" {

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

}  // extern "C"
