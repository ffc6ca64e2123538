// topolow_amd/csrc/topolow_reduce.hip -- plot coordinates of libtopolow_relax.so: topolow_scale_objective, its _ex
// twin and topolow_scale_to_original_distances over the kernels of relax_reduce.h.  A source of its own: the step
// reads two coordinate arrays and needs neither a session nor a prepared handle.
//
// Replaces the n x n matrices and the objective of the reference's scale_to_original_distances
// (R/visualization.R:624-640); the minimiser is Brent's fmin, the algorithm behind R's optimize.

#include "topolow_session.h"
#include "relax_reduce.h"

#include <cfloat>

namespace {

constexpr int kRedMaxDim = 16;

// Columns per unit when the caller names none: a function of n alone, so a given n always adds in one order.
// 256 up to 16 384 points (N = 10 000: 40 row blocks, 820 units in the triangle -- three waves on every SIMD of the
// card); beyond that n / 64 rounded up to a multiple of 256, which keeps a row block at 64 units or fewer.
int reduce_default_chunk(int n) { return n <= 16384 ? 256 : ((n / 64 + 255) / 256) * 256; }

bool reduce_chunk_ok(int chunk) { return chunk == 0 || chunk == 64 || chunk == 128 || chunk == 256 || chunk == 512; }

// The units of the triangle j < i, row block by row block, columns ascending: (b, c) exists iff column c * chunk is
// below the block's last row.
std::vector<int2> reduce_units(int n, int chunk) {
  std::vector<int2> units;
  const int row_blocks = (n + kRedThreads - 1) / kRedThreads;
  for (int b = 0; b < row_blocks; ++b) {
    const int last_row = std::min((b + 1) * kRedThreads, n) - 1;
    for (int c = 0; (long long)c * chunk < last_row; ++c) units.push_back(make_int2(b, c));
  }
  return units;
}

struct RedEvents {
  hipEvent_t a = nullptr, b = nullptr;
  void create() {
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
  }
  ~RedEvents() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
  RedEvents() = default;
  RedEvents(const RedEvents&) = delete;
  RedEvents& operator=(const RedEvents&) = delete;
};

// k <= 2 runs with two reduced coordinates (one when ndim is 1), more with as many as the positions: a zero
// coordinate adds exactly 0 to r^2.  m = 1 has an instance of its own (the minimiser's), 2..8 run as 8 with scales 0.
template <int DIM>
void reduce_launch(bool narrow, bool single, int units, const double* pos, const double* red, const int2* unit_list, int n,
                   int chunk, const ReduceScales& scales, double* part) {
  constexpr int K2 = DIM < 2 ? DIM : 2;
  const dim3 grid(units), block(kRedThreads);
  if (narrow && single)
    hipLaunchKernelGGL((scale_objective_partial_kernel<DIM, K2, 1>), grid, block, 0, nullptr, pos, red, unit_list, n, chunk,
                       scales, part);
  else if (narrow)
    hipLaunchKernelGGL((scale_objective_partial_kernel<DIM, K2, kRedMaxScales>), grid, block, 0, nullptr, pos, red,
                       unit_list, n, chunk, scales, part);
  else if (single)
    hipLaunchKernelGGL((scale_objective_partial_kernel<DIM, DIM, 1>), grid, block, 0, nullptr, pos, red, unit_list, n, chunk,
                       scales, part);
  else
    hipLaunchKernelGGL((scale_objective_partial_kernel<DIM, DIM, kRedMaxScales>), grid, block, 0, nullptr, pos, red,
                       unit_list, n, chunk, scales, part);
}

#define TL_RED_DIM(dim, ...)                                \
  switch (dim) {                                            \
    case 1: reduce_launch<1>(__VA_ARGS__); break;           \
    case 2: reduce_launch<2>(__VA_ARGS__); break;           \
    case 3: reduce_launch<3>(__VA_ARGS__); break;           \
    case 4: reduce_launch<4>(__VA_ARGS__); break;           \
    case 5: reduce_launch<5>(__VA_ARGS__); break;           \
    case 6: reduce_launch<6>(__VA_ARGS__); break;           \
    case 7: reduce_launch<7>(__VA_ARGS__); break;           \
    case 8: reduce_launch<8>(__VA_ARGS__); break;           \
    case 9: reduce_launch<9>(__VA_ARGS__); break;           \
    case 10: reduce_launch<10>(__VA_ARGS__); break;         \
    case 12: reduce_launch<12>(__VA_ARGS__); break;         \
    default: reduce_launch<16>(__VA_ARGS__); break;         \
  }

// X and Y on the device, the unit list, the partials: uploaded once, evaluated any number of times.
struct ReducePass {
  int n = 0, dim = 0, kdim = 0, chunk = 0, units = 0;
  bool narrow = false;
  DevBuf<double> pos, red, part, out;
  DevBuf<int2> unit_list;

  void upload(const double* positions, const double* reduced, int n_, int ndim, int k, int chunk_cols) {
    n = n_;
    dim = kernel_dim(ndim);   // 11 runs as 12, 13..15 as 16: a zero coordinate adds exactly 0 to every distance
    narrow = k <= 2;
    kdim = narrow ? std::min(2, dim) : dim;
    chunk = chunk_cols > 0 ? chunk_cols : reduce_default_chunk(n);
    const size_t N = (size_t)n;
    std::vector<double> hp(N * (size_t)dim, 0.0), hr(N * (size_t)kdim, 0.0);
    memcpy(hp.data(), positions, N * (size_t)ndim * 8);
    memcpy(hr.data(), reduced, N * (size_t)k * 8);
    const std::vector<int2> list = reduce_units(n, chunk);
    units = (int)list.size();
    pos.alloc(hp.size());
    red.alloc(hr.size());
    unit_list.alloc(list.size());
    part.alloc(list.size() * (size_t)(kRedMaxScales + 2));
    out.alloc(kRedMaxScales + 2);
    HIP_TRY(hipMemcpy(pos.p, hp.data(), hp.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(red.p, hr.data(), hr.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(unit_list.p, list.data(), list.size() * sizeof(int2), hipMemcpyHostToDevice));
  }

  // one launch pair; result: F_0 .. F_{m-1}, G, H
  void launch(const double* scales, int m) {
    ReduceScales s;
    for (int q = 0; q < kRedMaxScales; ++q) s.s[q] = q < m ? scales[q] : 0.0;
    const bool single = m == 1;
    TL_RED_DIM(dim, narrow, single, units, pos.p, red.p, unit_list.p, n, chunk, s, part.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(scale_objective_combine_kernel, dim3(1), dim3(kRedThreads), 0, nullptr, part.p, units,
                       (single ? 1 : kRedMaxScales) + 2, m, out.p);
    HIP_TRY(hipGetLastError());
  }

  void fetch(double* result, int m) { HIP_TRY(hipMemcpy(result, out.p, (size_t)(m + 2) * 8, hipMemcpyDeviceToHost)); }
};

// what the three entries share; 0 = fine
int reduce_check_inputs(const char* fn, const double* positions, const double* reduced, int32_t n, int32_t ndim, int32_t k,
                        char* errbuf, size_t errlen) {
  if (!positions || !reduced) {
    set_err(errbuf, errlen, "%s: positions and reduced must not be NULL", fn);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (n < 2) {
    set_err(errbuf, errlen, "%s: needs n >= 2 (one pair of points)", fn);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (k < 1 || k > ndim) {
    set_err(errbuf, errlen, "%s: needs 1 <= k <= ndim", fn);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (ndim > kRedMaxDim) {
    set_err(errbuf, errlen, "%s: ndim must be between 1 and %d", fn, kRedMaxDim);
    return TOPOLOW_ERR_UNSUPPORTED;
  }
  if (n > (1 << 30)) {
    set_err(errbuf, errlen, "%s: n must be at most 2^30", fn);
    return TOPOLOW_ERR_UNSUPPORTED;
  }
  const size_t N = (size_t)n;
  for (size_t i = 0; i < N * (size_t)ndim; ++i)
    if (!std::isfinite(positions[i])) {
      set_err(errbuf, errlen, "%s: positions[%zu, %zu] is not finite", fn, i % N, i / N);
      return TOPOLOW_ERR_BAD_ARGUMENT;
    }
  for (size_t i = 0; i < N * (size_t)k; ++i)
    if (!std::isfinite(reduced[i])) {
      set_err(errbuf, errlen, "%s: reduced[%zu, %zu] is not finite", fn, i % N, i / N);
      return TOPOLOW_ERR_BAD_ARGUMENT;
    }
  return TOPOLOW_OK;
}

}  // namespace

extern "C" {

int topolow_scale_objective_ex(const double* positions, const double* reduced, int32_t n, int32_t ndim, int32_t k,
                               const double* scales, int32_t m, double* objective, double* sum_orig, double* sum_reduced,
                               int32_t device, int32_t chunk_cols, double* seconds, char* errbuf, size_t errlen) {
  const char* fn = "topolow_scale_objective";
  if (!scales || !objective) {
    set_err(errbuf, errlen, "%s: scales and objective must not be NULL", fn);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (m < 1 || m > kRedMaxScales) {
    set_err(errbuf, errlen, "%s: m must be between 1 and %d", fn, kRedMaxScales);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  for (int q = 0; q < m; ++q)
    if (!std::isfinite(scales[q])) {
      set_err(errbuf, errlen, "%s: scales[%d] is not finite", fn, q);
      return TOPOLOW_ERR_BAD_ARGUMENT;
    }
  if (!reduce_chunk_ok(chunk_cols)) {
    set_err(errbuf, errlen, "%s: chunk_cols must be 0 (the library's width), 64, 128, 256 or 512", fn);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (const int rc = reduce_check_inputs(fn, positions, reduced, n, ndim, k, errbuf, errlen)) return rc;
  return guarded(errbuf, errlen, [&] {
    select_device(device);
    ReducePass pass;
    pass.upload(positions, reduced, n, ndim, k, chunk_cols);
    RedEvents ev;
    if (seconds) {
      ev.create();
      HIP_TRY(hipEventRecord(ev.a, nullptr));
    }
    pass.launch(scales, m);
    if (seconds) HIP_TRY(hipEventRecord(ev.b, nullptr));
    double result[kRedMaxScales + 2];
    pass.fetch(result, m);
    for (int q = 0; q < m; ++q) objective[q] = result[q];
    if (sum_orig) *sum_orig = result[m];
    if (sum_reduced) *sum_reduced = result[m + 1];
    if (seconds) {
      float ms = 0.0f;
      HIP_TRY(hipEventSynchronize(ev.b));
      HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
      *seconds = 1e-3 * ms;
    }
  });
}

int topolow_scale_objective(const double* positions, const double* reduced, int32_t n, int32_t ndim, int32_t k,
                            const double* scales, int32_t m, double* objective, double* sum_orig, double* sum_reduced,
                            int32_t device, char* errbuf, size_t errlen) {
  return topolow_scale_objective_ex(positions, reduced, n, ndim, k, scales, m, objective, sum_orig, sum_reduced, device, 0,
                                    nullptr, errbuf, errlen);
}

int topolow_scale_to_original_distances(const double* positions, const double* reduced, int32_t n, int32_t ndim, int32_t k,
                                        double lower, double upper, double tol, double* scale, double* objective,
                                        int32_t* evaluations, double* trace_scale, double* trace_objective,
                                        int32_t trace_len, int32_t device, char* errbuf, size_t errlen) {
  const char* fn = "topolow_scale_to_original_distances";
  if (!scale) {
    set_err(errbuf, errlen, "%s: scale must not be NULL", fn);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (!std::isfinite(lower) || !std::isfinite(upper) || !std::isfinite(tol)) {
    set_err(errbuf, errlen, "%s: lower, upper and tol must be finite", fn);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (!(lower < upper)) {
    set_err(errbuf, errlen, "%s: needs lower < upper", fn);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (!(tol > 0.0)) {
    set_err(errbuf, errlen, "%s: tol must be > 0", fn);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (trace_len < 0 || (trace_len > 0 && (!trace_scale != !trace_objective))) {
    set_err(errbuf, errlen, "%s: trace_len must be >= 0 and the two trace arrays given together", fn);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (const int rc = reduce_check_inputs(fn, positions, reduced, n, ndim, k, errbuf, errlen)) return rc;
  return guarded(errbuf, errlen, [&] {
    select_device(device);
    ReducePass pass;
    pass.upload(positions, reduced, n, ndim, k, 0);
    int32_t evals = 0;
    auto f = [&](double s) {
      double result[3];
      pass.launch(&s, 1);
      pass.fetch(result, 1);
      if (trace_scale && trace_objective && evals < trace_len) {
        trace_scale[evals] = s;
        trace_objective[evals] = result[0];
      }
      ++evals;
      return result[0];
    };

    // Brent's fmin (Algorithms for Minimization without Derivatives, 1973, ch. 5): golden section with parabolic
    // steps; x the best point so far, w the second best, v the previous w; [a, b] brackets the minimum.
    const double golden = 0.5 * (3.0 - std::sqrt(5.0));
    const double eps = std::sqrt(DBL_EPSILON), tol3 = tol / 3.0;
    double a = lower, b = upper;
    double x = a + golden * (b - a), w = x, v = x;
    double d = 0.0, e = 0.0;
    double fx = f(x), fw = fx, fv = fx;
    for (;;) {
      const double xm = 0.5 * (a + b);
      const double tol1 = eps * std::fabs(x) + tol3, t2 = 2.0 * tol1;
      if (std::fabs(x - xm) <= t2 - 0.5 * (b - a)) break;
      double p = 0.0, q = 0.0, r = 0.0;
      if (std::fabs(e) > tol1) {   // fit a parabola through x, w, v
        r = (x - w) * (fx - fv);
        q = (x - v) * (fx - fw);
        p = (x - v) * q - (x - w) * r;
        q = 2.0 * (q - r);
        if (q > 0.0) p = -p; else q = -q;
        r = e;
        e = d;
      }
      if (std::fabs(p) >= std::fabs(0.5 * q * r) || p <= q * (a - x) || p >= q * (b - x)) {
        e = x < xm ? b - x : a - x;   // a golden-section step into the larger part
        d = golden * e;
      } else {
        d = p / q;                    // the parabola's step
        const double u = x + d;
        if (u - a < t2 || b - u < t2) d = x < xm ? tol1 : -tol1;   // not too close to the ends
      }
      // f is never evaluated closer than tol1 to x
      const double u = std::fabs(d) >= tol1 ? x + d : (d > 0.0 ? x + tol1 : x - tol1);
      const double fu = f(u);
      if (fu <= fx) {
        if (u < x) b = x; else a = x;
        v = w; fv = fw;
        w = x; fw = fx;
        x = u; fx = fu;
      } else {
        if (u < x) a = u; else b = u;
        if (fu <= fw || w == x) {
          v = w; fv = fw;
          w = u; fw = fu;
        } else if (fu <= fv || v == x || v == w) {
          v = u; fv = fu;
        }
      }
    }
    *scale = x;
    if (objective) *objective = fx;
    if (evaluations) *evaluations = evals;
  });
}

}  // extern "C"
