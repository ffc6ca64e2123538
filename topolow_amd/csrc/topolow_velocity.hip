// topolow_amd/csrc/topolow_velocity.hip -- antigenic velocities of libtopolow_relax.so: topolow_kernel_velocity and
// its _ex twin over the kernels of relax_velocity.h.  A source of its own: the step reads positions and times and
// needs neither a session nor a prepared handle.
//
// Replaces the reference's compute_kernel_velocity (R/visualization.R:802-843), an R loop over the rows.

#include "topolow_session.h"
#include "relax_velocity.h"

namespace {

constexpr int kVelMaxDim = 16;

// Columns per chunk when the caller names none: a function of n alone, so a given n always adds in one order.
// 256 up to 16 384 points (N = 10 000: 40 row blocks x 40 chunks, about 820 of them inside the lower triangle --
// three to four waves on every SIMD of the card); beyond that n / 64 rounded up to a multiple of 256, which keeps the
// partials at 64 chunks or fewer.
int velocity_default_chunk(int n) { return n <= 16384 ? 256 : ((n / 64 + 255) / 256) * 256; }

// a double's bit pattern as an unsigned key that sorts like the number (NaNs beyond the infinities of their sign)
uint64_t velocity_order_key(double v) {
  uint64_t u;
  memcpy(&u, &v, sizeof u);
  return (u >> 63) ? ~u : (u | ((uint64_t)1 << 63));
}

struct VelEvents {
  hipEvent_t a = nullptr, b = nullptr;
  void create() {
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
  }
  ~VelEvents() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
  VelEvents() = default;
  VelEvents(const VelEvents&) = delete;
  VelEvents& operator=(const VelEvents&) = delete;
};

template <int DIM>
void velocity_launch(bool with_bits, dim3 grid, const double* pos, const double* times, const int32_t* past,
                     const uint64_t* bits, int n, int words, int chunk, double hx, double ht, double* part) {
  if (with_bits)
    hipLaunchKernelGGL((velocity_partial_kernel<DIM, true>), grid, dim3(kVelThreads), 0, nullptr, pos, times, past, bits,
                       n, words, chunk, hx, ht, part);
  else
    hipLaunchKernelGGL((velocity_partial_kernel<DIM, false>), grid, dim3(kVelThreads), 0, nullptr, pos, times, past,
                       nullptr, n, words, chunk, hx, ht, part);
}

#define TL_VEL_DIM(dim, ...)                                  \
  switch (dim) {                                              \
    case 1: velocity_launch<1>(__VA_ARGS__); break;           \
    case 2: velocity_launch<2>(__VA_ARGS__); break;           \
    case 3: velocity_launch<3>(__VA_ARGS__); break;           \
    case 4: velocity_launch<4>(__VA_ARGS__); break;           \
    case 5: velocity_launch<5>(__VA_ARGS__); break;           \
    case 6: velocity_launch<6>(__VA_ARGS__); break;           \
    case 7: velocity_launch<7>(__VA_ARGS__); break;           \
    case 8: velocity_launch<8>(__VA_ARGS__); break;           \
    case 9: velocity_launch<9>(__VA_ARGS__); break;           \
    case 10: velocity_launch<10>(__VA_ARGS__); break;         \
    case 12: velocity_launch<12>(__VA_ARGS__); break;         \
    default: velocity_launch<16>(__VA_ARGS__); break;         \
  }

}  // namespace

extern "C" {

int topolow_kernel_velocity_ex(const double* positions, const double* times, int32_t n, int32_t ndim, double sigma_t,
                               double sigma_x, const uint64_t* excluded_bits, double* velocity, double* weight_sum,
                               int32_t device, int32_t chunk_cols, double* seconds, char* errbuf, size_t errlen) {
  const char* fn = "topolow_kernel_velocity";
  if (!positions || !times || !velocity) {
    set_err(errbuf, errlen, "%s: positions, times and velocity must not be NULL", fn);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (n < 1 || ndim < 1) {
    set_err(errbuf, errlen, "%s: needs n >= 1 and ndim >= 1", fn);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (!std::isfinite(sigma_t) || !(sigma_t > 0.0) || !std::isfinite(sigma_x) || !(sigma_x > 0.0)) {
    set_err(errbuf, errlen, "%s: sigma_t and sigma_x must be finite and > 0", fn);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (chunk_cols < 0 || chunk_cols % kVelTile != 0) {
    set_err(errbuf, errlen, "%s: chunk_cols must be 0 (the library's width) or a positive multiple of %d", fn, kVelTile);
    return TOPOLOW_ERR_BAD_ARGUMENT;
  }
  if (ndim > kVelMaxDim) {
    set_err(errbuf, errlen, "%s: ndim must be between 1 and %d", fn, kVelMaxDim);
    return TOPOLOW_ERR_UNSUPPORTED;
  }
  if (n > (1 << 30)) {
    set_err(errbuf, errlen, "%s: n must be at most 2^30", fn);
    return TOPOLOW_ERR_UNSUPPORTED;
  }
  return guarded(errbuf, errlen, [&] {
    select_device(device);
    const size_t N = (size_t)n;
    const int dim = kernel_dim(ndim);   // 11 runs as 12, 13..15 as 16: a zero coordinate adds exactly 0 to every distance
    const int chunk = chunk_cols > 0 ? chunk_cols : velocity_default_chunk(n);
    const int words = (n + 63) / 64;

    // sorted order: ascending time, NaN last, stable -- except that points of EQUAL time stand in the order of their
    // coordinates (compared as bit patterns, a total order), so that the order of a row's additions, and with it
    // every bit of the result, does not depend on the order the caller lists the points in.  Points equal in time and
    // in every coordinate add the same terms wherever they stand; those keep the caller's order -- which shows only
    // when exclusion bits differ between such twins: a row that takes one and not the other then adds the term at the
    // place of the one it takes (include/topolow_relax.h says so).
    std::vector<int32_t> perm(N);
    for (size_t i = 0; i < N; ++i) perm[i] = (int32_t)i;
    std::stable_sort(perm.begin(), perm.end(), [&](int32_t a, int32_t b) {
      const double ta = times[a], tb = times[b];
      if (std::isnan(ta) || std::isnan(tb)) return !std::isnan(ta) && std::isnan(tb);
      if (ta != tb) return ta < tb;
      for (int d = 0; d < ndim; ++d) {
        const uint64_t ka = velocity_order_key(positions[(size_t)d * N + (size_t)a]);
        const uint64_t kb = velocity_order_key(positions[(size_t)d * N + (size_t)b]);
        if (ka != kb) return ka < kb;
      }
      return false;
    });
    std::vector<double> st(N), sp(N * (size_t)dim, 0.0);
    for (size_t i = 0; i < N; ++i) st[i] = times[perm[i]];
    for (int d = 0; d < ndim; ++d)
      for (size_t i = 0; i < N; ++i) sp[(size_t)d * N + i] = positions[(size_t)d * N + (size_t)perm[i]];
    // past[i]: the points strictly before row i are the sorted columns [0, past[i]); a tie starts where its first
    // member stands, a NaN time has no past
    std::vector<int32_t> past(N);
    int32_t max_past = 0;
    for (size_t i = 0; i < N; ++i) {
      if (std::isnan(st[i])) past[i] = 0;
      else past[i] = (i > 0 && st[i - 1] == st[i]) ? past[i - 1] : (int32_t)i;
      max_past = std::max(max_past, past[i]);
    }
    const int chunks = std::max(1, (max_past + chunk - 1) / chunk);

    // the exclusion bits in sorted order; only the bits of a row's past are ever read
    std::vector<uint64_t> sbits;
    if (excluded_bits) {
      sbits.assign(N * (size_t)words, 0);
      const size_t grain = std::max<size_t>(1, ((size_t)4 << 20) / N);
      host_parallel(N, grain, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i) {
          const uint64_t* src = excluded_bits + (size_t)perm[i] * words;
          uint64_t* dst = sbits.data() + i * words;
          for (int32_t j = 0; j < past[i]; ++j) {
            const uint32_t c = (uint32_t)perm[(size_t)j];
            dst[j >> 6] |= ((src[c >> 6] >> (c & 63)) & 1ull) << (j & 63);
          }
        }
      });
    }

    DevBuf<double> dpos, dt, dpart, dvel, dw;
    DevBuf<int32_t> dpast, dperm;
    DevBuf<uint64_t> dbits;
    dpos.alloc(sp.size());
    dt.alloc(N);
    dpast.alloc(N);
    dperm.alloc(N);
    dpart.alloc((size_t)chunks * (size_t)(dim + 1) * N);
    dvel.alloc(N * (size_t)ndim);
    dw.alloc(N);
    HIP_TRY(hipMemcpy(dpos.p, sp.data(), sp.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dt.p, st.data(), N * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dpast.p, past.data(), N * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dperm.p, perm.data(), N * 4, hipMemcpyHostToDevice));
    if (excluded_bits) {
      dbits.alloc(sbits.size());
      HIP_TRY(hipMemcpy(dbits.p, sbits.data(), sbits.size() * 8, hipMemcpyHostToDevice));
    }

    VelEvents ev;
    if (seconds) {
      ev.create();
      HIP_TRY(hipEventRecord(ev.a, nullptr));
    }
    const int row_blocks = (n + kVelThreads - 1) / kVelThreads;
    const double hx = 1.0 / (2.0 * sigma_x * sigma_x), ht = 1.0 / (2.0 * sigma_t * sigma_t);
    TL_VEL_DIM(dim, excluded_bits != nullptr, dim3(row_blocks, chunks), dpos.p, dt.p, dpast.p, dbits.p, n, words, chunk,
               hx, ht, dpart.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(velocity_combine_kernel, dim3(row_blocks), dim3(kVelThreads), 0, nullptr, dpart.p, dpast.p, dperm.p,
                       n, ndim, dim + 1, chunk, dvel.p, dw.p);
    HIP_TRY(hipGetLastError());
    if (seconds) HIP_TRY(hipEventRecord(ev.b, nullptr));
    HIP_TRY(hipMemcpy(velocity, dvel.p, N * (size_t)ndim * 8, hipMemcpyDeviceToHost));
    if (weight_sum) HIP_TRY(hipMemcpy(weight_sum, dw.p, N * 8, hipMemcpyDeviceToHost));
    if (seconds) {
      float ms = 0.0f;
      HIP_TRY(hipEventSynchronize(ev.b));
      HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
      *seconds = 1e-3 * ms;
    }
  });
}

int topolow_kernel_velocity(const double* positions, const double* times, int32_t n, int32_t ndim, double sigma_t,
                            double sigma_x, const uint64_t* excluded_bits, double* velocity, double* weight_sum,
                            int32_t device, char* errbuf, size_t errlen) {
  return topolow_kernel_velocity_ex(positions, times, n, ndim, sigma_t, sigma_x, excluded_bits, velocity, weight_sum,
                                    device, 0, nullptr, errbuf, errlen);
}

}  // extern "C"
