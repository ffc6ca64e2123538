// topolow_amd/csrc/relax_host.h -- host helpers shared by the library's sources (topolow_*.hip) and the host
// halves of their headers (relax_gs.h): error type and HIP check, error text, host threads, the edge-list test.
// Every source includes it, so the functions here are stateless and have internal linkage; HipError alone is ONE
// type for the whole library (hidden, not exported): what one source throws another one's guarded() catches.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <exception>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/topolow_relax.h"

struct __attribute__((visibility("hidden"))) HipError {
  int code;
  std::string msg;
};

namespace {

void set_err(char* errbuf, size_t errlen, const char* fmt, ...) {
  if (!errbuf || errlen == 0) return;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(errbuf, errlen, fmt, ap);
  va_end(ap);
}

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) {                                                             \
      throw HipError{e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice              \
                         ? TOPOLOW_ERR_NO_DEVICE                                        \
                         : TOPOLOW_ERR_HIP,                                             \
                     std::string(#expr) + ": " + hipGetErrorString(e_)};                \
    }                                                                                   \
  } while (0)

// Runs body() and turns what it throws into a result code and the caller's error text.
template <typename F>
int guarded(char* errbuf, size_t errlen, F&& body) {
  try {
    body();
    return TOPOLOW_OK;
  } catch (const HipError& e) {
    set_err(errbuf, errlen, "%s", e.msg.c_str());
    return e.code;
  } catch (const std::bad_alloc&) {
    set_err(errbuf, errlen, "out of host memory");
    return TOPOLOW_ERR_HIP;
  }
}

constexpr size_t kEdgeGrain = (size_t)1 << 18;   // edges per host thread (a one-shot call passes over 10^7..10^8)

// Splits [0, n) into contiguous ranges over at most 16 host threads, one per `grain` items; fewer items run on the
// calling thread.  fn(begin, end) must be thread-safe.  Every worker is joined, then the first exception any range
// threw is rethrown on the calling thread.
template <typename Fn>
void host_parallel(size_t n, size_t grain, Fn fn) {
  const unsigned hw = std::thread::hardware_concurrency();
  const size_t workers = std::max<size_t>(1, std::min<size_t>({n / grain, (size_t)(hw ? hw : 1), (size_t)16}));
  if (workers <= 1) { fn((size_t)0, n); return; }
  std::mutex mu;
  std::exception_ptr first;
  auto run = [&](size_t lo, size_t hi) {
    try {
      fn(lo, hi);
    } catch (...) {
      std::lock_guard<std::mutex> lock(mu);
      if (!first) first = std::current_exception();
    }
  };
  std::vector<std::thread> pool;
  pool.reserve(workers);
  const size_t step = (n + workers - 1) / workers;
  for (size_t lo = 0; lo < n; lo += step) {
    const size_t hi = std::min(n, lo + step);
    try {
      pool.emplace_back(run, lo, hi);
    } catch (...) {
      run(lo, hi);   // no thread to be had: this range runs here
    }
  }
  for (auto& t : pool) t.join();
  if (first) std::rethrow_exception(first);
}

// Is the edge list exactly the measured strict-upper-triangle of the dense inputs (same pairs, same
// targets, same threshold codes)?  Host only: one streaming pass over the upper triangle to count its
// finite cells, one gather per edge; on a few threads unless `threads` is false.  (A pair listed twice
// is not detected here; the slab path cross-checks the count on the device.)
bool edges_are_the_matrix(const double* D, const int32_t* T, int n, const int32_t* ei, const int32_t* ej,
                          const double* ed, const int32_t* et, int64_t n_edges, bool threads) {
  const size_t grain = threads ? kEdgeGrain : SIZE_MAX;
  std::atomic<long long> finite{0};
  host_parallel((size_t)n, grain, [&](size_t lo, size_t hi) {   // columns; work grows with j, close enough
    long long c = 0;
    for (size_t j = lo; j < hi; ++j) {
      const double* col = D + j * (size_t)n;
      for (size_t i = 0; i < j; ++i) c += std::isfinite(col[i]) ? 1 : 0;
    }
    finite.fetch_add(c);
  });
  if (finite.load() != (long long)n_edges) return false;
  std::atomic<bool> ok{true};
  host_parallel((size_t)n_edges, grain, [&](size_t lo, size_t hi) {
    for (size_t e = lo; e < hi; ++e) {
      const int a = ei[e], b = ej[e];
      if (a < 0 || b <= a || b >= n) { ok.store(false); return; }
      const size_t cell = (size_t)a + (size_t)b * n;
      const int tc = T[cell], ec = et[e];
      const int tn = tc == 0 ? 0 : (tc == 1 ? 1 : -1), en = ec == 0 ? 0 : (ec == 1 ? 1 : -1);
      if (!(D[cell] == ed[e]) || !std::isfinite(ed[e]) || tn != en) { ok.store(false); return; }
    }
  });
  return ok.load();
}

}  // namespace
