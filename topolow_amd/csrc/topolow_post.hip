// topolow_amd/csrc/topolow_post.hip -- the post-metrics of libtopolow_relax.so: est_distances, and est_distances with
// the terms of mae in one pass over the caller's matrices or a prepared handle's resident ones.  The only source that
// includes relax_post.h: its kernels are plain __global__ functions and compile wherever the header is read.

#include "topolow_prep.h"
#include "relax_post.h"

// ---- post-metrics: est_distances and the terms of mae in one pass (R/core.R:474-481) ----
// The caller's matrices travel in tiles of whole columns (contiguous in column-major storage).  A tile's upload, the
// kernel of the tile before it and the download of the est tile before that run on three streams and overlap; kPostSlots
// sets of buffers go round, ordered by events.  What is allocated is bounded whatever n is: per slot one tile of values,
// of codes and of est on the device (<= kPostTileBytes each while a column fits in that), and as much pinned memory when
// the staging is PINNED.
namespace {

constexpr size_t kPostTileBytes = (size_t)32 << 20;   // of `values` per tile

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

}  // namespace

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

extern "C" {

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
      dim3 grid(rows, (n + kPostThreads - 1) / kPostThreads);
      hipLaunchKernelGGL(pdist_kernel, grid, dim3(kPostThreads), 0, 0, dp.p, n, ndim, r0, rows, dout.p);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpy(out + (size_t)(r0 - row_begin) * n, dout.p, (size_t)rows * n * 8, hipMemcpyDeviceToHost));
    }
  });
}

int topolow_est_distances(const double* positions, int32_t n, int32_t ndim,
                          double* est_distances, int32_t device, char* errbuf, size_t errlen) {
  return topolow_est_distances_rows(positions, n, ndim, 0, n, est_distances, device, errbuf, errlen);
}

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

}  // extern "C"
