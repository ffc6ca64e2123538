// topolow_amd/csrc/topolow_gs.hip -- the one-workgroup exact Gauss-Seidel entries of libtopolow_relax.so (relax_gs.h):
// the batch of independent embeddings and what sizes it.  The only source that instantiates gs_embed_kernel: the
// one-workgroup branch of topolow_optimize_layout_exact (topolow_drivers.hip) comes here through gs_relax_by_precision.

#include "topolow_drivers.h"
#include "relax_gs.h"

// gs_relax in the precision asked for (F32: float; anything else, AUTO included: double).  Throws HipError.
void gs_relax_by_precision(int32_t precision, const topolow_problem* problems, topolow_result* results, int32_t count,
                           double* device_seconds, int32_t (*interrupt_cb)(void*), void* interrupt_user,
                           std::vector<double>* trace_out) {
  if (precision == TOPOLOW_PRECISION_F32)
    gs_relax<float>(problems, results, count, device_seconds, interrupt_cb, interrupt_user, trace_out);
  else
    gs_relax<double>(problems, results, count, device_seconds, interrupt_cb, interrupt_user, trace_out);
}

extern "C" {

int64_t topolow_gs_pair_order(int32_t n, uint64_t seed, int32_t iter, int32_t* pairs_out) {
  return gs_pair_order(n, seed, iter, pairs_out);
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
    gs_relax_by_precision(precision, problems, results, count, device_seconds, nullptr, nullptr, nullptr);
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

}  // extern "C"
