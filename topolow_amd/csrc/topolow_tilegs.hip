// topolow_amd/csrc/topolow_tilegs.hip -- the exact tile Gauss-Seidel schedule of a session (relax_tilegs.h): the
// launches of one iteration and of the non-finite inspection, which the session's loop (topolow_relax.hip) calls
// through topolow_session.h, and topolow_tilegs_pair_order of include/topolow_relax.h.

#include "topolow_session.h"
#include "relax_tilegs.h"

namespace {

// ---- exact tile Gauss-Seidel iteration (relax_tilegs.h): in place on `pos` -------------------
template <int DIM>
void launch_tilegs_iteration(topolow_session* s, void* pos, int iter, double k) {
  if constexpr (DIM > kMaxTunedDim) {
    throw HipError{TOPOLOW_ERR_UNSUPPORTED, "schedule gs: ndim must be between 1 and 16 (wider embeddings run the slab schedule)"};
  } else {
  const int nb = (s->n + kTile - 1) / kTile;
  if ((int)s->bperm.n < nb) s->bperm.alloc(nb);
  hipLaunchKernelGGL(tilegs_perm_kernel, dim3(1), dim3(256), 0, s->stream, s->seed, iter, nb, s->bperm.p,
                     s->state.p);
  const int M = nb + (nb & 1), m1 = M - 1;
  const float* no_delta = nullptr;
  for (int r = 0; r < m1 && nb >= 2; ++r) {
    if (s->exact)
      hipLaunchKernelGGL((tilegs_pair_kernel<DIM, double, true>), dim3(M / 2), dim3(kTile), 0, s->stream, s->enc.p,
                         s->denc.p, s->ld, s->n, (double*)pos, s->gplus.p, s->bperm.p, nb, r, s->state.p, s->seed, iter, k,
                         s->c_rep);
    else if (s->precision == TOPOLOW_PRECISION_F64)
      hipLaunchKernelGGL((tilegs_pair_kernel<DIM, double>), dim3(M / 2), dim3(kTile), 0, s->stream, s->enc.p,
                         no_delta, s->ld, s->n, (double*)pos, s->gplus.p, s->bperm.p, nb, r, s->state.p, s->seed, iter, k,
                         s->c_rep);
    else
      hipLaunchKernelGGL((tilegs_pair_kernel<DIM, float>), dim3(M / 2), dim3(kTile), 0, s->stream, s->enc.p,
                         no_delta, s->ld, s->n, (float*)pos, s->gplus.p, s->bperm.p, nb, r, s->state.p, s->seed, iter, k,
                         s->c_rep);
    s->stage_launches += 1;
  }
  if (s->exact)
    hipLaunchKernelGGL((tilegs_intra_kernel<DIM, double, true>), dim3(nb), dim3(kTile), 0, s->stream, s->enc.p, s->denc.p,
                       s->ld, s->n, (double*)pos, s->gplus.p, s->state.p, s->seed, iter, k, s->c_rep);
  else if (s->precision == TOPOLOW_PRECISION_F64)
    hipLaunchKernelGGL((tilegs_intra_kernel<DIM, double>), dim3(nb), dim3(kTile), 0, s->stream, s->enc.p, no_delta, s->ld,
                       s->n, (double*)pos, s->gplus.p, s->state.p, s->seed, iter, k, s->c_rep);
  else
    hipLaunchKernelGGL((tilegs_intra_kernel<DIM, float>), dim3(nb), dim3(kTile), 0, s->stream, s->enc.p, no_delta, s->ld,
                       s->n, (float*)pos, s->gplus.p, s->state.p, s->seed, iter, k, s->c_rep);
  s->stage_launches += 1;
  HIP_TRY(hipGetLastError());
  }
}

}  // namespace

// ---- what the session's loop calls (declared in topolow_session.h) ----

void tilegs_run_iteration(topolow_session* s, void* pos, int iter, double k) {
  TL_DISPATCH_DIM(s->dim, launch_tilegs_iteration, s, pos, iter, k);
}

void launch_tilegs_finite(topolow_session* s, const void* pos, int iter1) {
  const long long nv = (long long)s->n * s->dim;
  if (s->precision == TOPOLOW_PRECISION_F64)
    hipLaunchKernelGGL((tilegs_finite_kernel<double>), dim3(64), dim3(256), 0, s->stream, (const double*)pos, nv,
                       s->state.p, iter1);
  else
    hipLaunchKernelGGL((tilegs_finite_kernel<float>), dim3(64), dim3(256), 0, s->stream, (const float*)pos, nv,
                       s->state.p, iter1);
  HIP_TRY(hipGetLastError());
}

extern "C" {

int64_t topolow_tilegs_pair_order(int32_t n, uint64_t seed, int32_t iter, int32_t* pairs_out) {
  return tilegs_pair_order(n, seed, iter, pairs_out);
}

}  // extern "C"
