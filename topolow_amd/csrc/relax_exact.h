// topolow_amd/csrc/relax_exact.h -- the row-owner stage kernel of precision f64_exact.
//
// slab_stage_pipe_kernel<DIM, double, ...> (relax_kernels.h) takes its forces from the 4-byte target words: fp32 rounded
// to 4 ulp, up to 3e-7 relative off the caller's f64 targets.  A session of precision f64_exact keeps, beside the words,
// what the rounding took away -- one fp32 delta per cell, same layout (relax_common.h: encode_delta) -- and this kernel
// reads both: target = word + delta, the caller's target to 2e-14 relative, for the force and for the r < t / r > t
// comparisons of the ">" and "<" codes alike.  Everything else is the pipe kernel's: the same pipeline (points one chunk
// ahead by direct-to-LDS transfers, words one 256-column group ahead), the same lane-to-column map, the same sums in the
// same order.  The delta words of a group are requested together with its target words, through a second buffer
// resource per row, into registers of their own: twice the loads per chunk, which is what the wait before the chunk
// barrier counts (pipe_await_points<GPC * RPW * 2>; tests/test_exact_f64_isa.py checks the ISA of every instance).
//
// Double only, the twelve tuned coordinate counts, with and without threshold targets: 24 instances, one wave per SIMD
// as the f64 pipe kernel's (StageCfg<256, 2, 0, 1>), no scratch.  No ERR form (f64 sessions fuse checks into the
// symmetric sweep only) and no peer pushes (an f64_exact session is never a row block of several).
#pragma once

#include "relax_kernels.h"

namespace topolow {

// pair_accum<DIM, double, THR> with the target word + delta
template <int DIM, bool THR>
__device__ __forceinline__ void pair_accum_exact(const double (&pc)[DIM], const double (&pi)[DIM], uint32_t w,
                                                 uint32_t dl_bits, double ks, double cg, double (&acc)[DIM]) {
  double dx[DIM];
  double s = 0;
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    dx[d] = pc[d] - pi[d];
    s = fma(dx[d], dx[d], s);
  }
  const double r = Math<double>::sqrt(s);
  const double inv = Math<double>::rcp(r + 0.01);
  // (an unmeasured cell: word +Inf or, unmasked, NaN, delta 0 -- only ever on the unselected side of the select below)
  const double t = (double)bits_f32(THR ? (w & ~kCodeMask) : w) + (double)bits_f32(dl_bits);
  bool spring;
  if constexpr (THR) {
    const uint32_t code = w & kCodeMask;
    spring = (code == 0u) | ((code == 1u) & (r < t)) | ((code == 2u) & (r > t));
  } else {
    spring = __builtin_amdgcn_classf(bits_f32(w), 0x1f8);   // finite of either sign
  }
  const double fs = (t - r) * inv * ks;
  const double fr = inv * inv * inv * cg;
  const double coef = spring ? fs : fr;
#pragma unroll
  for (int d = 0; d < DIM; ++d) acc[d] = fma(dx[d], coef, acc[d]);
}

// pipe_chunk with the delta words: w / dw hold this chunk's groups on entry, the next chunk's on exit.
template <int DIM, typename CFG, bool ANYTHR>
__device__ __forceinline__ void pipe_chunk_exact(PipeRows<DIM, double, CFG::RPW, ANYTHR>& R, const row_rsrc_t (&drsrc)[CFG::RPW],
                                                 const double* __restrict__ pos, int pos_bytes, const unsigned char* cur,
                                                 unsigned char* oth, int cw, int ncb, int ncw,
                                                 uint4 (&w)[PipeGeom<DIM, double, CFG::CHUNK>::GPC][CFG::RPW],
                                                 uint4 (&dw)[PipeGeom<DIM, double, CFG::CHUNK>::GPC][CFG::RPW], int wave,
                                                 int lane) {
  using G = PipeGeom<DIM, double, CFG::CHUNK>;
  constexpr int RPW = CFG::RPW;
  if (ncw > 0) pipe_request_points<DIM, double, CFG::WAVES, CFG::CHUNK>(pos, pos_bytes, ncb, ncw, oth, wave, lane);
  const double* lds_pos = reinterpret_cast<const double*>(cur);
#pragma unroll
  for (int g = 0; g < G::GPC; ++g) {
    const int c4 = lane * 4 + g * 256;
    if (c4 < cw) {
      double pc[4][DIM];
      load_points<DIM, double>(lds_pos, c4, pc);
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        if (ANYTHR && R.thr) {
          pair_accum_exact<DIM, true>(pc[0], R.pi[r], w[g][r].x, dw[g][r].x, R.ks[r], R.cg[r], R.acc[r]);
          pair_accum_exact<DIM, true>(pc[1], R.pi[r], w[g][r].y, dw[g][r].y, R.ks[r], R.cg[r], R.acc[r]);
          pair_accum_exact<DIM, true>(pc[2], R.pi[r], w[g][r].z, dw[g][r].z, R.ks[r], R.cg[r], R.acc[r]);
          pair_accum_exact<DIM, true>(pc[3], R.pi[r], w[g][r].w, dw[g][r].w, R.ks[r], R.cg[r], R.acc[r]);
        } else {
          pair_accum_exact<DIM, false>(pc[0], R.pi[r], w[g][r].x, dw[g][r].x, R.ks[r], R.cg[r], R.acc[r]);
          pair_accum_exact<DIM, false>(pc[1], R.pi[r], w[g][r].y, dw[g][r].y, R.ks[r], R.cg[r], R.acc[r]);
          pair_accum_exact<DIM, false>(pc[2], R.pi[r], w[g][r].z, dw[g][r].z, R.ks[r], R.cg[r], R.acc[r]);
          pair_accum_exact<DIM, false>(pc[3], R.pi[r], w[g][r].w, dw[g][r].w, R.ks[r], R.cg[r], R.acc[r]);
        }
      }
    }
    // the same group of the next chunk, words and deltas: unconditional (2 * RPW loads per group is what the wait below
    // counts); past the slab's end the offset is out of range, which a buffer load answers with 0 without touching memory
    const int noff = g * 256 < ncw ? enc_col_offset_bytes(ncb + c4) : 0x7ffffff0;
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      w[g][r] = load_words(R.rsrc[r], noff);
      dw[g][r] = load_words(drsrc[r], noff);
    }
  }
  pipe_await_points<G::GPC * RPW * 2>();
  __syncthreads();   // next chunk's points have landed; every wave is done reading `cur`
}

// One slab stage for rows [row_begin, row_end) of an f64_exact session.  Arguments as slab_stage_pipe_kernel's;
// ddelta: the delta block, (row_end - row_begin) x ld floats in the layout of denc.
template <int DIM, typename CFG, bool ANYTHR>
__global__ __launch_bounds__(CFG::THREADS, CFG::MINWAVES) void slab_stage_exact_kernel(
    const uint32_t* __restrict__ denc, const float* __restrict__ ddelta, int ld, int row_begin, int row_end, int n,
    const double* __restrict__ pos_in, double* __restrict__ pos_out, const float* __restrict__ gplus,
    const unsigned char* __restrict__ rowflags, RunState* st, SlabRanges rg, int iter1, double k, double c_rep,
    int falling_priority) {
  if (st != nullptr && st->stopped) return;
  using G = PipeGeom<DIM, double, CFG::CHUNK>;
  constexpr int RPW = CFG::RPW;
  __shared__ __attribute__((aligned(16))) unsigned char bufs[2 * G::kBufBytes];   // double buffer

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = row_begin + blockIdx.x * CFG::ROWS + wave * RPW;
  const int pos_bytes = ((n + 3) & ~3) * DIM * (int)sizeof(double);
  const int nc0 = (rg.e0 - rg.b0 + G::CHUNK - 1) / G::CHUNK;
  const int nch = nc0 + (rg.e1 - rg.b1 + G::CHUNK - 1) / G::CHUNK;

  PipeRows<DIM, double, RPW, ANYTHR> R;
  row_rsrc_t drsrc[RPW];
  int rr[RPW];
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int row = row0 + r;
    rr[r] = row < row_end ? row : row_end - 1;  // clamp: result discarded below
    R.rsrc[r] = make_row_rsrc(denc, rr[r] - row_begin, ld);
    drsrc[r] = make_row_rsrc(reinterpret_cast<const uint32_t*>(ddelta), rr[r] - row_begin, ld);
  }
  // first chunk's points, target words and deltas are on their way before anything else
  int cb, cw;
  pipe_chunk_at<G::CHUNK>(rg, nc0, 0, cb, cw);
  pipe_request_points<DIM, double, CFG::WAVES, CFG::CHUNK>(pos_in, pos_bytes, cb, cw, bufs, wave, lane);
  uint4 w[G::GPC][RPW], dw[G::GPC][RPW];
#pragma unroll
  for (int g = 0; g < G::GPC; ++g) {
    const int off = g * 256 < cw ? enc_col_offset_bytes(cb + g * 256 + lane * 4) : 0x7ffffff0;
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      w[g][r] = load_words(R.rsrc[r], off);
      dw[g][r] = load_words(drsrc[r], off);
    }
  }

  int thr_any = 0;  // wave-uniform: do any of this wave's rows hold threshold targets?
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    thr_any |= rowflags[rr[r] - row_begin];
    double p[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) p[d] = uniform(pos_in[(size_t)rr[r] * DIM + d]);  // scalar registers
    const double g = (double)gplus[rr[r]];
    R.set_row(r, p, uniform((2.0 * k) / (4.0 * g + k)), uniform((0.5 * c_rep) / g));
  }
  R.thr = ANYTHR && __builtin_amdgcn_readfirstlane(thr_any) != 0;
  pipe_await_points<0>();
  __syncthreads();

#pragma unroll 1
  for (int c = 0; c < nch; ++c) {
    int ncb, ncw;
    pipe_chunk_at<G::CHUNK>(rg, nc0, c + 1, ncb, ncw);
    if (c + 1 >= nch) ncw = 0;
    unsigned char* cur = bufs + (c & 1) * G::kBufBytes;
    unsigned char* oth = bufs + ((c & 1) ^ 1) * G::kBufBytes;
    if (CFG::PRIO == 1 && falling_priority) {   // see slab_stage_pipe_kernel
      const int left = nch - c;
      if (left >= 4) __builtin_amdgcn_s_setprio(3);
      else if (left == 3) __builtin_amdgcn_s_setprio(2);
      else if (left == 2) __builtin_amdgcn_s_setprio(1);
      else __builtin_amdgcn_s_setprio(0);
    }
    pipe_chunk_exact<DIM, CFG, ANYTHR>(R, drsrc, pos_in, pos_bytes, cur, oth, cw, ncb, ncw, w, dw, wave, lane);
    cw = ncw;
  }

#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int row = row0 + r;
    bool finite = true;
    double out[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      out[d] = R.origin(r, d) - wave_sum<double>(R.lane_sum(r, d));
      finite = finite && isfinite(out[d]);
    }
    if (lane == 0 && row < row_end) {
#pragma unroll
      for (int d = 0; d < DIM; ++d) pos_out[(size_t)row * DIM + d] = out[d];
      if (!finite && st != nullptr) atomicMin(&st->first_nonfinite, iter1);
    }
  }
}

}  // namespace topolow
