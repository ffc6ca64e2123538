// topolow_amd/csrc/relax_symm64.h -- the symmetric sweep in f64 (the reference's arithmetic type)
//
// The same sweep as relax_symm.h -- one-stage iterations, every unordered pair met once from the tile-major copy of the
// upper triangle, both ends moved, the same plan (units / runs), the same tiles and word order, the same partial
// buffers and the same fixed-order sum in the apply kernel -- with positions, records, sums and the pair update in
// f64 (reference src/optimization.cpp:203-281 in double; sqrt and reciprocal to 1 ulp, see sym64_pair).  Against the
// row-owner f64 stage kernel it halves the pair evaluations; an f64 pair costs ~60 full-rate f64 instructions, so the
// sweep is VALU-bound and what matters is the count of pairs, not bytes.
//
// Differences from the fp32 kernel, all consequences of the type: a lane keeps its eight rows (coordinates, two
// constants: 14 doubles per row at ndim 5) in LDS and only their sums in registers -- 80 of the 254 the ndim-5
// instance uses, two waves per SIMD (ndim 6: one); nothing is packed; the column sums of a half tile are reduced over the 8 lanes of a
// column group with three lane exchanges per value (the fp32 kernel's one-instruction DPP adds have no f64 form).
//
// The fused convergence check (ERR instance) is EXACT.  The tiles hold the targets as 4-byte words (fp32 rounded to
// 4 ulp, 3e-7 relative): reduced from them the MAE would sit 3e-8 off the reference's edge MAE (measured), where the
// separate pass of f64 sessions over the f64 edge list is exact.  So the ERR instance also reads, tile-major like the
// words, what the rounding took away: delta = (exact f64 target) - (decoded word), stored as fp32 (symm64_delta_kernel,
// from the session's f64 edge list; 6e-8 of 3e-7 of the target: 2e-14 relative), and sums |t_word + delta - r| = the
// exact |t - r|.  That is precision = "f64": its forces still come from the words, as in its stage kernel and tile GS.
//
// precision = "f64_exact" runs symm64x_sweep_kernel (below): the same body with the delta words in EVERY instance, made
// from the session's delta block (the matrix, not the edge list), and target = word + delta for the force, the
// threshold comparisons and the check alike -- the caller's f64 targets to 2e-14 relative throughout.
#pragma once

#include "relax_device.h"
#include "relax_symm.h"

namespace topolow {

// One point as the sweep reads it: DIM coordinates, then ks = 2k / (4 g + k) and cg = (c_rep / 2) / g, padded to 16 bytes.
template <int DIM> struct SymRec64 { static constexpr int W = (DIM + 2 + 1) & ~1; };

__device__ __forceinline__ double sym64_xor(double v, int mask) { return __shfl_xor(v, mask, 64); }

// The apply and records kernels in f64 (relax_symm.h: symm_apply_kernel<DIM, double>, symm_records_kernel<DIM, double>).
template <int DIM> struct SymReal<DIM, double> {
  static constexpr int W = SymRec64<DIM>::W;
  __device__ static double ks(double k, double g) { return 2.0 * k / (4.0 * g + k); }
  __device__ static double cg(double c_rep, double g) { return 0.5 * c_rep / g; }
  __device__ static double far(int d) { return d == 0 ? kFarF64 : 0.0; }
  __device__ static double lane_xor(double v, int mask) { return sym64_xor(v, mask); }
};

// one row x one column: both halves of the pair.  base = (t - r) / (r + 0.01) for a spring, 1 / (r + 0.01)^3 otherwise;
// every endpoint multiplies it with its own constant of that kind.  EXACT (f64_exact sessions): the target is the word
// plus its delta -- for the force, for the comparisons of the ">" and "<" codes and for the check alike.
template <int DIM, bool THR, bool ERR, bool EXACT = false>
__device__ __forceinline__ void sym64_pair(const double (&pc)[DIM], double ksc, double cgc, const double (&pi)[DIM],
                                           double ksr, double cgr, uint32_t w, double (&racc)[DIM], double (&cacc)[DIM],
                                           uint32_t dl_bits, double& err, unsigned& cnt) {
  double dx[DIM];
  double s = 0.0;
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    dx[d] = pc[d] - pi[d];
    s = fma(dx[d], dx[d], s);
  }
  const double r = Math<double>::sqrt(s);             // 1 ulp (relax_device.h): estimate + two Newton steps
  const double inv = Math<double>::rcp(r + 0.01);
  double t = (double)bits_f32(THR ? (w & ~kCodeMask) : w);
  if constexpr (EXACT) {
    t += (double)bits_f32(dl_bits);
    // pinned: where only the spring's side of the select below reads t (no thresholds, no check) the optimiser sank the
    // conversions and the add behind a branch on `spring` -- the tile fell into basic blocks (scratch at ndim 4)
    asm volatile("" : "+v"(t));
  }
  bool spring;
  if constexpr (THR) {
    // 0: exact target; 1: ">" -- a spring while r < t; 2: "<" -- while r > t: the sign of t - r, turned round for code 2,
    // and two comparisons per pair (one per code and relation keeps six lane masks per pair alive)
    const uint32_t code = w & kCodeMask;
    const double e = t - r;
    const double es = __hiloint2double(__double2hiint(e) ^ (int)((w << 30) & 0x80000000u), __double2loint(e));
    spring = (code == 0u) | (es > 0.0);
  } else {
    spring = __builtin_amdgcn_classf(bits_f32(w), 0x1f8);   // measured = finite
  }
  const double base = spring ? (t - r) * inv : inv * inv * inv;
  const double coef = base * (spring ? ksr : cgr);
  const double cc = base * (spring ? ksc : cgc);
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    racc[d] = fma(dx[d], coef, racc[d]);
    cacc[d] = fma(dx[d], cc, cacc[d]);
  }
  if constexpr (ERR) {   // the convergence MAE of the positions this sweep reads, against the EXACT target t + delta
    if constexpr (EXACT) err += spring ? fabs(t - r) : 0.0;
    else err += spring ? fabs((t - r) + (double)bits_f32(dl_bits)) : 0.0;
    if constexpr (THR) cnt += spring ? 1u : 0u;
  }
}

// delta tiles: for every edge of the session's f64 edge list (session labels; codes 0, 1, -1) the difference between the
// exact target and what its 4-byte word decodes to, at the cell(s) of the tile-major copy the sweep meets the pair at
// (a pair inside a diagonal square is met from both sides).  tdelta: zero-filled by the caller.
__global__ __launch_bounds__(256) void symm64_delta_kernel(const int* __restrict__ ei, const int* __restrict__ ej,
                                                          const double* __restrict__ et, const int8_t* __restrict__ ec,
                                                          long long n_edges, float* __restrict__ tdelta, int TC, int n) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += (long long)gridDim.x * blockDim.x) {
    const int a = ei[e], b = ej[e], c = ec[e];
    if (a < 0 || b < 0 || a >= n || b >= n || a == b || c == 2) continue;
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    const double t = et[e];
    const uint32_t w = encode_target(t, c);
    if (w == kInfWord) continue;
    const float dl = (float)(t - (double)bits_f32(w & ~kCodeMask));
    const int R = lo / kSymRows;
    tdelta[(size_t)sym_tile_index(R, hi / kSymCols, TC) * kSymTileWords + sym_word_in_tile(lo % kSymRows, hi % kSymCols)] = dl;
    if (hi / kSymRows == R)
      tdelta[(size_t)sym_tile_index(R, lo / kSymCols, TC) * kSymTileWords + sym_word_in_tile(hi % kSymRows, lo % kSymCols)] = dl;
  }
}

// enc, units, runs, col_row0: as symm_sweep_kernel.  rec: npad records of SymRec64<DIM>::W doubles.
// rowpart [n_units][64][DIM], colpart [n_tile_rows][npad][DIM] in f64.  ERR: tdelta (tile-major like enc, see above);
// part_sum / part_cnt / fixed_cnt as symm_sweep_kernel leaves them (TWICE the sum and the count over the unit's
// contributing pairs; a pair of the diagonal square is met from both sides and counts once per visit).
template <int DIM, bool ANYTHR, bool ERR>
__global__ __launch_bounds__(64 * kSymWaves, ((DIM <= 3 || (DIM == 4 && !(ANYTHR && ERR)) || (DIM == 5 && !ERR)) ? 2 : 1)) void symm64_sweep_kernel(
    const uint32_t* __restrict__ enc, const double* __restrict__ rec, const SymUnit* __restrict__ units,
    const SymRun* __restrict__ runs, double* __restrict__ rowpart, double* __restrict__ colpart, int npad,
    const RunState* st, int col_row0, const float* __restrict__ tdelta, double* __restrict__ part_sum,
    unsigned long long* __restrict__ part_cnt, unsigned long long fixed_cnt) {
#define SYM64_BODY_EXACT false
#include "relax_symm64_body.h"
#undef SYM64_BODY_EXACT
}

// The sweep of an f64_exact session: every target is word + delta (tdelta: the tile-major copy of the session's delta
// block, made by symm_tiles_kernel like the words' copy), so the forces see the caller's f64 targets to 2e-14 relative
// and the ERR form's |t - r| needs no separate delta term.  Every instance carries the 32 registers of delta words that
// only the ERR instances of symm64_sweep_kernel carry.  Waves per SIMD (kSym64xWaves; tests/test_exact_f64_isa.py):
// two up to ndim 4 (182 .. 253 registers), one at ndim 5 and 6 (256 and accumulator registers); no scratch in any
// instance; 13 .. 18 branches each, as symm64_sweep_kernel: the tile is one basic block.
template <int DIM> constexpr int kSym64xWaves = DIM <= 4 ? 2 : 1;

template <int DIM, bool ANYTHR, bool ERR>
__global__ __launch_bounds__(64 * kSymWaves, kSym64xWaves<DIM>) void symm64x_sweep_kernel(
    const uint32_t* __restrict__ enc, const double* __restrict__ rec, const SymUnit* __restrict__ units,
    const SymRun* __restrict__ runs, double* __restrict__ rowpart, double* __restrict__ colpart, int npad,
    const RunState* st, int col_row0, const float* __restrict__ tdelta, double* __restrict__ part_sum,
    unsigned long long* __restrict__ part_cnt, unsigned long long fixed_cnt) {
#define SYM64_BODY_EXACT true
#include "relax_symm64_body.h"
#undef SYM64_BODY_EXACT
}

}  // namespace topolow
