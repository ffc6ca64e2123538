// topolow_amd/csrc/relax_symm_wide.h -- the symmetric sweep for ndim 7..10 (fp32)
//
// The same sweep as relax_symm.h -- one-stage iterations (and the stages of pair-split ones), every unordered pair met
// once from the tile-major copy of the upper triangle, both ends moved; the same 64 x 32 tiles and word order, the same
// records (SymRec<DIM>: W = 12 floats for all four dims, 96 16-byte pieces per column block: two per lane), the same
// plans (SymUnit / SymRun), the same rowpart / colpart / part_sum / part_cnt and col_row0 -- so the records, tiles,
// apply, partial and owner-apply kernels and the hold-out patches of relax_symm.h / relax_cv.h serve it unchanged.
//
// What differs is where a lane keeps its eight rows.  symm_sweep_kernel holds their coordinates, constants and sums
// in VGPRs (20 x ndim + 16 of them): from ndim 7 that no longer fits two waves per SIMD, nor one without scratch
// (cross-compiled: 968 B of scratch at ndim 7, 1 952 B at ndim 10 with thresholds and ERR).  Here, as in the f64 sweep
// (relax_symm64.h), the tile-row's 64 row records live in LDS and only their sums (8 x ndim) in VGPRs; a row pair's
// coordinates and constants are read just ahead of the column they meet.  The rows are stored PACKED: the two rows of a
// row pair interleaved word by word, so that one 16-byte LDS read delivers two (row 0, row 1) operands of v_pk_*_f32 in
// aligned register pairs.  A lane group a (8 rows = 4 row pairs x 24 floats) takes 24 16-byte slots and one of skew:
// the eight groups of a 16-byte read then fall on eight different 16-byte bank groups (25 a mod 16 is a permutation of
// the even/odd slots), and the 8 lanes b that share a group read one address (a broadcast).  LDS per wave: 3.2 KB of
// rows + 2 x 2.2 KB of column blocks.
//
// Kept from symm_sweep_kernel: the packed pair update with one selection of the shared factor (sym_pair), the
// one-instruction DPP column reduction with its hazard spacing (sym_col_reduce), branch-free column stores through the
// bounds-checked buffer, requests a half tile ahead, the issue priority by work left, the batch of scalar loads at the
// head of the wave.  The tile is one basic block: the hand-over of the next column block's records is unconditional
// (128 slots per block whatever the 96 in use: a divergent store would split the tile, see relax_symm64.h).
//
// Waves per SIMD: two for all sixteen instances (ndim 7..10 x {threshold-free, threshold} x {plain, ERR}), without
// scratch: 173 VGPRs at ndim 7 up to 240 at ndim 10 with thresholds and ERR, of the 256 that two waves leave each
// (tests/test_symm_wide_isa.py).  At ndim 10 the row sums are 80 of them, the prefetched words and records 40, a
// column's packed sums, a row pair and the column itself 56.
//
// Which sessions run it is the host's decision (topolow_symm.hip: sym_shape_ok, sym_dim_default): a dimension is on
// by default where the sweep measured faster than the row-owner kernel -- all four: at N = 10 000 an iteration takes
// 69 .. 82 us (87 with thresholds) against 96 .. 116 (145) us (profiles/r05_symm_wide.txt).  Also measured there and
// not kept: reading a column's record one column and a row pair one pair ahead of their use (+29 VGPRs, spills from
// ndim 9): 68.2 / 72.3 us at ndim 7 / 8 against 68.8 / 71.3 -- inside the spread; the other wave of the SIMD covers
// the LDS latency.
#pragma once

#include "relax_symm.h"

namespace topolow {

constexpr int kSymWideMinDim = 7, kSymWideMaxDim = 10;

// enc, rec, units, runs, rowpart, colpart, part_sum, part_cnt, fixed_cnt, col_row0, prio: as symm_sweep_kernel.
template <int DIM, bool ANYTHR, bool ERR>
__global__ __launch_bounds__(64 * kSymWaves, 2) void symm_sweep_wide_kernel(
    const uint32_t* __restrict__ enc, const float* __restrict__ rec, const SymUnit* __restrict__ units,
    const SymRun* __restrict__ runs, float* __restrict__ rowpart, float* __restrict__ colpart, int npad,
    const RunState* st, double* __restrict__ part_sum, unsigned long long* __restrict__ part_cnt,
    unsigned long long fixed_cnt, int col_row0, int prio) {
  static_assert(DIM >= kSymWideMinDim && DIM <= kSymWideMaxDim, "ndim 2..6: symm_sweep_kernel");
  // the head of the wave as in symm_sweep_kernel: the run is requested together with the stop flag, and everything up
  // to the first vector load is pinned in scalar registers in front of the branch
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gw = blockIdx.x * kSymWaves + wave;
  const SymRun run = runs[gw];
  int stopped = st->stopped;   // (st is never null here: the probe passes a cleared RunState)
  if constexpr (ERR)
    asm("" : "+s"(stopped) : "s"(run.u0), "s"(run.u1), "s"(run.first.tile_row), "s"(run.first.j0), "s"(run.first.j1),
        "s"(run.first.tile0), "s"(run.tiles), "s"(enc), "s"(rec), "s"(units),
        "s"(rowpart), "s"(colpart), "s"(npad), "s"(col_row0), "s"(prio), "s"(part_sum), "s"(part_cnt), "s"(fixed_cnt));
  else
    asm("" : "+s"(stopped) : "s"(run.u0), "s"(run.u1), "s"(run.first.tile_row), "s"(run.first.j0), "s"(run.first.j1),
        "s"(run.first.tile0), "s"(run.tiles), "s"(enc), "s"(rec), "s"(units),
        "s"(rowpart), "s"(colpart), "s"(npad), "s"(col_row0), "s"(prio));
  if (stopped) return;
  constexpr int W = SymRec<DIM>::W;
  static_assert(W == 12, "ndim 7..10: records of 12 floats");
  constexpr int kRecVec = W / 4;                   // 16-byte pieces per record: 3
  constexpr int kTileVec = kSymCols * kRecVec;     // ... per column block: 96, two per lane (the second of lanes >= 32 unused)
  // a column block's 32 records in LDS, one 16-byte piece of skew after every 4 records (symm_sweep_kernel); 128 pieces
  // are written per block, so that the hand-over needs no lane condition
  constexpr int kLdsVec = 128 + 128 / (4 * kRecVec) + 1;
  constexpr int kRowVec = 2 * kRecVec;             // 16-byte pieces per packed row pair: 6
  constexpr int kRowGroup = 4 * kRowVec + 1;       // ... per lane group a, with one piece of skew: 25
  __shared__ uint4 lds[kSymWaves][2][kLdsVec];
  // (words, written and read as words: a store of floats into an array that is read as 16-byte vectors is not one the
  //  optimiser has to honour -- it kept one word of each piece; the four word reads of a piece still merge into one
  //  ds_read_b128, the array and every piece being 16-byte aligned)
  __shared__ __attribute__((aligned(16))) uint32_t rows_lds[kSymWaves][8 * kRowGroup * 4];
  auto lds_slot = [](int q) { return q + (q / (4 * kRecVec)); };   // q = record * kRecVec + piece
  const int lane = threadIdx.x & 63;
  const int a = lane & 7, b = lane >> 3;

  const int u_begin = __builtin_amdgcn_readfirstlane(run.u0);
  const int u_end = __builtin_amdgcn_readfirstlane(run.u1);
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  const __amdgpu_buffer_rsrc_t rec_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(rec), 0, npad * W * 4, 0x00020000);
  // tiles of the run still to do, and the counts above which the priority is 3, 2, 1 (more than 3/4, 1/2, 1/4 of the run)
  int left = __builtin_amdgcn_readfirstlane(run.tiles);
  const int lv3 = (3 * left) >> 2, lv2 = left >> 1, lv1 = left >> 2;
  SymUnit U_next = run.first;
  for (int u = u_begin; u < u_end; ++u) {
    const SymUnit U = U_next;
    U_next = units[u + 1 < u_end ? u + 1 : u];
    const int R = __builtin_amdgcn_readfirstlane(U.tile_row);
    const int J0 = __builtin_amdgcn_readfirstlane(U.j0), J1 = __builtin_amdgcn_readfirstlane(U.j1);
    __builtin_assume(J0 < J1);
    const int slot = u;
    const int tile0 = __builtin_amdgcn_readfirstlane(U.tile0);

    // the tile-row's 64 row records into LDS, packed by row pair: word k of row r = 8 a' + 2 p + e sits at float
    // 4 (25 a' + 6 p) + 2 k + e.  Three 16-byte pieces per lane, read coalesced (64 R + 63 < npad: inside the records);
    // the previous unit's reads of these slots are complete (a wave's LDS operations complete in order)
    symf2 racc2[4][DIM];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int d = 0; d < DIM; ++d) racc2[p][d] = (symf2){0.0f, 0.0f};
    {
      uint32_t* rows_w = &rows_lds[wave][0];
#pragma unroll
      for (int j = 0; j < kRecVec; ++j) {
        const int q = lane + 64 * j;               // piece q of the tile-row: row q / 3, words 4 (q % 3) ..
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rec_rsrc, (R * kSymRows * kRecVec + q) * 16, 0, 0);
        const int r = q / kRecVec, k0 = 4 * (q % kRecVec);
        uint32_t* dst = rows_w + 4 * (kRowGroup * (r >> 3) + kRowVec * ((r & 7) >> 1)) + 2 * k0 + (r & 1);
        dst[0] = v.x;
        dst[2] = v.y;
        dst[4] = v.z;
        dst[6] = v.w;
      }
    }
    // row pair p of this lane: coordinates (row 0's, row 1's) per dimension, then the two constants
    const uint32_t* my_rows = &rows_lds[wave][4 * kRowGroup * a];
    auto read_rows = [&](int p, symf2 (&pi2)[DIM], symf2& ks2, symf2& cg2) {
      symf2 f[2 * ((DIM + 2 + 1) / 2)];
#pragma unroll
      for (int v = 0; v < (DIM + 2 + 1) / 2; ++v) {
        const uint32_t* q = my_rows + 4 * (kRowVec * p + v);
        f[2 * v] = (symf2){__builtin_bit_cast(float, q[0]), __builtin_bit_cast(float, q[1])};
        f[2 * v + 1] = (symf2){__builtin_bit_cast(float, q[2]), __builtin_bit_cast(float, q[3])};
      }
#pragma unroll
      for (int d = 0; d < DIM; ++d) pi2[d] = f[d];
      ks2 = f[DIM];
      cg2 = f[DIM + 1];
    };
    // the unit's tiles as one buffer (wave-uniform descriptor): tile J at (J - J0) * 8 KB; a lane's load (h, p) 1 KB apart
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint32_t*>(enc) + (size_t)tile0 * kSymTileWords, 0, (J1 - J0) * kSymTileWords * 4, 0x00020000);
    // the tile-row's column partials as one buffer; lane a = 0 stores the first column of a half, a = 1 the second,
    // the other lanes get an offset past its end
    const __amdgpu_buffer_rsrc_t col_rsrc = __builtin_amdgcn_make_buffer_rsrc(colpart + (size_t)(R - col_row0) * npad * DIM, 0, npad * DIM * 4, 0x00020000);
    const int col_off = a < 2 ? (4 * b + a) * DIM * 4 : 0x40000000;
    const int swap = a & 1;                // this lane's q-th column of a half is column 2h + (q ^ swap)
    auto request = [&](int J, int h, u32x4 (&dst)[4]) {
#pragma unroll
      for (int p = 0; p < 4; ++p)
        dst[p] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane * 16 + ((J - J0) * 8 + 4 * h + p) * 1024, 0, 0);
    };
    u32x4 wa[4], wb[4];
    request(J0, 0, wa);
    // a column block's records: two pieces per lane through the bounds-checked buffer (lanes >= 32 fetch pieces of the
    // next block, or zeros past the last one, into slots nobody reads)
    auto request_rec = [&](int J, u32x4& r0, u32x4& r1) {
      r0 = __builtin_amdgcn_raw_buffer_load_b128(rec_rsrc, (J * kTileVec + lane) * 16, 0, 0);
      r1 = __builtin_amdgcn_raw_buffer_load_b128(rec_rsrc, (J * kTileVec + lane + 64) * 16, 0, 0);
    };
    auto hand_over = [&](int J, const u32x4& r0, const u32x4& r1) {
      lds[wave][J & 1][lds_slot(lane)] = make_uint4(r0.x, r0.y, r0.z, r0.w);
      lds[wave][J & 1][lds_slot(lane + 64)] = make_uint4(r1.x, r1.y, r1.z, r1.w);
    };
    {
      u32x4 r0, r1;
      request_rec(J0, r0, r1);
      hand_over(J0, r0, r1);
    }

    symf2 err2 = {0.0f, 0.0f};
    float err_unit = 0.0f;
    unsigned cnt_wave = 0, cnt_unit2 = 0;   // err_unit, cnt_unit2: twice the sum / count (the diagonal square counts once per visit)
    auto read_rec = [&](int J, int idx, float (&f)[W]) {   // the lane's idx-th column of the tile, in ITS order
      const int col = idx ^ swap;
      const uint4* cp = &lds[wave][J & 1][4 * b * kRecVec + b];
#pragma unroll
      for (int v = 0; v < kRecVec; ++v) {
        const uint4 q = cp[col * kRecVec + v];
        f[4 * v + 0] = __builtin_bit_cast(float, q.x);
        f[4 * v + 1] = __builtin_bit_cast(float, q.y);
        f[4 * v + 2] = __builtin_bit_cast(float, q.z);
        f[4 * v + 3] = __builtin_bit_cast(float, q.w);
      }
    };
#pragma unroll 1
    for (int J = J0; J < J1; ++J) {
      if (prio) {   // wave-uniform: scalar compares and branches around s_setprio with an immediate
        if (left > lv3) __builtin_amdgcn_s_setprio(3);
        else if (left > lv2) __builtin_amdgcn_s_setprio(2);
        else if (left > lv1) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
      }
      --left;
      const int Jn = J + 1 < J1 ? J + 1 : J;
      // requests first: the second half's words, the next column block's records
      request(J, 1, wb);
      u32x4 rn0, rn1;
      request_rec(Jn, rn0, rn1);
      __builtin_amdgcn_sched_barrier(0);   // the requests stay up here ...

      const bool diag = J < 2 * R + 2;   // (its column sums go to slots nobody reads: no need to switch the column side off)
      auto half = [&](auto hc, const u32x4 (&wc)[4]) {   // columns 2h, 2h + 1 of the lane's four x its eight rows
        constexpr int h = decltype(hc)::value;
        float first[DIM], second[DIM];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          float f[W];
          read_rec(J, 2 * h + c, f);
          float pc[DIM];
#pragma unroll
          for (int d = 0; d < DIM; ++d) pc[d] = f[d];
          const float ksc = f[DIM], cgc = f[DIM + 1];
          symf2 cacc2[DIM];
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            symf2 pi2[DIM], ks2, cg2;
            read_rows(p, pi2, ks2, cg2);
            const uint32_t w0 = c == 0 ? wc[p].x : wc[p].z, w1 = c == 0 ? wc[p].y : wc[p].w;
            if (p == 0)
              sym_pair<DIM, ANYTHR, ERR, ANYTHR, true>(pc, ksc, cgc, pi2, ks2, cg2, w0, w1, racc2[p], cacc2, err2, cnt_wave);
            else
              sym_pair<DIM, ANYTHR, ERR, ANYTHR, false>(pc, ksc, cgc, pi2, ks2, cg2, w0, w1, racc2[p], cacc2, err2, cnt_wave);
            // one row pair in flight: the sums are pinned here, so that instruction selection cannot put every pair's
            // distance first and all the updates last, with each pair's dx alive in between (relax_symm64.h)
#pragma unroll
            for (int d = 0; d < DIM; ++d) asm volatile("" : "+v"(racc2[p][d]), "+v"(cacc2[d]));
            __builtin_amdgcn_sched_barrier(0);
          }
          // the column's sum over the lane's eight rows: the two halves of the packed sums
#pragma unroll
          for (int d = 0; d < DIM; ++d) (c == 0 ? first[d] : second[d]) = cacc2[d].x + cacc2[d].y;
        }
        // column sums over the 8 lanes a = 0..7 of a column group (sym_col_reduce); lanes a = 0 and a = 1 store a column
        // each: a buffer store whose offset lies past the buffer's end for the other lanes -- no branch.  The diagonal
        // square's sums land in slots nobody reads.
        sym_col_reduce<DIM>(first, second);
        const int off0 = col_off + ((J * kSymCols) * DIM + h * 2 * DIM) * 4;
#pragma unroll
        for (int q = 0; q < DIM; q += 4) {
          if (q + 4 <= DIM) {
            const u32x4 pk = {__builtin_bit_cast(uint32_t, first[q]), __builtin_bit_cast(uint32_t, first[q + 1]),
                              __builtin_bit_cast(uint32_t, first[q + 2]), __builtin_bit_cast(uint32_t, first[q + 3])};
            __builtin_amdgcn_raw_buffer_store_b128(pk, col_rsrc, off0 + q * 4, 0, 0);
          } else {
#pragma unroll
            for (int t = q; t < DIM; ++t)
              __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, first[t]), col_rsrc, off0 + t * 4, 0, 0);
          }
        }
      };
      half(std::integral_constant<int, 0>{}, wa);
      request(Jn, 0, wa);                  // the next tile's first half, while this tile's second half is computed
      __builtin_amdgcn_sched_barrier(0);
      half(std::integral_constant<int, 1>{}, wb);
      if constexpr (ERR) {
        const float es = err2.x + err2.y;
        err_unit += diag ? es : 2.0f * es;
        cnt_unit2 += diag ? cnt_wave : 2u * cnt_wave;
        err2 = (symf2){0.0f, 0.0f};
        cnt_wave = 0;
      }
      // hand over: next column block's records into the other LDS half
      __builtin_amdgcn_sched_barrier(0);   // ... and their first use stays down here, a tile's arithmetic later
      hand_over(J + 1, rn0, rn1);
    }
    // row sums over the 8 lanes b = 0..7 of a row group (lane bits 3..5); lane b = 0 stores
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int d = 0; d < DIM; ++d) {
        symf2 v = racc2[p][d];
        v.x += __shfl_xor(v.x, 8, 64);  v.y += __shfl_xor(v.y, 8, 64);
        v.x += __shfl_xor(v.x, 16, 64); v.y += __shfl_xor(v.y, 16, 64);
        v.x += __shfl_xor(v.x, 32, 64); v.y += __shfl_xor(v.y, 32, 64);
        racc2[p][d] = v;
      }
    if (b == 0) {
      float* dst = rowpart + ((size_t)slot * kSymRows + 8 * a) * DIM;
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
          dst[(2 * p) * DIM + d] = racc2[p][d].x;
          dst[(2 * p + 1) * DIM + d] = racc2[p][d].y;
        }
    }
    if constexpr (ERR) {
      double s = (double)err_unit;
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
      if constexpr (ANYTHR) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) cnt_unit2 += __shfl_xor(cnt_unit2, m, 64);
      }
      if (lane == 0) {
        part_sum[slot] = s;
        // threshold-free block: the number of contributing cells is the host's; otherwise the wave's counts
        part_cnt[slot] = ANYTHR ? (unsigned long long)cnt_unit2 : (slot == 0 ? fixed_cnt : 0ull);
      }
    }
  }
}

}  // namespace topolow
