// topolow_amd/csrc/relax_symm64_body.h -- the body of the f64 symmetric sweep's kernels, included into each of them
// (relax_symm64.h: symm64_sweep_kernel with SYM64_BODY_EXACT false, symm64x_sweep_kernel with true).  Text, not a
// function: shared as an inlined __device__ template, one instance of symm64_sweep_kernel came out with two more
// registers (ndim 3, threshold-free, ERR: 220 for 218); included, its twenty instances are what they were before the
// exact kernel existed, instruction for instruction.  In scope: the template parameters DIM, ANYTHR, ERR and the
// kernel's arguments.  No include guard.
  if (st != nullptr && st->stopped) return;
  constexpr bool EXACT = SYM64_BODY_EXACT;
  constexpr bool DELTA = ERR || EXACT;   // the delta words travel with the target words
  constexpr int W = SymRec64<DIM>::W;
  constexpr int kRecVec = W / 2;                   // 16-byte pieces per record
  constexpr int kTileVec = kSymCols * kRecVec;     // ... per column block (<= 128)
  static_assert(kTileVec <= 128, "two pieces per lane");
  // (two 16-byte pieces per lane: 128 slots per block whatever kTileVec is, so that the hand-over at the end of a tile
  //  is unconditional -- a divergent store there splits the tile into basic blocks, see the column stores below)
  __shared__ uint4 lds[kSymWaves][2][128];
  __shared__ uint4 rows_lds[kSymWaves][kSymRows * kRecVec + 8];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int a = lane & 7, b = lane >> 3;
  const int gw = blockIdx.x * kSymWaves + wave;
  const SymRun run = runs[gw];
  const int u_begin = __builtin_amdgcn_readfirstlane(run.u0);
  const int u_end = __builtin_amdgcn_readfirstlane(run.u1);
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  const __amdgpu_buffer_rsrc_t rec_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(rec), 0, npad * W * 8, 0x00020000);
  for (int u = u_begin; u < u_end; ++u) {
    const SymUnit U = u == u_begin ? run.first : units[u];
    const int R = __builtin_amdgcn_readfirstlane(U.tile_row);
    const int J0 = __builtin_amdgcn_readfirstlane(U.j0), J1 = __builtin_amdgcn_readfirstlane(U.j1);
    const int tile0 = __builtin_amdgcn_readfirstlane(U.tile0);

    // the tile-row's 64 row records go to LDS (a lane re-reads the two rows of a row pair whenever it meets them: kept
    // in registers, eight rows' coordinates and constants cost 112 of them and the kernel spilled); only the row sums
    // stay in registers.  Record r sits one 16-byte piece further for every 8 rows, so the 8 lane groups a read 8 banks
    double racc[8][DIM];
    double err_tile = 0.0, err_unit = 0.0;
    unsigned cnt_tile = 0, cnt_unit2 = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
      for (int d = 0; d < DIM; ++d) racc[q][d] = 0.0;
    {
      const uint4* rr = reinterpret_cast<const uint4*>(rec + (size_t)R * kSymRows * W);
#pragma unroll
      for (int q = lane; q < kSymRows * kRecVec; q += 64) rows_lds[wave][q + (q / (8 * kRecVec))] = rr[q];
    }
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint32_t*>(enc) + (size_t)tile0 * kSymTileWords, 0, (J1 - J0) * kSymTileWords * 4, 0x00020000);
    const int swap = a & 1;                // this lane's q-th column of a half is column 2h + (q ^ swap)
    auto request = [&](int J, int h, u32x4 (&dst)[4]) {
#pragma unroll
      for (int p = 0; p < 4; ++p)
        dst[p] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane * 16 + ((J - J0) * 8 + 4 * h + p) * 1024, 0, 0);
    };
    // the delta words: the same addresses in the tile-major delta array
    const __amdgpu_buffer_rsrc_t drsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(DELTA ? tdelta + (size_t)tile0 * kSymTileWords : nullptr), 0, DELTA ? (J1 - J0) * kSymTileWords * 4 : 0, 0x00020000);
    auto request_delta = [&](int J, int h, u32x4 (&dst)[4]) {
      if constexpr (DELTA) {
#pragma unroll
        for (int p = 0; p < 4; ++p)
          dst[p] = __builtin_amdgcn_raw_buffer_load_b128(drsrc, lane * 16 + ((J - J0) * 8 + 4 * h + p) * 1024, 0, 0);
      }
    };
    u32x4 wa[4], wb[4], da[4], db[4];
    request(J0, 0, wa);
    request_delta(J0, 0, da);
    const uint4* recv = reinterpret_cast<const uint4*>(rec);
    if (lane < kTileVec) lds[wave][J0 & 1][lane] = recv[(size_t)J0 * kTileVec + lane];
    if constexpr (kTileVec > 64) if (lane + 64 < kTileVec) lds[wave][J0 & 1][lane + 64] = recv[(size_t)J0 * kTileVec + lane + 64];
    const __amdgpu_buffer_rsrc_t col_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        colpart + (size_t)(R - col_row0) * npad * DIM, 0, npad * DIM * 8, 0x00020000);
    const int col_off = a < 2 ? (4 * b + a) * DIM * 8 : 0x40000000;
#pragma unroll 1
    for (int J = J0; J < J1; ++J) {
      const int Jn = J + 1 < J1 ? J + 1 : J;
      request(J, 1, wb);
      request_delta(J, 1, db);
      u32x4 rn0 = {0, 0, 0, 0}, rn1 = {0, 0, 0, 0};
      rn0 = __builtin_amdgcn_raw_buffer_load_b128(rec_rsrc, (Jn * kTileVec + lane) * 16, 0, 0);
      if constexpr (kTileVec > 64) rn1 = __builtin_amdgcn_raw_buffer_load_b128(rec_rsrc, (Jn * kTileVec + lane + 64) * 16, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      auto half = [&](auto hc, const u32x4 (&wc)[4], const u32x4 (&dc)[4]) {   // columns 2h, 2h + 1 of the lane's four x its eight rows
        constexpr int h = decltype(hc)::value;
        double cacc[2][DIM], pc[2][DIM], ksc[2], cgc[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          // the lane's c-th column of the half (its order: see sym_word_in_tile) from the wave's LDS copy of the block
          const int col = 4 * b + 2 * h + (c ^ swap);
          const double* f = reinterpret_cast<const double*>(&lds[wave][J & 1][col * kRecVec]);
#pragma unroll
          for (int d = 0; d < DIM; ++d) {
            pc[c][d] = f[d];
            cacc[c][d] = 0.0;
          }
          ksc[c] = f[DIM];
          cgc[c] = f[DIM + 1];
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          double pi[2][DIM], ks[2], cg[2];
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const int q = (8 * a + 2 * p + e) * kRecVec;
            const double* f = reinterpret_cast<const double*>(&rows_lds[wave][q + a]);     // (8a + 2p + e) / 8 == a
#pragma unroll
            for (int d = 0; d < DIM; ++d) pi[e][d] = f[d];
            ks[e] = f[DIM];
            cg[e] = f[DIM + 1];
          }
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const uint32_t w0 = c == 0 ? wc[p].x : wc[p].z, w1 = c == 0 ? wc[p].y : wc[p].w;
            const uint32_t d0 = DELTA ? (c == 0 ? dc[p].x : dc[p].z) : 0u, d1 = DELTA ? (c == 0 ? dc[p].y : dc[p].w) : 0u;
            sym64_pair<DIM, ANYTHR, ERR, EXACT>(pc[c], ksc[c], cgc[c], pi[0], ks[0], cg[0], w0, racc[2 * p], cacc[c], d0, err_tile, cnt_tile);
            sym64_pair<DIM, ANYTHR, ERR, EXACT>(pc[c], ksc[c], cgc[c], pi[1], ks[1], cg[1], w1, racc[2 * p + 1], cacc[c], d1, err_tile, cnt_tile);
          }
          // four pairs in flight, no more.  The sums are pinned here (empty statements that "use" them): a scheduling
          // barrier alone does not order pure arithmetic -- instruction selection had put every pair's distance and factor
          // first and all the updates of the sums last, with each pair's dx and factor alive in between (370 registers
          // at ndim 2, scratch from ndim 4)
#pragma unroll
          for (int d = 0; d < DIM; ++d)
            asm volatile("" : "+v"(racc[2 * p][d]), "+v"(racc[2 * p + 1][d]), "+v"(cacc[0][d]), "+v"(cacc[1][d]));
          if constexpr (ERR) asm volatile("" : "+v"(err_tile));
          __builtin_amdgcn_sched_barrier(0);
        }
        // column sums over the 8 lanes a = 0..7 of the column group: lanes a and a ^ 1 hold the two columns in opposite
        // order, so own first + the partner's second is one column's sum over both; then a ^ 2, a ^ 4.  Lane a = 0 ends
        // with column 2h, lane a = 1 with column 2h + 1.  (The diagonal square's sums land in slots nobody reads.)
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
          double v = cacc[0][d] + sym64_xor(cacc[1][d], 1);
          v += sym64_xor(v, 2);
          v += sym64_xor(v, 4);
          cacc[0][d] = v;
        }
        // lanes a = 0 and a = 1 store a column each: a buffer store whose offset lies past the buffer's end for the other
        // lanes (dropped by the bounds check).  No branch: the tile stays ONE basic block -- with a divergent store the
        // optimiser sank the row-sum updates of the whole tile behind it and kept every pair's dx and factor alive
        const int off0 = col_off + ((J * kSymCols + 2 * h) * DIM) * 8;
#pragma unroll
        for (int d = 0; d < DIM; d += 2) {
          if (d + 2 <= DIM) {
            const uint4 pk = __builtin_bit_cast(uint4, (double2){cacc[0][d], cacc[0][d + 1]});
            __builtin_amdgcn_raw_buffer_store_b128((u32x4){pk.x, pk.y, pk.z, pk.w}, col_rsrc, off0 + d * 8, 0, 0);
          } else {
            const uint2 pk = __builtin_bit_cast(uint2, cacc[0][d]);
            typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
            __builtin_amdgcn_raw_buffer_store_b64((u32x2){pk.x, pk.y}, col_rsrc, off0 + d * 8, 0, 0);
          }
        }
      };
      half(std::integral_constant<int, 0>{}, wa, da);
      request(Jn, 0, wa);                  // the next tile's first half, while this tile's second half is computed
      request_delta(Jn, 0, da);
      __builtin_amdgcn_sched_barrier(0);
      half(std::integral_constant<int, 1>{}, wb, db);
      if constexpr (ERR) {
        const bool diag = J < 2 * R + 2;
        err_unit += diag ? err_tile : 2.0 * err_tile;
        cnt_unit2 += diag ? cnt_tile : 2u * cnt_tile;
        err_tile = 0.0;
        cnt_tile = 0;
      }
      __builtin_amdgcn_sched_barrier(0);
      lds[wave][(J + 1) & 1][lane] = make_uint4(rn0.x, rn0.y, rn0.z, rn0.w);
      if constexpr (kTileVec > 64) lds[wave][(J + 1) & 1][lane + 64] = make_uint4(rn1.x, rn1.y, rn1.z, rn1.w);   // (slots >= kTileVec: never read)
    }
    // row sums over the 8 lanes b = 0..7 of a row group (lane bits 3..5); lane b = 0 stores
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
      for (int d = 0; d < DIM; ++d) {
        double v = racc[q][d];
        v += sym64_xor(v, 8);
        v += sym64_xor(v, 16);
        v += sym64_xor(v, 32);
        racc[q][d] = v;
      }
    if (b == 0) {
      double* dst = rowpart + ((size_t)u * kSymRows + 8 * a) * DIM;
#pragma unroll
      for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int d = 0; d < DIM; ++d) dst[q * DIM + d] = racc[q][d];
    }
    if constexpr (ERR) {
      double es = err_unit;
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) es += sym64_xor(es, m);
      if constexpr (ANYTHR) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) cnt_unit2 += __shfl_xor(cnt_unit2, m, 64);
      }
      if (lane == 0) {
        part_sum[u] = es;
        part_cnt[u] = ANYTHR ? (unsigned long long)cnt_unit2 : (u == 0 ? fixed_cnt : 0ull);
      }
    }
  }
