// topolow_amd/csrc/relax_symm_plan.h -- the symmetric sweep's tile geometry, its plan types and the host planner
// (the kernels: relax_symm.h, relax_symm64.h, relax_symm_wide.h).  No kernels here: struct topolow_session
// (topolow_session.h) holds plans on the device, so every source of the library reads this file.
#pragma once

#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>
#include "relax_common.h"

namespace topolow {

constexpr int kSymRows = 64;   // rows of a tile: 8 lane groups a x 8 rows
constexpr int kSymCols = 32;   // columns of a tile: 8 lane groups b x 4 columns
constexpr int kSymTileWords = kSymRows * kSymCols;
constexpr int kSymWaves = 4;   // waves per workgroup (independent of one another)

// One point as the sweep reads it: DIM coordinates, then ks = 2k / (4 g + k) and cg = (c_rep / 2) / g of THIS
// iteration (relax_kernels.h: pair_accum), padded to a multiple of 4 floats.
template <int DIM> struct SymRec { static constexpr int W = (DIM + 2 + 3) & ~3; };

struct SymUnit {
  int tile_row;   // R: rows [64 R, 64 R + 64)
  int j0, j1;     // column blocks [j0, j1) of 32 columns, j0 >= 2 R
  int tile0;      // index of tile (R, j0) in the tile-major copy of the upper triangle (sym_tile_index)
};   // unit u stores its row partial and its error partial in slot u; the units of a tile-row are consecutive

// The sweep reads the targets from a TILE-MAJOR copy of the upper triangle (incl. the whole 64 x 64 squares on the
// diagonal): with TC = npad / 32 column blocks, tile (R, J), J >= 2 R, is 8 KB at tile index R TC - R (R - 1) + (J - 2 R),
// so a unit is one contiguous run.  Inside a tile a lane's eight 16-byte loads are the (column half h, row pair p)
// groups in the order the sweep consumes them: the words of rows 8a + 2p + {0, 1} x columns 4b + 2h + {0, 1} sit at
// (((4 h + p) * 64 + a + 8 b) * 4 + 2 (f ^ (a & 1)) + e) -- a column's two rows adjacent, as the packed pair update
// reads them, and the two columns of a half in opposite order for odd and even a: a lane sweeps "its first" column
// then "its second", which for odd a are columns 2h + 1 and 2h, so that the first step of the column reduction --
// between the lanes a and a ^ 1 -- can add the one's first to the other's second with one instruction per
// coordinate (sym_col_reduce).  Each load of the wave covers 1 KB.
TL_HD inline long long sym_tile_index(int R, int J, int TC) { return (long long)R * TC - (long long)R * (R - 1) + (J - 2 * R); }
TL_HD inline size_t sym_word_in_tile(int r, int c) {   // r in [0, 64), c in [0, 32)
  const int a = r >> 3, p = (r & 7) >> 1, e = r & 1, b = c >> 2, h = (c & 3) >> 1, f = c & 1;
  return (size_t)((((4 * h + p) * 64) + a + 8 * b) * 4 + 2 * (f ^ (a & 1)) + e);
}

// Host: the plan of a sweep over npad / 64 tile-rows for a grid of n_waves waves.
//   units      : tile-row-major; unit u covers column blocks [j0, j1) of tile-row R
//   wave_first : n_waves + 1 entries, wave w sweeps units [wave_first[w], wave_first[w + 1]) (the kernel reads runs())
//   row_units  : per tile-row (first unit, number of units)
struct alignas(32) SymRun {   // one wave's run: units [u0, u1), the first of them inline (one load instead of two dependent ones)
  int u0, u1;
  SymUnit first;
  int tiles;         // tiles of the whole run: the sweep's issue priority follows the share of them still to do
  int reserved;      // (32 bytes: one aligned scalar load)
};
struct SymPlan {
  std::vector<SymUnit> units;
  std::vector<int> wave_first;
  std::vector<int2> row_units;
  std::vector<SymRun> runs() const {       // what the kernel reads: wave_first with every wave's first unit beside it
    std::vector<SymRun> r(wave_first.size() - 1);
    for (size_t w = 0; w + 1 < wave_first.size(); ++w) {
      r[w].u0 = wave_first[w];
      r[w].u1 = wave_first[w + 1];
      r[w].first = r[w].u0 < r[w].u1 ? units[r[w].u0] : SymUnit{0, 0, 0, 0};
      r[w].tiles = 0;
      for (int u = r[w].u0; u < r[w].u1; ++u) r[w].tiles += units[u].j1 - units[u].j0;
      r[w].reserved = 0;
    }
    return r;
  }
};
// The plan of the tiles [t0, t1) of the tile-row-major list (a SEGMENT: the whole list on one GPU, one of P equal
// runs of it when the sweep is sharded over P row-block sessions): tile0 counts from t0, row_units is indexed by
// R - r_first and covers the tile-rows [r_first, r_last] that hold a tile of the segment.
inline SymPlan relax_symm_plan(int npad, int n_waves, long long t0 = 0, long long t1 = -1, int* r_first = nullptr,
                               int* r_last = nullptr) {
  SymPlan P;
  const int TR = npad / kSymRows, TC = npad / kSymCols;
  if (t1 < 0) t1 = (long long)TR * (TR + 1);
  const long long total = t1 - t0;
  int rf = -1, rl = -1;
  for (int R = 0; R < TR; ++R) {
    const long long a = sym_tile_index(R, 2 * R, TC), b = a + (TC - 2 * R);
    if (b > t0 && a < t1) { if (rf < 0) rf = R; rl = R; }
  }
  if (r_first) *r_first = rf;
  if (r_last) *r_last = rl;
  P.wave_first.assign(n_waves + 1, 0);
  if (rf < 0) return P;
  P.row_units.resize(rl - rf + 1);
  long long done = 0;   // tiles handed out so far
  int w = 0;
  long long w_end = (total * (w + 1) + n_waves - 1) / n_waves;   // wave w's run ends at tile w_end (exclusive)
  for (int R = rf; R <= rl; ++R) {
    P.row_units[R - rf].x = (int)P.units.size();
    const long long row0 = sym_tile_index(R, 2 * R, TC);
    int j = 2 * R + (int)std::max<long long>(0, t0 - row0);
    const int j_end = 2 * R + (int)std::min<long long>(TC - 2 * R, t1 - row0);
    while (j < j_end) {
      while (done >= w_end && w + 1 < n_waves) {
        ++w;
        P.wave_first[w] = (int)P.units.size();
        w_end = (total * (w + 1) + n_waves - 1) / n_waves;
      }
      const int take = (int)std::min<long long>(j_end - j, std::max<long long>(w_end - done, 1));
      P.units.push_back({R, j, j + take, (int)(sym_tile_index(R, j, TC) - t0)});
      j += take;
      done += take;
    }
    P.row_units[R - rf].y = (int)P.units.size() - P.row_units[R - rf].x;
  }
  for (int q = w + 1; q <= n_waves; ++q) P.wave_first[q] = (int)P.units.size();
  return P;
}

// ---- multi-stage iterations on the symmetric sweep: S stages that split the PAIRS (S = 2, 4, 8) -----------------------
// The tile-rows are cut into S slabs (tile-rows [q TR / S, (q + 1) TR / S)); stage st sweeps the pairs between slabs a and
// b with (a + b) mod S == st -- for every slab a exactly one partner slab b = (st - a) mod S, itself included -- so over
// the S stages every point meets each slab once, both ends of a pair move in the same stage, and every pair is evaluated
// once per iteration.  In the upper triangle the pairs (a, b) live in the tile-rows of min(a, b).
TL_HD inline int sym_rr_bound(int TR, int S, int q) { return (int)((long long)q * TR / S); }
TL_HD inline int sym_rr_slab(int TR, int S, int R) {
  int q = 0;
  while (q + 1 < S && R >= sym_rr_bound(TR, S, q + 1)) ++q;
  return q;
}
// The column blocks [j0, j1) of tile-row R that stage st sweeps (empty: j0 >= j1).
TL_HD inline void sym_rr_row(int TR, int S, int st, int R, int& j0, int& j1) {
  const int a = sym_rr_slab(TR, S, R), b = ((st - a) % S + S) % S;
  if (b < a) { j0 = j1 = 0; return; }
  j0 = b == a ? 2 * R : 2 * sym_rr_bound(TR, S, b);
  j1 = 2 * sym_rr_bound(TR, S, b + 1);
}
// The tile-rows [rp0, rp1) whose column sums of stage st belong to a point of tile-row R (symm_apply_kernel).
TL_HD inline void sym_rr_above(int TR, int S, int st, int R, int& rp0, int& rp1) {
  const int c = sym_rr_slab(TR, S, R), a = ((st - c) % S + S) % S;
  if (a > c) { rp0 = rp1 = 0; return; }
  rp0 = sym_rr_bound(TR, S, a);
  rp1 = a == c ? R : sym_rr_bound(TR, S, a + 1);
}
// The order of the stages in iteration `iter` (random per iteration, like the slabs of the row-owner form).
TL_HD inline void sym_rr_order(uint64_t seed, int iter, int S, int* perm) {
  for (int q = 0; q < S; ++q) perm[q] = q;
  for (int q = S - 1; q > 0; --q) {
    const uint32_t r = rnd_below(rnd64(seed, 0x2a1f5ull, ((uint64_t)iter << 8) | (uint64_t)q), (uint32_t)(q + 1));
    const int tmp = perm[q]; perm[q] = perm[r]; perm[r] = tmp;
  }
}

// The plan of an arbitrary set of tiles given per tile-row as ONE interval of column blocks: rows_j(R, j0, j1) sets the
// interval [j0, j1) of tile-row R (j0 >= 2 R; empty when j0 >= j1).  Equal runs per wave as above; row_units covers all
// tile-rows.  Used for the stages of a multi-stage iteration (topolow_symm.hip: sym_rr_plan).
template <typename RowsJ>
inline SymPlan relax_symm_plan_rows(int npad, int n_waves, RowsJ rows_j) {
  SymPlan P;
  const int TR = npad / kSymRows, TC = npad / kSymCols;
  long long total = 0;
  for (int R = 0; R < TR; ++R) {
    int j0 = 0, j1 = 0;
    rows_j(R, j0, j1);
    if (j1 > j0) total += j1 - j0;
  }
  P.wave_first.assign(n_waves + 1, 0);
  P.row_units.assign(TR, int2{0, 0});
  if (total == 0) return P;
  long long done = 0;
  int w = 0;
  long long w_end = (total * (w + 1) + n_waves - 1) / n_waves;
  for (int R = 0; R < TR; ++R) {
    P.row_units[R].x = (int)P.units.size();
    int j = 0, j_end = 0;
    rows_j(R, j, j_end);
    while (j < j_end) {
      while (done >= w_end && w + 1 < n_waves) {
        ++w;
        P.wave_first[w] = (int)P.units.size();
        w_end = (total * (w + 1) + n_waves - 1) / n_waves;
      }
      const int take = (int)std::min<long long>(j_end - j, std::max<long long>(w_end - done, 1));
      P.units.push_back({R, j, j + take, (int)sym_tile_index(R, j, TC)});
      j += take;
      done += take;
    }
    P.row_units[R].y = (int)P.units.size() - P.row_units[R].x;
  }
  for (int q = w + 1; q <= n_waves; ++q) P.wave_first[q] = (int)P.units.size();
  return P;
}

}  // namespace topolow
