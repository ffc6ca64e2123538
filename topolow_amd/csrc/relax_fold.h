// topolow_amd/csrc/relax_fold.h -- host-side construction of one cross-validation fold's problem from
// the cell list of the full matrix (no device code).
//
// Mirrors what the reference does per fold in R (R/adaptive_sampling.R:2600-2640 masks the held-out
// cells, then euclidean_embedding's pre-processing R/core.R:269-436 runs on the masked n x n matrix):
// ordering by mean dissimilarity, degrees, the upper-triangle edge list in column-major scan order,
// and the out-of-sample cells -- but from the list of non-NA cells, O(E log E) instead of several
// n x n passes.  The Python twin is topolow_amd/cv.py: FoldBuilder.fold_numpy, to which this must be
// (and is tested to be) identical, including the last bit of the means that decide the ordering:
// NumPy sums a row of the zero-filled matrix pairwise, and zeros are exact identities of that
// summation tree, so the same tree over the non-zero cells alone gives the same sum.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/topolow_relax.h"

namespace topolow {

// Sum of a dense row of length (hi - lo) whose non-zero entries are (pos[q], val[q]), q in [b, e),
// positions ascending -- in the association order of NumPy's pairwise summation (blocks of 128,
// eight strided accumulators per block, remainder added one by one).
inline double fold_pairwise(const int32_t* pos, const double* val, int b, int e, int lo, int hi) {
  const int len = hi - lo;
  if (len < 8) {
    double res = 0.0;
    for (int q = b; q < e; ++q) res += val[q];
    return res;
  }
  if (len <= 128) {
    double r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int body = len - len % 8;
    int q = b;
    for (; q < e && pos[q] - lo < body; ++q) r[(pos[q] - lo) & 7] += val[q];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; q < e; ++q) res += val[q];
    return res;
  }
  int n2 = len / 2;
  n2 -= n2 % 8;
  const int mid = lo + n2;
  const int m = (int)(std::lower_bound(pos + b, pos + e, mid) - pos);
  return fold_pairwise(pos, val, b, m, lo, mid) + fold_pairwise(pos, val, m, e, mid, hi);
}

// Step 1 of a fold: the held-out cells and their mirrors as indices into the cell list, every cell once,
// ascending (the list is in column-major order, so ascending linear index = ascending list index).
inline int fold_dropped(const topolow_cell_list* L, const int64_t* picks, int64_t n_picks, std::vector<int64_t>& dropped) {
  const int n = L->n;
  std::vector<int64_t> lin;
  lin.reserve((size_t)n_picks * 2);
  for (int64_t q = 0; q < n_picks; ++q) {
    const int64_t r = picks[q] % n, c = picks[q] / n;
    if (picks[q] < 0 || c >= n) return TOPOLOW_ERR_BAD_ARGUMENT;
    lin.push_back(r + c * n);
    lin.push_back(c + r * n);
  }
  std::sort(lin.begin(), lin.end());
  lin.erase(std::unique(lin.begin(), lin.end()), lin.end());
  dropped.clear();
  for (int64_t x : lin) {
    const int64_t at = L->pos_of[x];
    if (at >= 0) dropped.push_back(at);
  }
  return TOPOLOW_OK;
}

// Step 2 of a fold: ordering by mean dissimilarity (R/core.R:269-319): mean of row mean and column mean over the
// non-NA off-diagonal cells, threshold prefixes stripped.  kept_list(q): is cell q still in the fold, asked for q
// ascending; kept_row(i, q): the same, asked row by row (i ascending, q ascending inside a row).  Fills order / inv and
// returns true when the points are reordered (inv stays the identity otherwise).
template <typename KeptList, typename KeptRow>
inline bool fold_order(const topolow_cell_list* L, int32_t preserve_order, KeptList&& kept_list, KeptRow&& kept_row,
                       int32_t* order, std::vector<int32_t>& inv) {
  const int n = L->n;
  const int64_t nc = L->n_cells;
  inv.resize(n);
  for (int i = 0; i < n; ++i) inv[i] = i;
  if (n <= 1 || preserve_order) return false;
  std::vector<double> avg(n);
  std::vector<int32_t> pos;
  std::vector<double> val;
  std::vector<double> csum(n, 0.0);
  std::vector<int32_t> ccnt(n, 0);
  // column sums: NumPy adds the rows of the matrix one after another, i.e. per column in
  // ascending row order -- the order of the (column-major) cell list itself
  for (int64_t q = 0; q < nc; ++q) {
    if (!kept_list(q) || L->row[q] == L->col[q]) continue;
    csum[L->col[q]] += L->value[q];
    ccnt[L->col[q]] += 1;
  }
  for (int i = 0; i < n; ++i) {
    pos.clear();
    val.clear();
    for (int64_t p = L->row_ptr[i]; p < L->row_ptr[i + 1]; ++p) {
      const int64_t q = L->by_row[p];
      if (!kept_row(i, q) || L->col[q] == i) continue;
      pos.push_back(L->col[q]);
      val.push_back(L->value[q]);
    }
    const double rs = fold_pairwise(pos.data(), val.data(), 0, (int)pos.size(), 0, n);
    const double rm = pos.empty() ? NAN : rs / (double)pos.size();
    const double cm = ccnt[i] == 0 ? NAN : csum[i] / (double)ccnt[i];
    const double a = (rm + cm) / 2.0;
    avg[i] = std::isnan(a) ? 0.0 : a;
  }
  int positive = 0;
  for (int i = 0; i < n; ++i) positive += avg[i] > 0 ? 1 : 0;
  if (positive <= 1) return false;
  std::vector<int32_t> ord(n);
  for (int i = 0; i < n; ++i) ord[i] = i;
  std::stable_sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return avg[x] < avg[y]; });
  for (int i = 0; i < n; ++i) { order[i] = ord[i]; inv[ord[i]] = i; }
  return true;
}

inline int fold_problem(const topolow_cell_list* L, const int64_t* picks, int64_t n_picks,
                        int32_t preserve_order, int32_t named, int32_t* order, int32_t* degrees,
                        int32_t* edge_i, int32_t* edge_j, double* edge_dist, int32_t* edge_thresh,
                        int64_t* n_edges, int32_t* hold_i, int32_t* hold_j, double* hold_truth,
                        int64_t* n_hold, double* numeric_max) {
  const int n = L->n;
  const int64_t nc = L->n_cells;
  if (n < 1 || nc < 0) return TOPOLOW_ERR_BAD_ARGUMENT;
  // 1. the held-out cells and their mirrors, every cell once, ascending linear (column-major) index
  std::vector<int64_t> dropped;
  const int rc = fold_dropped(L, picks, n_picks, dropped);
  if (rc != TOPOLOW_OK) return rc;
  std::vector<char> keep((size_t)nc, 1);
  for (int64_t at : dropped) keep[(size_t)at] = 0;
  // 2. ordering by mean dissimilarity
  std::vector<int32_t> inv;
  const bool reordered = fold_order(L, preserve_order, [&](int64_t q) { return keep[(size_t)q] != 0; },
                                    [&](int, int64_t q) { return keep[(size_t)q] != 0; }, order, inv);
  if (!reordered) order[0] = -1;
  // 3. degrees (non-NA cells of a row, diagonal included: R/core.R:341), edges, largest numeric value
  for (int i = 0; i < n; ++i) degrees[i] = 0;
  struct Edge { int32_t i, j; double d; int32_t t; };
  std::vector<Edge> edges;
  edges.reserve((size_t)nc / 2 + 1);
  double vmax = NAN;
  for (int64_t q = 0; q < nc; ++q) {
    if (!keep[(size_t)q]) continue;
    const int32_t r = inv[L->row[q]], c = inv[L->col[q]];
    degrees[r] += 1;
    if (L->code[q] == 0 && !(L->value[q] <= vmax)) vmax = L->value[q];   // NaN-safe running maximum
    if (r < c) edges.push_back(Edge{r, c, L->value[q], L->code[q]});
  }
  std::sort(edges.begin(), edges.end(), [](const Edge& a, const Edge& b) {
    return a.j != b.j ? a.j < b.j : a.i < b.i;                           // column-major scan
  });
  for (size_t q = 0; q < edges.size(); ++q) {
    edge_i[q] = edges[q].i; edge_j[q] = edges[q].j; edge_dist[q] = edges[q].d; edge_thresh[q] = edges[q].t;
  }
  *n_edges = (int64_t)edges.size();
  *numeric_max = vmax;
  // 4. out-of-sample cells: held out AND numeric in the truth; lined up with the prediction by name
  //    (R/error_metrics.R:100-112) -- an unnamed matrix is compared in the returned numbering
  int64_t nh = 0;
  for (int64_t at : dropped) {
    if (L->code[at] != 0) continue;
    hold_i[nh] = named ? inv[L->row[at]] : L->row[at];
    hold_j[nh] = named ? inv[L->col[at]] : L->col[at];
    hold_truth[nh] = L->value[at];
    ++nh;
  }
  *n_hold = nh;
  return TOPOLOW_OK;
}

// Is the cell list symmetric: every off-diagonal cell has its mirror, with the same value and code?  What a session
// needs to hold a fold out of ONE resident block (with asymmetric NA the reference reads the upper triangle of the
// per-fold REORDERED matrix, which cell is "upper" then changes from fold to fold).
constexpr const char* kAsymmetricCells =
    "the cell list is not symmetric (an off-diagonal cell without its mirror, or with another value or code): one "
    "resident block cannot represent the per-fold reordered upper triangle the reference reads; use topolow_cv_sweep";
inline bool fold_cells_symmetric(const topolow_cell_list* L) {
  const int n = L->n;
  for (int64_t q = 0; q < L->n_cells; ++q) {
    const int64_t r = L->row[q], c = L->col[q];
    if (r == c) continue;
    const int64_t m = L->pos_of[c + r * n];
    if (m < 0 || !(L->value[m] == L->value[q]) || L->code[m] != L->code[q]) return false;
  }
  return true;
}

// A fold as a resident session holds it out (topolow_session_hold_out / _score_pairs): the same fold as fold_problem
// builds, without its edge list -- everything in the CALLER's labels, host memory O(n + picks).
struct FoldPairs {
  std::vector<int32_t> order;     // order[0] = -1: input order kept (as fold_problem)
  std::vector<int32_t> degrees;   // per caller's point
  std::vector<int32_t> pair_i, pair_j;                // unique held-out unordered pairs, i < j
  std::vector<int32_t> score_i, score_j;              // scored cells: held out AND numeric, every mirror on its own;
  std::vector<double> score_truth;                    // an unnamed matrix is scored in the returned numbering (-> order)
  int64_t n_edges = 0;            // measured upper-triangle cells the fold keeps
  double numeric_max = NAN;
};

inline int fold_pairs(const topolow_cell_list* L, const int64_t* picks, int64_t n_picks, int32_t preserve_order,
                      int32_t named, FoldPairs& out) {
  const int n = L->n;
  const int64_t nc = L->n_cells;
  if (n < 1 || nc < 0) return TOPOLOW_ERR_BAD_ARGUMENT;
  std::vector<int64_t> dropped;
  const int rc = fold_dropped(L, picks, n_picks, dropped);
  if (rc != TOPOLOW_OK) return rc;
  // the dropped cells once more in row-by-row order, for the row pass of the ordering
  std::vector<int64_t> by_row(dropped);
  std::sort(by_row.begin(), by_row.end(), [&](int64_t a, int64_t b) {
    return L->row[a] != L->row[b] ? L->row[a] < L->row[b] : a < b;
  });
  size_t pc = 0, pr = 0;   // cursors: both passes ask in ascending order
  auto kept_list = [&](int64_t q) {
    while (pc < dropped.size() && dropped[pc] < q) ++pc;
    return !(pc < dropped.size() && dropped[pc] == q);
  };
  auto kept_row = [&](int i, int64_t q) {
    while (pr < by_row.size() && (L->row[by_row[pr]] < i || (L->row[by_row[pr]] == i && by_row[pr] < q))) ++pr;
    return !(pr < by_row.size() && by_row[pr] == q);
  };
  out.order.assign(n, 0);
  std::vector<int32_t> inv;
  const bool reordered = fold_order(L, preserve_order, kept_list, kept_row, out.order.data(), inv);
  if (!reordered) out.order[0] = -1;
  // degrees, kept upper-triangle cells, largest numeric value: the loop of fold_problem's step 3
  out.degrees.assign(n, 0);
  double vmax = NAN;
  int64_t ne = 0;
  pc = 0;
  for (int64_t q = 0; q < nc; ++q) {
    if (!kept_list(q)) continue;
    out.degrees[L->row[q]] += 1;
    if (L->code[q] == 0 && !(L->value[q] <= vmax)) vmax = L->value[q];
    if (L->row[q] < L->col[q]) ++ne;
  }
  out.n_edges = ne;
  out.numeric_max = vmax;
  out.pair_i.clear(); out.pair_j.clear(); out.score_i.clear(); out.score_j.clear(); out.score_truth.clear();
  for (int64_t at : dropped) {
    const int32_t r = L->row[at], c = L->col[at];
    if (r < c) { out.pair_i.push_back(r); out.pair_j.push_back(c); }
    if (L->code[at] != 0) continue;
    // fold_problem scores (inv[r], inv[c]) of the reordered problem when named, (r, c) of it otherwise: the points
    // order[inv[r]] = r and order[r] of the caller
    out.score_i.push_back(named || !reordered ? r : out.order[r]);
    out.score_j.push_back(named || !reordered ? c : out.order[c]);
    out.score_truth.push_back(L->value[at]);
  }
  return TOPOLOW_OK;
}

// What a sweep makes of a built fold (rc of fold_problem / fold_pairs): a fold without valid measurements, or whose
// unit draws are not the (ndim, n - 1) numbers of its start walk, is left out with TOPOLOW_ERR_BAD_ARGUMENT.
inline int fold_check(int rc, int64_t n_edges, double numeric_max, int ndim, int64_t n_draws, int n) {
  if (rc != TOPOLOW_OK) return rc;
  if (n_edges == 0 || !(numeric_max == numeric_max)) return TOPOLOW_ERR_BAD_ARGUMENT;   // no valid measurements
  if (ndim < 1 || n_draws != (int64_t)ndim * (n - 1)) return TOPOLOW_ERR_BAD_ARGUMENT;
  return TOPOLOW_OK;
}

// Start positions from the caller's unit draws ((ndim, n - 1), row-major) with NumPy's / R's arithmetic: a random walk
// from the origin whose steps are uniform(0, 2 max / n), R/core.R:407-415.  out: n x ndim, column-major; point i of the
// walk is row i, or row order[i] where an order is given (point i of a fold's order = the caller's point order[i]).
inline void start_walk(const double* unit_draws, double vmax, int n, int ndim, const int32_t* order, std::vector<double>& out) {
  const double step = vmax / (double)n;
  out.assign((size_t)n * ndim, 0.0);
  for (int d = 0; d < ndim; ++d) {
    double acc = 0.0;
    for (int i = 1; i < n; ++i) {
      const double st_ = 0.0 + (2.0 * step - 0.0) * unit_draws[(size_t)d * (n - 1) + (i - 1)];   // Generator.uniform's arithmetic
      acc = i == 1 ? st_ : acc + st_;                             // cumsum
      out[(size_t)(order ? order[i] : i) + (size_t)d * n] = acc;
    }
  }
}

}  // namespace topolow
