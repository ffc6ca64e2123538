// topolow_amd/csrc/relax_prep_types.h -- the launch constants and the totals of the pre-processing kernels
// (relax_prep.h, relax_prep_fold.h): what struct topolow_layout_prep (topolow_prep.h) and the two kernels a session
// loads from a handle with (relax_kernels.h) need of them.  No kernels here.
#pragma once

#include "relax_common.h"

namespace topolow {

constexpr int kPrepThreads = 256;
constexpr int kPrepWaves = kPrepThreads / 64;

constexpr int kPrepTile = 64;

// Whole-matrix quantities.  Integer counts and a maximum: atomics do not make them depend on the grid.
struct PrepTotals {
  unsigned long long n_finite_nonzero, n_infinite, n_negative, n_inexact;
  unsigned long long max_key;   // prep_order_key of the largest non-NA code-0 value; 0: there is none
};

// Integer counts and a maximum: atomics do not make them depend on the grid.
struct FoldTotals {
  unsigned long long max_key;        // prep_order_key of the largest kept non-NA code-0 value; 0: there is none
  unsigned long long n_upper;        // kept non-NA cells strictly above the diagonal (row < column)
  unsigned long long n_bad_picks;    // picks outside [0, n * n): counted, written nowhere
  unsigned long long n_asymmetric;   // off-diagonal cells that differ from their mirror (fold_symmetry_kernel)
};

}  // namespace topolow
