"""Shared set-up of the exact Gauss-Seidel form tests (tests/test_gpu_exact_gs_forms.py, tests/test_gs_batch_limit.py):
the one-workgroup kernel's size limit read from the library, large problems with threshold codes built on arrays, and the
CPU oracle replaying the library's pair orders.  Test infrastructure."""
import dataclasses
import functools

import numpy as np

from oracle import topolow_oracle as orc
from tests import parity_problems as pp
from tests.conftest import layout_call_args
from topolow_amd import _native

GS_NDIMS = tuple(range(1, 17))      # coordinate counts the exact-GS kernels take (11 runs as 12, 13..15 as 16)
SCAN_TO = 12000                     # beyond every limit: fp32 at ndim 1 needs 20 bytes of LDS per point -> about 8 200


def kernel_dim(ndim):
    """Coordinates the exact-GS kernels carry for a caller's ndim: 11 runs zero-padded as 12, 13..15 as 16."""
    return ndim if ndim <= 10 else (12 if ndim <= 12 else 16)


def lds_bytes(n, dim, real_size, table_edges=0):
    """LDS the one-workgroup kernel carves for n points of `dim` carried coordinates (relax_gs.h, restated from its
    comments: positions | perm (n + 1) | keys | degree terms (f64) | two 16-entry reduction arrays and a flag word, each
    piece rounded up to 16 bytes; the table form adds targets, two round-offset arrays, four 16-bit edge arrays, three
    per-round slot tables of n / 2 entries, rounded up to 8 bytes, and the codes)."""
    def up(x, a):
        return (x + a - 1) // a * a
    total = up(n * dim * real_size, 16) + up((n + 1) * 4, 16) + up(n * 4, 16) + up(n * 8, 16) + 16 * 8 + 16 * 8 + 16
    if table_edges > 0:
        half = (n + (n & 1)) // 2
        total += up(table_edges * real_size, 8) + 2 * up((n + 2) * 4, 8) + 4 * up(table_edges * 2, 8)
        total += up(3 * half * 2, 8) + up(table_edges, 16)
    return total


LDS_LIMIT = 160 * 1024          # what one workgroup of an MI355X may hold (include/topolow_relax.h)
TABLE_BUDGET = 78 * 1024        # the LDS-table form is taken below this (two workgroups per CU still fit)


def table_eligible(call, precision="f64"):
    """Does GsBatch::stage take the LDS-table form for this call when it runs alone (its documented rule: at most
    2 048 points, fewer than 65 535 edges, table within the 78 KB budget; the edge list is the matrix by construction)?"""
    n, dim = call.initial_positions.shape
    ne = int(call.edge_i.shape[0])
    return n <= 2048 and 0 < ne < 65535 and lds_bytes(n, kernel_dim(dim), 4 if precision == "f32" else 8, ne) <= TABLE_BUDGET


@functools.lru_cache(maxsize=None)
def batch_limit(ndim, precision):
    """Largest n with _native.batch_problem_fits(n, ndim, precision, 0), found by bisection; the answer is then checked to
    be monotone over every n in [2, SCAN_TO] (true up to the limit, false beyond it)."""
    fits = lambda n: _native.batch_problem_fits(n, ndim, precision, 0)   # noqa: E731
    assert fits(2) and not fits(SCAN_TO), (ndim, precision)
    lo, hi = 2, SCAN_TO
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if fits(mid):
            lo = mid
        else:
            hi = mid
    flags = np.array([fits(n) for n in range(2, SCAN_TO + 1)])
    assert flags[: lo - 1].all() and not flags[lo - 1:].any(), (ndim, precision, lo)
    return lo


def with_thresholds(call, fraction, seed):
    """`call` with `fraction` of its measured pairs turned into threshold codes that the measured value satisfies: half
    ">" holding 0.9 x the value, half "<" holding 1.1 x (what parity_problems.random_problem(thresholds=...) builds
    through a character matrix, here on the arrays: a loop over the pairs of 2 900 points takes minutes)."""
    if fraction <= 0:
        return call
    rng = np.random.default_rng(seed)
    u = rng.random(call.edge_i.shape[0])
    code = np.where(u < fraction / 2, 1, np.where(u < fraction, -1, 0)).astype(np.int32)
    dist = call.edge_dist * np.where(code == 1, 0.9, np.where(code == -1, 1.1, 1.0))
    D, T = call.dissimilarity_matrix.copy(), call.threshold_matrix.copy()
    i, j = call.edge_i, call.edge_j
    D[i, j] = D[j, i] = dist
    T[i, j] = T[j, i] = code
    return dataclasses.replace(call, dissimilarity_matrix=D, threshold_matrix=T, edge_dist=dist, edge_thresh=code)


def problem(n, dim, missing, seed, thresholds=0.0, **kw):
    """parity_problems.random_problem with the thresholds set on arrays (same fractions, same 0.9 / 1.1 scaling)."""
    call, _ = pp.random_problem(n, dim, missing if n > 4 else 0.0, seed=seed, thresholds=0.0, **kw)
    return with_thresholds(call, thresholds, seed + 1)


def matrix_of_edges(call):
    """The dense arguments that an edge list standing for the matrix means: unlisted pairs unmeasured, diagonal 0,
    degrees counted from the list (+ the diagonal cell, as R/core.R:340 counts it)."""
    n = call.initial_positions.shape[0]
    D = np.full((n, n), np.inf)
    np.fill_diagonal(D, 0.0)
    T = np.zeros((n, n), dtype=np.int32)
    i, j = call.edge_i, call.edge_j
    D[i, j] = D[j, i] = call.edge_dist
    T[i, j] = T[j, i] = call.edge_thresh
    return D, T


def subset_of_edges(call, fraction, seed):
    """`call` restricted to a random `fraction` of its edges, as a call whose list IS the matrix (no dense arrays), and
    the same problem with the dense arrays rebuilt from the list (for the oracle)."""
    rng = np.random.default_rng(seed)
    keep = np.flatnonzero(rng.random(call.edge_i.shape[0]) < fraction)
    n = call.initial_positions.shape[0]
    deg = (1 + np.bincount(call.edge_i[keep], minlength=n) + np.bincount(call.edge_j[keep], minlength=n)).astype(np.int32)
    lean = dataclasses.replace(call, dissimilarity_matrix=None, threshold_matrix=None, degrees=deg,
                               edge_i=call.edge_i[keep], edge_j=call.edge_j[keep], edge_dist=call.edge_dist[keep],
                               edge_thresh=call.edge_thresh[keep])
    D, T = matrix_of_edges(lean)
    return lean, dataclasses.replace(lean, dissimilarity_matrix=D, threshold_matrix=T)


def oracle_gs(call, seed, arith="f64"):
    """The CPU oracle replaying topolow_gs_pair_order (the one-workgroup kernel's order)."""
    n = call.initial_positions.shape[0]

    def order_fn(it, arr):
        arr[:] = _native.gs_pair_order(n, seed, it)
    return orc.optimize_layout_exact(*layout_call_args(call), order_mode=orc.ORDER_SUPPLIED, order_fn=order_fn, arith=arith)


def oracle_tilegs(call, seed, arith="f64"):
    """The CPU oracle replaying topolow_tilegs_pair_order (the tile schedule's order)."""
    n = call.initial_positions.shape[0]

    def order_fn(it, arr):
        arr[:] = _native.tilegs_pair_order(n, seed, it)
    return orc.optimize_layout_exact(*layout_call_args(call), order_mode=orc.ORDER_SUPPLIED, order_fn=order_fn, arith=arith)


def round_targets(values):
    """The sessions' 4-ulp-rounded fp32 target of every finite value (topolow_encode_target), on arrays."""
    values = np.asarray(values, dtype=np.float64)
    out = values.copy()
    fin = np.isfinite(values)
    u = values[fin].astype(np.float32).view(np.uint32)
    mag = ((u & np.uint32(0x7FFFFFFF)) + np.uint32(2)) & np.uint32(0xFFFFFFFC)
    out[fin] = ((u & np.uint32(0x80000000)) | mag).view(np.float32).astype(np.float64)
    sample = np.flatnonzero(fin.ravel())[:64]
    assert all(_native.decode_target(_native.encode_target(values.ravel()[q], 0))[0] == out.ravel()[q] for q in sample)
    return out


def rounded(call):
    """`call` with the targets a session keeps: what the tile schedule's kernels read, given to the oracle."""
    return dataclasses.replace(call, dissimilarity_matrix=round_targets(call.dissimilarity_matrix),
                               edge_dist=round_targets(call.edge_dist))
