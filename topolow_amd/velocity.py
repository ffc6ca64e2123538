"""Antigenic velocity of a finished map: the reference's compute_kernel_velocity (R/visualization.R:802-843) and the
bandwidths plot_temporal_mapping / plot_cluster_mapping give it by default (:1157-1173, :1743-1757).

`kernel_velocity(..., device=None)` is the host form in NumPy and the specification: it follows the reference line
by line.  With a device it runs topolow_kernel_velocity (csrc/relax_velocity.h), which has no host fallback.
`prepare_clade_membership` is not here: the clade rule takes any dictionary of member lists.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

from . import _native


class CladeRule:
    """The clade rule (:816-823), one row at a time: row(i) is None when names[i] has no entry in clade_members (every
    earlier point is eligible), else the boolean vector of the points that do not contribute to row i -- names[j] is in
    tree_present_points and not in the entry, the reference's setdiff(tree_present_points, clade_members[[i]]).  A row
    costs O(n) for the copy and O(len(entry)) for the members; no n x n array is built."""

    def __init__(self, names, clade_members, tree_present_points):
        self.names = list(names)
        self.n = len(self.names)
        self.clade_members = clade_members
        in_tree = set(tree_present_points if tree_present_points is not None else ())
        self.tree_col = np.array([nm in in_tree for nm in self.names], dtype=bool)
        self.where = {}
        for j, nm in enumerate(self.names):
            self.where.setdefault(nm, []).append(j)

    def row(self, i):
        if self.names[i] not in self.clade_members:
            return None
        out = self.tree_col.copy()
        for member in self.clade_members[self.names[i]]:
            if member in self.where:                     # a member that is no point excludes and spares nobody
                out[self.where[member]] = False
        return out

    def bits(self) -> np.ndarray:
        """The rule as the library's n x ceil(n / 64) words, packed row by row."""
        out = np.zeros((self.n, (self.n + 63) // 64), dtype=np.uint64)
        for i in range(self.n):
            r = self.row(i)
            if r is not None:
                out[i] = pack_exclusion_bits(r[None, :])[0]
        return out


def exclusion_matrix(names, clade_members, tree_present_points) -> np.ndarray:
    """CladeRule as an n x n boolean matrix: [i, j] is True when j does not contribute to row i.  For tests and small
    maps; kernel_velocity itself goes row by row."""
    rule = CladeRule(names, clade_members, tree_present_points)
    out = np.zeros((rule.n, rule.n), dtype=bool)
    for i in range(rule.n):
        r = rule.row(i)
        if r is not None:
            out[i] = r
    return out


def pack_exclusion_bits(mask) -> np.ndarray:
    """A boolean matrix of n columns (n x n: the whole rule) as the library's 64-bit words, ceil(n / 64) per row: bit
    (j % 64) of word (j // 64) of row i is mask[i, j].  Packed in blocks of rows: the temporaries stay at a few MB."""
    mask = np.asarray(mask, dtype=bool)
    if mask.ndim != 2:
        raise ValueError("the exclusion matrix must have two dimensions")
    rows, n = mask.shape
    words = (n + 63) // 64
    out = np.empty((rows, words), dtype=np.uint64)
    block = max(1, (1 << 22) // max(1, words * 64))
    for r0 in range(0, rows, block):
        part = mask[r0:r0 + block]
        padded = np.zeros((part.shape[0], words * 64), dtype=np.uint8)
        padded[:, :n] = part
        out[r0:r0 + block] = np.packbits(padded, axis=1, bitorder="little").view("<u8")
    return out


def _host_velocity(X, t, sigma_t, sigma_x, excluded):
    """excluded: None, an n x n boolean matrix, or a function i -> boolean row or None (CladeRule.row)."""
    n, k = X.shape
    V = np.full((n, k), np.nan)
    weight_sum = np.zeros(n)
    for i in range(n):
        past = t < t[i]                                    # strict; a NaN on either side compares False
        out = None if excluded is None else (excluded(i) if callable(excluded) else excluded[i])
        if out is not None:
            past &= ~out
        past_indices = np.flatnonzero(past)
        if past_indices.size:
            dt = t[i] - t[past_indices]
            dX = X[i] - X[past_indices]
            d2 = (dX ** 2).sum(axis=1)
            w = np.exp(-d2 / (2 * sigma_x ** 2)) * np.exp(-(dt ** 2) / (2 * sigma_t ** 2))
            w_sum = w.sum()
            weight_sum[i] = w_sum
            if w_sum > 0:
                V[i] = (w[:, None] * (dX / dt[:, None])).sum(axis=0) / w_sum
    return V, weight_sum


def kernel_velocity(positions, times, sigma_t, sigma_x, names=None, clade_members=None, tree_present_points=None,
                    device: Optional[int] = None):
    """Kernel-weighted antigenic velocity of every point: returns (V n x ndim, magnitude n, weight_sum n).

    For row i over the points j with times[j] < times[i] (strictly) that the clade rule leaves eligible:
    w = exp(-||x_i - x_j||^2 / (2 sigma_x^2)) * exp(-(t_i - t_j)^2 / (2 sigma_t^2)), V[i] = sum w (x_i - x_j) /
    (t_i - t_j) / sum w; V[i] is NaN (R's NA) where there is no eligible past point or every weight is 0, and
    magnitude = sqrt(rowSums(V^2)).  weight_sum is the denominator (0 without an eligible past point).
    clade_members: None, or a dictionary name -> member names; with tree_present_points it excludes from row i every
    tree point outside i's clade when i has an entry (names default to 0 .. n-1).
    device=None computes on the host; a device ordinal runs the HIP kernel (one exp of the summed exponent in place of
    the product of two: see include/topolow_relax.h).  With clades the device form packs the rule row by row into
    n x ceil(n / 64) words (n^2 / 8 bytes: 12.5 MB at 10 000 points, 313 MB at 50 000) and the library permutes the
    bits of every row's past to its sorted order on the host, about n^2 / 2 single-bit moves over up to 16 threads."""
    X = np.asarray(positions, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("positions must be an n x ndim matrix")
    n = X.shape[0]
    t = np.asarray(times, dtype=np.float64)
    if t.shape != (n,):
        raise ValueError("times must hold one value per position")
    if not (math.isfinite(sigma_t) and sigma_t > 0 and math.isfinite(sigma_x) and sigma_x > 0):
        raise ValueError("sigma_t and sigma_x must be finite and > 0")
    rule = None
    if clade_members is not None:
        names = list(range(n)) if names is None else list(names)
        if len(names) != n:
            raise ValueError("names must hold one name per position")
        rule = CladeRule(names, clade_members, tree_present_points)
    if device is None:
        V, weight_sum = _host_velocity(X, t, float(sigma_t), float(sigma_x), rule.row if rule is not None else None)
    else:
        bits = rule.bits() if rule is not None else None
        V, weight_sum = _native.kernel_velocity(X, t, sigma_t, sigma_x, bits, device=device)
        V = np.ascontiguousarray(V)
    return V, np.sqrt((V ** 2).sum(axis=1)), weight_sum


def silverman_bandwidth(x) -> float:
    """R's bw.nrd: 1.06 * min(sd, IQR / 1.34) * n^(-1/5), quantiles of type 7."""
    x = np.asarray(x, dtype=np.float64).ravel()
    if x.size < 2:
        raise ValueError("need at least 2 data points")
    q1, q3 = np.quantile(x, [0.25, 0.75])
    h = (q3 - q1) / 1.34
    return 1.06 * min(math.sqrt(np.var(x, ddof=1)), h) * x.size ** (-1 / 5)


def _pairs_at_most(s, v):
    """How many pairs i < j of the sorted s have fl(s[j] - s[i]) <= v.  fl is monotone, so per i the pairs are a run
    j in (i, hi[i]); searchsorted on s[i] + v lands within a rounding of its end and is then moved by whole blocks of
    equal values until the subtraction itself agrees."""
    n = s.size
    first = np.arange(1, n + 1)
    hi = np.maximum(np.searchsorted(s, s + v, side="right"), first)
    while True:
        grow = np.flatnonzero(hi < n)
        grow = grow[s[hi[grow]] - s[grow] <= v]
        if grow.size:
            hi[grow] = np.searchsorted(s, s[hi[grow]], side="right")
            continue
        shrink = np.flatnonzero(hi > first)
        shrink = shrink[s[hi[shrink] - 1] - s[shrink] > v]
        if shrink.size:
            hi[shrink] = np.maximum(np.searchsorted(s, s[hi[shrink] - 1], side="left"), first[shrink])
            continue
        return int((hi - first).sum())


def _pair_difference_order_statistic(s, rank):
    """The rank-th smallest (0-based) of the n (n - 1) / 2 values |s[j] - s[i]| of the sorted s, without forming them:
    bisection over the bit patterns of the non-negative doubles (which sort like the numbers) for the smallest v
    with more than `rank` pairs <= v.  That v is one of the differences, with the bits the subtraction gives."""
    lo, hi = 0, int(np.float64(s[-1] - s[0]).view(np.uint64))
    while lo < hi:
        mid = (lo + hi) // 2
        if _pairs_at_most(s, np.uint64(mid).view(np.float64)) > rank:
            hi = mid
        else:
            lo = mid + 1
    return float(np.uint64(lo).view(np.float64))


def _pair_difference_quartiles(s):
    """The type-7 quartiles of the pair differences of the sorted s: each from the two order statistics around it,
    interpolated as numpy.quantile interpolates (by numpy.quantile itself, on the two of them)."""
    n = s.size
    m = n * (n - 1) // 2
    quartiles = []
    for p in (0.25, 0.75):
        virtual = (m - 1) * p
        below = int(math.floor(virtual))
        a = _pair_difference_order_statistic(s, below)
        b = _pair_difference_order_statistic(s, min(below + 1, m - 1))
        quartiles.append(float(np.quantile(np.array([a, b]), virtual - below)))
    return quartiles


def pair_difference_bandwidth(times) -> float:
    """bw.nrd(dist(times)) with no n^2-sized temporary.  Over the m = n (n - 1) / 2 pair differences d, from the
    sorted times s and the sorted CENTRED times c:  sum |d| = sum_k (2k - n + 1) c_(k),  sum d^2 = n sum c^2 -
    (sum c)^2  (centring keeps both free of cancellation against the times' offset), and each quartile from the two
    order statistics around it, found by bisection (_pair_difference_quartiles)."""
    s = np.sort(np.asarray(times, dtype=np.float64).ravel())
    n = s.size
    if n < 3:
        raise ValueError("need at least 3 times (2 pair differences)")
    if not np.isfinite(s).all():
        raise ValueError("times must be finite")
    m = n * (n - 1) // 2
    c = s - math.fsum(s) / n
    k = np.arange(n, dtype=np.float64)
    sum_abs = math.fsum((2.0 * k - (n - 1)) * c)
    sum_sq = n * math.fsum(c * c) - math.fsum(c) ** 2
    var = (sum_sq - sum_abs * sum_abs / m) / (m - 1)
    quartiles = _pair_difference_quartiles(s)
    h = (quartiles[1] - quartiles[0]) / 1.34
    return 1.06 * min(math.sqrt(max(var, 0.0)), h) * m ** (-1 / 5)


def default_bandwidths(positions, times):
    """The reference's default bandwidths: (sigma_x_nd, sigma_t) with sigma_x_nd the root mean square of the
    per-dimension bw.nrd (:1167-1172) and sigma_t = bw.nrd(dist(times)) (:1745)."""
    X = np.asarray(positions, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("positions must be an n x ndim matrix")
    sigma_x = math.sqrt(float(np.mean([silverman_bandwidth(X[:, d]) ** 2 for d in range(X.shape[1])])))
    return sigma_x, pair_difference_bandwidth(times)
