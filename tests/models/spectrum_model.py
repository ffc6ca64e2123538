"""NumPy model of the device's symmetric eigenvalue path (topolow_amd/csrc/relax_spectrum.h): unblocked Householder
tridiagonalisation with the rank-2 update of the trailing matrix, then Sturm bisection with dstebz's pivmin guard.
The same algorithm with NumPy's own summation order.  It sets the constant of the eigenvalue tolerance
(tests/spectrum_helpers.py) against np.linalg.eigvalsh and serves the CPU tests; the product never imports it."""
import numpy as np

U = 2.0 ** -52


def tridiagonalize(a):
    """(d, e) of Q^T A Q for the symmetric matrix whose lower triangle is a's."""
    a = np.array(a, dtype=np.float64)
    n = a.shape[0]
    A = np.tril(a) + np.tril(a, -1).T
    d, e = np.zeros(n), np.zeros(max(n - 1, 0))
    for k in range(n - 1):
        d[k] = A[k, k]
        x = A[k + 1:, k].copy()
        tail2 = float(x[1:] @ x[1:])
        if x.shape[0] == 1 or tail2 == 0.0:      # nothing below the sub-diagonal: no reflection
            e[k] = x[0]
            continue
        alpha = -np.copysign(np.sqrt(x[0] * x[0] + tail2), x[0])
        v = x
        v[0] = x[0] - alpha
        beta = 2.0 / (v[0] * v[0] + tail2)
        e[k] = alpha
        T = A[k + 1:, k + 1:]
        p = beta * (T @ v)
        w = p - (0.5 * beta * (p @ v)) * v
        T -= np.outer(v, w) + np.outer(w, v)
    d[n - 1] = A[n - 1, n - 1]
    return d, e


def sturm_count(d, e2, x, pivmin):
    """Eigenvalues below each x (a vector), by the guarded Sturm sequence."""
    q = d[0] - x
    q = np.where(np.abs(q) < pivmin, -pivmin, q)
    count = (q < 0).astype(np.int64)
    for i in range(1, d.shape[0]):
        q = d[i] - x - e2[i - 1] / q
        q = np.where(np.abs(q) < pivmin, -pivmin, q)
        count += q < 0
    return count


def bisect(d, e):
    """All eigenvalues of the tridiagonal (d, e), descending."""
    d, e = np.asarray(d, dtype=np.float64), np.asarray(e, dtype=np.float64)
    n = d.shape[0]
    e2 = e * e
    r = np.zeros(n)
    r[1:] += np.abs(e)
    r[:-1] += np.abs(e)
    pivmin = np.finfo(np.float64).tiny * max(1.0, float(e2.max()) if n > 1 else 0.0)
    lo0, hi0 = float((d - r).min()), float((d + r).max())
    widen = 2.1 * max(abs(lo0), abs(hi0)) * U * n + 2.1 * 2.0 * pivmin
    lo, hi = np.full(n, lo0 - widen), np.full(n, hi0 + widen)
    j = np.arange(n)
    for _ in range(2200):
        live = (hi - lo) > 2.0 * U * np.maximum(np.abs(lo), np.abs(hi)) + pivmin
        mid = 0.5 * lo + 0.5 * hi
        live &= (mid > lo) & (mid < hi)
        if not live.any():
            break
        below = sturm_count(d, e2, mid, pivmin) > j
        hi = np.where(live & below, mid, hi)
        lo = np.where(live & ~below, mid, lo)
    lam = 0.5 * lo + 0.5 * hi
    lam[np.maximum(np.abs(lo), np.abs(hi)) <= 8.0 * pivmin] = 0.0
    return lam[::-1].copy()


def eigenvalues(a):
    d, e = tridiagonalize(a)
    return bisect(d, e)
