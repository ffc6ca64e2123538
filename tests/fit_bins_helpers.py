"""What tests/test_gpu_fit_bins.py shares with tests/test_gpu_fit_report.py, as copies (that file is left as it is): the
noisy test matrix, the hold-out mask and the host's view of what the fit kernels read."""
import numpy as np


def matrix(n, seed, codes=True, symmetric=True, special=True):
    """values (NaN = NA; a few +-Inf cells, zeros on the diagonal) and codes (or None) of a noisy distance matrix."""
    rng = np.random.default_rng(seed)
    pts = rng.normal(size=(n, 3))
    d = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1)) * (1.0 + 0.3 * rng.normal(size=(n, n)))
    d = np.abs(np.triu(d, 1))
    d = d + d.T
    hole = np.triu(rng.random((n, n)) < 0.4, 1)
    d[hole | hole.T] = np.nan
    cds = None
    if codes:
        u = np.triu(rng.random((n, n)), 1)
        u = u + u.T
        cds = np.zeros((n, n), dtype=np.int8)
        cds[(u > 0) & (u < 0.10)] = 1
        cds[(u >= 0.10) & (u < 0.15)] = -1
    if special and n >= 8:
        d[1, 3] = d[3, 1] = np.inf
        d[2, 6] = d[6, 2] = -np.inf
        d[4, 4] = np.nan
        d[5, 5] = 1.25
    if not symmetric:
        d[np.tril_indices(n, -1)] = np.nan        # cells in one triangle only
    return d, cds


def held_mask(n, picks):
    held = np.zeros((n, n), dtype=bool)
    if picks is not None and len(picks):
        p = np.asarray(picks, dtype=np.int64)
        held[p % n, p // n] = True
        held |= held.T
    return held


def picks_of(kind, n, seed):
    if kind == "none":
        return None
    if kind == "all":
        return np.arange(n * n, dtype=np.int64)
    return np.random.default_rng(seed).choice(n * n, max(1, n * n // 10), replace=False).astype(np.int64)


def host_view(h, values, codes, picks, pos):
    """What the device reads, in BUFFER coordinates: v, code, held per cell (a, b) of the ordered matrix as the handle's
    lines hold it, and est from the handle's own post-metrics pass."""
    n = h.n
    cds = np.zeros((n, n), dtype=np.int8) if codes is None else codes
    held = held_mask(n, picks)
    o = h.order
    if o is not None:
        ix = np.ix_(o, o)
        values, cds, held = values[ix], cds[ix], held[ix]
    if h.layout == "F":                              # a line is a column
        values, cds = values.T, cds.T
    est, _, _ = h.post_metrics(pos)
    fin = np.isfinite(values)
    member = {"in": fin & (cds == 0) & ~held, "out": fin & (cds == 0) & held, "all": fin}
    return values, est, member


def axes_of(v, est, mask):
    """The four quantities of the cells of one series, as the device forms them."""
    vv, rr = v[mask], est[mask]
    return {"true": vv, "predicted": rr, "error": vv - rr, "residual": rr - vv}
