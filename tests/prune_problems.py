"""Small matrices for the pruning tests (tests/test_prune_host.py, tests/test_gpu_prune.py), each with a structure
whose pruning can be worked out by hand, and a brute-force recount to hold the host form against."""
import numpy as np


def empty(n):
    D = np.full((n, n), np.nan)
    np.fill_diagonal(D, 0.0)
    return D


def link(D, a, b, value=None):
    D[a, b] = D[b, a] = (1.0 + abs(a - b) * 0.25) if value is None else value


def add_clique(D, nodes):
    for a in nodes:
        for b in nodes:
            if a < b:
                link(D, a, b)


def add_circulant(D, nodes, steps):
    """Every node linked to the nodes `s` places on, for s in steps: degree 2 * len(steps) (steps < len(nodes) / 2)."""
    k = len(nodes)
    for q in range(k):
        for s in steps:
            link(D, nodes[q], nodes[(q + s) % k])


def clique_path(clique=6, path=5):
    """A clique on 0 .. clique-1 with a path clique, clique+1, ... hung on point 0.  At min_connections = 2 one path
    point leaves per round, from the far end: `path` rounds of removal, then the round that finds nothing."""
    D = empty(clique + path)
    add_clique(D, list(range(clique)))
    prev = 0
    for k in range(clique, clique + path):
        link(D, prev, k, 2.5)
        prev = k
    return D


def shuffled(D, seed):
    """D with its points relabelled at random: (matrix, perm) with matrix[a, b] = D[perm[a], perm[b]]."""
    perm = np.random.default_rng(seed).permutation(D.shape[0])
    return np.ascontiguousarray(D[np.ix_(perm, perm)]), perm


def layered(core="clique"):
    """Three disconnected layers: a core on 0..11 (a clique, degree 11, or a circulant of degree 8), a circulant of
    degree 4 on 12..31 and one of degree 6 on 32..51.  Threshold 4 keeps all 52, 6 drops the first circulant, 8 both."""
    D = empty(52)
    if core == "clique":
        add_clique(D, list(range(12)))
    else:
        add_circulant(D, list(range(12)), (1, 2, 3, 4))
    add_circulant(D, list(range(12, 32)), (1, 2))
    add_circulant(D, list(range(32, 52)), (1, 2, 3))
    return D


def regular(n=60, degree=24):
    D = empty(n)
    add_circulant(D, list(range(n)), tuple(range(1, degree // 2 + 1)))
    return D


def upper_only(n):
    """Every cell above the diagonal measured, none below: row i counts n - 1 - i, column counts are the mirror."""
    D = empty(n)
    D[np.triu_indices(n, 1)] = 1.0 + np.arange(n * (n - 1) // 2) * 0.5
    return D


def random_sparse(n, mean_degree, seed, symmetric=True):
    """Random measured pairs with about `mean_degree` per point; symmetric=False measures each direction on its own."""
    rng = np.random.default_rng(seed)
    p = min(1.0, mean_degree / max(n - 1, 1))
    vals = rng.uniform(0.5, 9.5, size=(n, n))
    if symmetric:
        on = np.triu(rng.random((n, n)) < p, 1)
        on = on | on.T
        vals = np.triu(vals, 1) + np.triu(vals, 1).T
    else:
        on = rng.random((n, n)) < p
    D = np.where(on, vals, np.nan)
    np.fill_diagonal(D, 0.0)
    return D


def heavy_tailed(n, seed, scale=3.0):
    """Measured pairs with heavy-tailed degrees: pair (a, b) is measured with probability min(1, w_a w_b / n), w Pareto."""
    rng = np.random.default_rng(seed)
    w = scale * (1.0 + rng.pareto(1.5, size=n))
    on = np.triu(rng.random((n, n)) < np.minimum(1.0, np.outer(w, w) / n), 1)
    on = on | on.T
    vals = np.triu(rng.uniform(0.5, 9.5, size=(n, n)), 1)
    D = np.where(on, vals + vals.T, np.nan)
    np.fill_diagonal(D, 0.0)
    return D


def brute_force(values, min_connections, max_iterations, min_points):
    """The reference's loop with a full recount of the kept submatrix every round (the copy it makes, R/
    data_preprocessing.R:1402): (kept indices, iterations, cells of the kept submatrix)."""
    kept = np.arange(values.shape[0])
    iteration, go_on = 0, True
    while go_on and iteration < max_iterations:
        iteration += 1
        adj = ~np.isnan(values[np.ix_(kept, kept)])
        np.fill_diagonal(adj, False)
        poor = adj.sum(axis=1) < min_connections
        if not poor.any() or len(kept) - int(poor.sum()) < min_points:
            go_on = False
        else:
            kept = kept[~poor]
            if len(kept) == 0:
                break
    adj = ~np.isnan(values[np.ix_(kept, kept)])
    np.fill_diagonal(adj, False)
    return kept, iteration, int(adj.sum())
