"""Problems and NumPy mirrors shared by test_prepare_layout_capi.py and test_gpu_prepare_layout.py."""
import numpy as np

from topolow_amd import core, synthetic

SYNTHETIC = [(33, 2, 0.3, 1), (65, 3, 0.5, 2), (257, 5, 0.7, 3), (1000, 3, 0.5, 4), (2049, 5, 0.7, 5)]


def synthetic_matrix(n, dim, missing, seed):
    return synthetic.make_problem(n, latent_dim=dim, missing=missing, seed=seed).dissimilarity


def numpy_sums(values):
    """Per point: sum and count of the non-NA off-diagonal cells along its row and along its column."""
    v = np.array(values, dtype=np.float64)
    np.fill_diagonal(v, np.nan)
    have = ~np.isnan(v)
    z = np.where(have, v, 0.0)
    return z.sum(axis=1), have.sum(axis=1), z.sum(axis=0), have.sum(axis=0)


def sums_flag(values):
    """What create() passes as exact_sums: 1 exact, 0 not exact but no negative / infinite cell, -1 otherwise."""
    v = np.asarray(values, dtype=np.float64)
    v = v[~np.isnan(v)]
    with np.errstate(invalid="ignore"):
        if np.all((v >= 0) & (v < 2.0 ** 20) & (v * 1024 == np.floor(v * 1024))):
            return 1
    return -1 if np.any((v < 0) | np.isinf(v)) else 0


def tied_integers(n=96, seed=11):
    """Integer distances between four groups: points of a group share their key exactly (unless a hole breaks it)."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, n)
    D = np.abs(g[:, None] - g[None, :]).astype(np.float64) * 3.0
    holes = rng.random((n, n)) < 0.002
    holes = np.triu(holes, 1)
    D[holes | holes.T] = np.nan
    return D


def same_values_other_columns(n=12, seed=5):
    """Rows 0 and 1 hold the same non-dyadic values in opposite column order: their keys agree to rounding."""
    rng = np.random.default_rng(seed)
    D = rng.uniform(0.1, 3.0, (n, n))
    D = (D + D.T) / 2
    w = rng.uniform(0.1, 3.0, n - 2)
    D[0, 2:] = D[2:, 0] = w
    D[1, 2:] = D[2:, 1] = w[::-1]
    D[0, 1] = D[1, 0] = 0.7
    np.fill_diagonal(D, 0.0)
    return D


def one_negative(n=33):
    D = synthetic_matrix(n, 2, 0.3, 1).copy()
    D[2, 5] = -0.3
    return D


def single_positive_key():
    D = np.zeros((4, 4))
    D[1, :] = np.nan
    D[0, 1] = 2.0
    return D


def no_positive_key():
    D = np.zeros((5, 5))
    D[0, 3] = D[3, 0] = np.nan
    return D


def unmeasured_point(n=40, at=7):
    D = synthetic_matrix(n, 2, 0.3, 9).copy()
    D[at, :] = np.nan
    D[:, at] = np.nan
    return D


def asymmetric_na(n=70, seed=3):
    rng = np.random.default_rng(seed)
    D = synthetic_matrix(n, 3, 0.2, 6).copy()
    D[rng.random((n, n)) < 0.15] = np.nan     # holes on one side only
    return D


def with_codes(n=130, seed=8):
    """10 % ">" and 5 % "<" cells, symmetric like a parsed titer table, some of them on NA cells of the values."""
    rng = np.random.default_rng(seed)
    D = synthetic_matrix(n, 3, 0.4, 7).copy()
    u = np.triu(rng.random((n, n)), 1)
    u = u + u.T
    codes = np.zeros((n, n), dtype=np.int8)
    codes[(u > 0) & (u < 0.10)] = 1
    codes[(u >= 0.10) & (u < 0.15)] = -1
    return core.CodedMatrix(D, codes, ["p%d" % q for q in range(n)], True)


def quickstart():
    pts = np.array([[0, 0], [3, 0], [4, 4], [2, 2], [0, 4]], dtype=float)
    D = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1))
    D[3, 4] = D[4, 3] = np.nan
    return D
