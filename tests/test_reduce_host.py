"""topolow_amd/reduce.py on the host: pca_scores against the definitions of prcomp, Brent's fmin and the scale against
the exact minimiser, temporal_map_data against a line-by-line recomputation.

The scale test stands in for a comparison against R.  F(s) = sum_ij |d_ij - s r_ij| = sum_ij r_ij |d_ij / r_ij - s| is
convex and piecewise linear, so its exact minimiser is the weighted median of d_ij / r_ij with weights r_ij (pairs
with r_ij = 0 add a constant): computed here by sort and cumulative sum.  Brent's guarantee is |s - s*| <= 3 tol1 with
tol1 = sqrt(eps) |s| + tol / 3; measured on the three maps below: 0.35 to 0.73 tol1, 15 to 21 evaluations.  The cap of
64 evaluations is a cap and not a measurement: golden section alone from a width of 40 to 8e-5 takes 27 steps."""
import math

import numpy as np
import pytest

import topolow_amd
from topolow_amd import reduce as rd
from topolow_amd import velocity as vel

EPS = float(np.finfo(np.float64).eps)
TOL = EPS ** 0.25
MAPS = [(65, 3), (300, 5), (1000, 7)]


def make_map(n, ndim, seed=None):
    rng = np.random.default_rng(1000 * n + ndim if seed is None else seed)
    return rng.normal(size=(n, ndim)) * rng.uniform(0.5, 3.0, size=ndim) + rng.normal(size=ndim)


def pair_distances(X):
    iu = np.triu_indices(X.shape[0], 1)
    return np.sqrt(((X[iu[0]] - X[iu[1]]) ** 2).sum(axis=1))


def weighted_median_scale(X, Y):
    """The exact minimiser of F: the weighted median of d / r with weights r, by sort and cumulative sum."""
    d, r = pair_distances(X), pair_distances(Y)
    ok = r > 0
    q, w = d[ok] / r[ok], r[ok]
    order = np.argsort(q, kind="stable")
    cum = np.cumsum(w[order])
    return float(q[order][np.searchsorted(cum, 0.5 * cum[-1])])


def tol1_of(s, tol=TOL):
    return math.sqrt(EPS) * abs(s) + tol / 3


def test_exports_and_config_validation():
    for name in ("DimReductionConfig", "pca_scores", "reduce_dimensions", "scale_to_original_distances",
                 "temporal_map_data"):
        assert name in topolow_amd.__all__ and getattr(topolow_amd, name) is getattr(rd, name)
    c = rd.DimReductionConfig()
    assert (c.method, c.n_components, c.scale, c.center, c.pca_tol, c.rank) == ("pca", 2, True, True, math.sqrt(EPS), None)
    for method in ("umap", "tsne"):
        with pytest.raises(NotImplementedError, match="package"):
            rd.DimReductionConfig(method=method)
    for kw in (dict(method="mds"), dict(n_components=0), dict(n_components=-1), dict(n_components="2"),
               dict(n_components=1.5), dict(scale=1), dict(center="yes"), dict(pca_tol=math.nan), dict(rank=0)):
        with pytest.raises(ValueError):
            rd.DimReductionConfig(**kw)
    assert rd.DimReductionConfig(n_components=3.0).n_components == 3


@pytest.mark.parametrize("n,ndim", MAPS)
def test_pca_scores_are_the_principal_components(n, ndim):
    X = make_map(n, ndim)
    S = rd.pca_scores(X, rd.DimReductionConfig(n_components=ndim))
    assert S.shape == (n, ndim)
    scale = np.abs(S).max()
    assert np.abs(S.mean(axis=0)).max() <= 1e-13 * scale                     # zero mean
    gram = S.T @ S
    off = gram - np.diag(np.diag(gram))
    assert np.abs(off).max() <= 1e-12 * gram[0, 0]                           # mutually orthogonal
    var = S.var(axis=0, ddof=1)
    assert (np.diff(var) < 0).all()                                          # descending
    top = np.sort(np.linalg.eigvalsh(np.cov(X, rowvar=False)))[::-1]
    assert np.abs(var - top).max() <= 1e-12 * top[0]                         # the eigenvalues of the covariance
    assert np.abs(pair_distances(S) - pair_distances(X)).max() <= 1e-12 * pair_distances(X).max()   # a rotation
    two = rd.pca_scores(X)                                                   # the default: the first two of them
    assert np.array_equal(two, S[:, :2])
    assert np.array_equal(rd.pca_scores(X, rd.DimReductionConfig(rank=2)), two)
    with pytest.raises(ValueError, match="remain"):
        rd.pca_scores(X, rd.DimReductionConfig(n_components=3, rank=2))


def test_pca_drops_a_rank_deficient_component():
    rng = np.random.default_rng(3)
    X = rng.normal(size=(40, 3))
    X[:, 2] = X[:, 0]                                                        # rank 2
    assert rd.pca_scores(X).shape == (40, 2)
    with pytest.raises(ValueError, match="2 remain"):
        rd.pca_scores(X, rd.DimReductionConfig(n_components=3))
    assert rd.pca_scores(X, rd.DimReductionConfig(n_components=3, pca_tol=None)).shape == (40, 3)   # tol = NULL keeps it
    X[:, 1] = 2 * X[:, 0]                                                    # rank 1: 2 cannot be served
    with pytest.raises(ValueError, match="1 remain"):
        rd.pca_scores(X)
    with pytest.raises(ValueError):
        rd.pca_scores(np.array([[1.0, np.nan], [0.0, 1.0], [2.0, 2.0]]))


def test_brent_fmin_on_known_functions():
    x, fx, trace = rd.brent_fmin(lambda s: (s - 2.0) ** 2 + 1.0, 0.01, 40.0, TOL)
    assert abs(x - 2.0) <= 3 * tol1_of(x) and fx == min(f for _, f in trace) and len(trace) <= 64
    assert trace[0][0] == 0.01 + 0.5 * (3 - math.sqrt(5)) * (40.0 - 0.01)    # the first point is the golden section
    x, fx, trace = rd.brent_fmin(lambda s: abs(s - 7.25), 0.01, 40.0, 1e-8)
    assert abs(x - 7.25) <= 3 * tol1_of(x, 1e-8) and len(trace) <= 64
    for bad in ((1.0, 1.0, TOL), (2.0, 1.0, TOL), (0.0, 1.0, 0.0), (0.0, math.inf, TOL), (0.0, 1.0, math.nan)):
        with pytest.raises(ValueError):
            rd.brent_fmin(abs, *bad)


@pytest.mark.parametrize("n,ndim", MAPS)
def test_scale_is_within_brents_band_of_the_weighted_median(n, ndim):
    X = make_map(n, ndim)
    Y = rd.pca_scores(X)
    scaled, s, info = rd.scale_to_original_distances(Y, positions=X)
    exact = weighted_median_scale(X, Y)
    print(f"n={n} ndim={ndim}: scale {s:.10f}, weighted median {exact:.10f}, |diff| = {abs(s - exact) / tol1_of(s):.3f} tol1, "
          f"{info['evaluations']} evaluations")
    assert abs(s - exact) <= 3 * tol1_of(s)
    assert info["evaluations"] <= 64 and info["trace"].shape == (info["evaluations"], 2)
    assert info["objective"] == info["trace"][:, 1].min()
    assert np.array_equal(scaled, Y * s)
    # the objective is the reference's: the sum over the full matrices
    D, R = rd.distance_matrix(X), rd.distance_matrix(Y)
    assert info["objective"] == np.abs(D - R * s).sum()
    assert np.abs(D[np.triu_indices(n, 1)] - pair_distances(X)).max() <= 4 * EPS * D.max()
    # from orig_dist the same steps, bit for bit
    _, s2, info2 = rd.scale_to_original_distances(Y, orig_dist=D)
    assert s2 == s and np.array_equal(info2["trace"], info["trace"])
    # k = ndim: the scores are a rotation of the map and the scale is 1
    full = rd.pca_scores(X, rd.DimReductionConfig(n_components=ndim))
    _, s1, info1 = rd.scale_to_original_distances(full, positions=X)
    assert abs(s1 - 1.0) <= 3 * tol1_of(s1) and info1["evaluations"] <= 64
    # reduce_dimensions: the scaled scores, and the bare ones with scale = False
    assert np.array_equal(rd.reduce_dimensions(X), scaled)
    assert np.array_equal(rd.reduce_dimensions(X, rd.DimReductionConfig(scale=False)), Y)


def test_scale_argument_errors():
    X = make_map(20, 3)
    Y = rd.pca_scores(X)
    with pytest.raises(ValueError):
        rd.scale_to_original_distances(Y)                                   # neither positions nor orig_dist
    with pytest.raises(ValueError):
        rd.scale_to_original_distances(Y, orig_dist=np.zeros((19, 19)))
    with pytest.raises(ValueError):
        rd.scale_to_original_distances(Y, positions=X, interval=(1.0, 1.0))
    with pytest.raises(ValueError):
        rd.scale_to_original_distances(Y, positions=X, tol=0.0)
    with pytest.raises(ValueError):
        rd.scale_to_original_distances(Y, device=0)                         # the device form needs positions
    with pytest.raises(ValueError):
        rd.scale_to_original_distances(Y, positions=X, orig_dist=rd.distance_matrix(X), device=0)
    bad = X.copy()
    bad[3, 1] = np.inf
    with pytest.raises(ValueError):
        rd.scale_to_original_distances(Y, positions=bad)


def test_temporal_map_data_line_by_line():
    n, ndim = 120, 4
    rng = np.random.default_rng(8)
    X = make_map(n, ndim, seed=8)
    t = rng.integers(2000, 2012, size=n).astype(float)
    names = ["S%03d" % i for i in range(n)]
    tree = [names[i] for i in range(n) if i % 4]
    clades = {names[i]: [names[j] for j in range(n) if (i + j) % 3] for i in range(0, n, 2)}
    clade = dict(names=names, clade_members=clades, tree_present_points=tree)
    out = rd.temporal_map_data(X, t, **clade)

    Y = rd.pca_scores(X)
    scaled, s, _ = rd.scale_to_original_distances(Y, positions=X)
    assert np.array_equal(out["reduced"], scaled)
    plot_x, plot_y = scaled[:, 1] * 1, scaled[:, 0] * 1
    assert np.array_equal(out["plot_x"], plot_x) and np.array_equal(out["plot_y"], plot_y)
    sigma_t = vel.pair_difference_bandwidth(t)
    sigma_x = math.sqrt(0.5 * (vel.silverman_bandwidth(plot_x) ** 2 + vel.silverman_bandwidth(plot_y) ** 2))
    sigma_x_nd = math.sqrt(np.mean([vel.silverman_bandwidth(X[:, d]) ** 2 for d in range(ndim)]))
    assert (out["sigma_t"], out["sigma_x"], out["sigma_x_nd"]) == (sigma_t, sigma_x, sigma_x_nd)
    assert out["sigma_x_nd"] == vel.default_bandwidths(X, t)[0] and out["sigma_t"] == vel.default_bandwidths(X, t)[1]
    V, mag, _ = vel.kernel_velocity(X, t, sigma_t, sigma_x_nd, **clade)
    P, pmag, _ = vel.kernel_velocity(np.column_stack([plot_x, plot_y]), t, sigma_t, sigma_x, **clade)
    assert np.array_equal(out["velocity"], V, equal_nan=True)
    assert np.array_equal(out["velocity_magnitude"], mag, equal_nan=True)
    assert np.array_equal(out["v_plot_x"], P[:, 0], equal_nan=True) and np.array_equal(out["v_plot_y"], P[:, 1], equal_nan=True)
    assert np.array_equal(out["plot_velocity_magnitude"], pmag, equal_nan=True)
    assert np.array_equal(out["arrows"], np.flatnonzero(pmag >= 0.1))
    assert 0 < out["arrows"].size < n and np.isnan(pmag).any()               # the threshold and the NaN rows both bite

    # the reverse flags flip the plot columns (and with them the plot velocities), nothing else
    flipped = rd.temporal_map_data(X, t, reverse_x=-1, reverse_y=-1, **clade)
    assert np.array_equal(flipped["plot_x"], -out["plot_x"]) and np.array_equal(flipped["plot_y"], -out["plot_y"])
    assert np.array_equal(flipped["reduced"], out["reduced"])
    assert np.array_equal(flipped["velocity"], out["velocity"], equal_nan=True)
    assert np.array_equal(flipped["v_plot_x"], -out["v_plot_x"], equal_nan=True)
    assert np.array_equal(flipped["arrows"], out["arrows"]) and flipped["sigma_x"] == out["sigma_x"]
    one = rd.temporal_map_data(X, t, reverse_x=-1, **clade)
    assert np.array_equal(one["plot_x"], -out["plot_x"]) and np.array_equal(one["plot_y"], out["plot_y"])

    # given bandwidths are taken as they are; another threshold selects other arrows
    given = rd.temporal_map_data(X, t, sigma_t=2.0, sigma_x=0.7, sigma_x_nd=0.9, arrow_plot_threshold=0.0, **clade)
    assert (given["sigma_t"], given["sigma_x"], given["sigma_x_nd"]) == (2.0, 0.7, 0.9)
    assert np.array_equal(given["arrows"], np.flatnonzero(~np.isnan(given["plot_velocity_magnitude"])))
    with pytest.raises(ValueError):
        rd.temporal_map_data(X, t, config=rd.DimReductionConfig(n_components=1))
    with pytest.raises(ValueError):
        rd.temporal_map_data(X, t[:-1])
