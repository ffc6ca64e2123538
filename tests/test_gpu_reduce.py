"""topolow_scale_objective and topolow_scale_to_original_distances on the device (csrc/relax_reduce.h) against NumPy,
and the device forms of topolow_amd/reduce.py against its host forms.

The kernel's widths: a tile of 64 columns, 256 rows per workgroup, units of 256 columns (the library's width up to
16 384 points; 64, 128, 256 and 512 through the _ex entry), the triangle j < i cut into a list of units.

Band of the objective: |F_dev - F_host| <= 1e-12 (G + s H), relative to G + s H and not to F, which cancels to about 0
at k = ndim, s = 1.  Per pair d carries at most ndim + 2 roundings and s r at most k + 3, the subtraction one (the
kernel fuses the product into it, the host does not: one rounding more on the host's side, counted): at most
2^-53 (2 * 16 + 6) = 4.2e-15 relative to d + s r.  Fixed-order adds stay below n 2^-53 = 8.6e-14 at n = 770, and the
host's sums are math.fsum over the pairs, exact to one rounding.  G and H are held to 1e-12 relative.  A skipped or
doubled pair moves a sum by about 2 / n^2 relative (3.4e-6 at n = 770), far outside the band: the coordinates have
distinct magnitudes per column, duplicate points (r = d = 0) and one far outlier, so no two pairs' terms are alike.

Scale: Brent's guarantee |s - s*| <= 3 tol1, tol1 = sqrt(eps) |s| + tol / 3, against the exact minimiser (the weighted
median of d / r with weights r, tests/test_reduce_host.py); the host form carries the same guarantee, so the two
forms are within 6 tol1 of each other."""
import math

import numpy as np
import pytest

from topolow_amd import _native
from topolow_amd import reduce as rd
from topolow_amd import velocity as vel
from tests.test_gpu_velocity import host as velocity_host, in_band as velocity_in_band
from tests.test_reduce_host import TOL, make_map, tol1_of, weighted_median_scale

pytestmark = pytest.mark.gpu

SCALES = np.array([0.01, 0.05, 0.3, 1.0, 1.7, 5.0, 13.0, 40.0])
CHUNKS = [None, 64, 128, 256, 512]                                # every width the _ex entry accepts
SIZES = [2, 3, 63, 64, 65, 255, 256, 257, 770]
DIMS = [1, 2, 5, 16]


def make_pair(n, ndim, k):
    """X: normal columns of distinct magnitudes, three duplicates of earlier points (one across the 64-column and one
    across the 256-row boundary where n allows) and one far outlier.  Y: X rotated by a random orthogonal matrix and
    cut to k columns -- a rotation of the map at k = ndim (F(1) cancels to roundings), shrunk by 0.8 otherwise."""
    rng = np.random.default_rng(7919 * n + 31 * ndim)
    X = rng.normal(size=(n, ndim)) * (1.0 + np.arange(ndim)) + 0.1 * np.arange(ndim)
    if n >= 63:
        X[n - 1] = X[0]
        X[62] = X[5]
        X[n // 2] = X[n // 2 - 1]
        X[7] = 1000.0 + np.arange(ndim)                           # the outlier
    Q, _ = np.linalg.qr(np.random.default_rng(ndim).normal(size=(ndim, ndim)))
    Y = X @ Q[:, :k]
    return X, (Y if k == ndim else 0.8 * Y)


_REFERENCE = {}


def reference(n, ndim, k):
    """(X, Y, F over SCALES, G, H) from NumPy: the pair distances once, every sum by math.fsum.  Computed once per
    case and shared; nothing writes to it."""
    key = (n, ndim, k)
    if key not in _REFERENCE:
        X, Y = make_pair(n, ndim, k)
        iu = np.triu_indices(n, 1)
        d = np.sqrt(((X[iu[0]] - X[iu[1]]) ** 2).sum(axis=1))
        r = np.sqrt(((Y[iu[0]] - Y[iu[1]]) ** 2).sum(axis=1))
        F = np.array([2.0 * math.fsum(np.abs(d - s * r)) for s in SCALES])
        _REFERENCE[key] = (X, Y, F, 2.0 * math.fsum(d), 2.0 * math.fsum(r), d, r)
    return _REFERENCE[key]


def host_objective(d, r, s):
    return 2.0 * math.fsum(np.abs(d - s * r))


def check_band(Fd, Gd, Hd, F, G, H, scales, label):
    band = 1e-12 * (G + scales * H)
    worst = float((np.abs(Fd - F) / band).max())
    print(f"{label}: max |dF| / band {worst:.2e}, |dG|/G {abs(Gd - G) / G:.2e}, |dH|/H {abs(Hd - H) / H:.2e}")
    assert (np.abs(Fd - F) <= band).all(), label
    assert abs(Gd - G) <= 1e-12 * G and abs(Hd - H) <= 1e-12 * H, label


@pytest.mark.parametrize("ndim", DIMS)
@pytest.mark.parametrize("n", SIZES)
def test_objective_against_numpy(n, ndim):
    for k in sorted({1, min(2, ndim), ndim}):
        X, Y, F, G, H, _, _ = reference(n, ndim, k)
        for chunk in CHUNKS:
            Fd, Gd, Hd = _native.scale_objective(X, Y, SCALES, chunk_cols=chunk)                     # m = 8
            check_band(Fd, Gd, Hd, F, G, H, SCALES, f"n={n} ndim={ndim} k={k} chunk={chunk} m=8")
            for q in (0, 3, 7):                                                                      # m = 1
                F1, G1, H1 = _native.scale_objective(X, Y, SCALES[q], chunk_cols=chunk)
                check_band(F1, G1, H1, F[q:q + 1], G, H, SCALES[q:q + 1], f"n={n} ndim={ndim} k={k} chunk={chunk} s={SCALES[q]}")
        if k == ndim and n >= 63:
            assert F[3] <= 1e-9 * G                                  # the case the band is written for: F(1) cancels


@pytest.mark.parametrize("n,ndim,k,m", [(300, 11, 3, 3), (130, 13, 13, 5), (200, 12, 2, 2), (257, 7, 6, 7), (65, 16, 3, 4),
                                        (129, 9, 1, 6)])
def test_padded_dimensions_and_scale_counts(n, ndim, k, m):
    """ndim 11 runs as 12 and 13 as 16, k > 2 with as many reduced coordinates as the positions, m = 2..7 as 8."""
    X, Y, F, G, H, _, _ = reference(n, ndim, k)
    for chunk in (None, 64):
        Fd, Gd, Hd = _native.scale_objective(X, Y, SCALES[:m], chunk_cols=chunk)
        assert Fd.shape == (m,)
        check_band(Fd, Gd, Hd, F[:m], G, H, SCALES[:m], f"n={n} ndim={ndim} k={k} m={m} chunk={chunk}")


@pytest.mark.parametrize("n,ndim,k", [(770, 5, 2), (257, 16, 16), (65, 2, 1), (600, 3, 3)])
def test_same_bits_on_repeated_calls_and_for_any_m(n, ndim, k):
    X, Y, F, G, H, _, _ = reference(n, ndim, k)
    for chunk in CHUNKS:
        first = _native.scale_objective(X, Y, SCALES, chunk_cols=chunk)
        again = _native.scale_objective(X, Y, SCALES, chunk_cols=chunk)
        assert np.array_equal(first[0], again[0]) and first[1:] == again[1:], chunk
        for q, s in enumerate(SCALES):                               # the m = 8 call is eight m = 1 calls, bit for bit
            one = _native.scale_objective(X, Y, s, chunk_cols=chunk)
            assert one[0][0] == first[0][q] and one[1:] == first[1:], (chunk, q)
        some = _native.scale_objective(X, Y, SCALES[2:5], chunk_cols=chunk)
        assert np.array_equal(some[0], first[0][2:5]) and some[1:] == first[1:], chunk
    plain = _native.scale_objective(X, Y, SCALES)                    # the library's width is 256 columns at these sizes
    wide = _native.scale_objective(X, Y, SCALES, chunk_cols=256)
    assert np.array_equal(plain[0], wide[0]) and plain[1:] == wide[1:]


@pytest.mark.parametrize("n,ndim", [(65, 3), (300, 5), (770, 7)])
def test_minimiser_against_the_weighted_median_and_the_host_form(n, ndim):
    X = make_map(n, ndim)
    Y = rd.pca_scores(X)
    s, objective, evaluations, trace = _native.scale_to_original_distances(X, Y, trace_len=64)
    iu = np.triu_indices(n, 1)
    d = np.sqrt(((X[iu[0]] - X[iu[1]]) ** 2).sum(axis=1))
    r = np.sqrt(((Y[iu[0]] - Y[iu[1]]) ** 2).sum(axis=1))
    G, H = 2.0 * math.fsum(d), 2.0 * math.fsum(r)
    assert evaluations <= 64 and trace.shape == (evaluations, 2)
    for ts, tf in trace:                                             # every evaluation is the objective at its scale
        assert 0.01 <= ts <= 40.0
        assert abs(tf - host_objective(d, r, ts)) <= 1e-12 * (G + ts * H), (ts, tf)
    assert objective == trace[:, 1].min() and s == trace[np.argmin(trace[:, 1]), 0]
    exact = weighted_median_scale(X, Y)
    _, s_host, info = rd.scale_to_original_distances(Y, positions=X)
    print(f"n={n} ndim={ndim}: device {s:.10f} ({evaluations} evaluations), host {s_host:.10f} ({info['evaluations']}), "
          f"weighted median {exact:.10f}: |device - median| = {abs(s - exact) / tol1_of(s):.3f} tol1, "
          f"|device - host| = {abs(s - s_host) / tol1_of(s):.3f} tol1")
    assert abs(s - exact) <= 3 * tol1_of(s)
    assert abs(s - s_host) <= 6 * tol1_of(s)
    # a short trace keeps the first pairs and still counts every evaluation
    s2, objective2, evaluations2, trace2 = _native.scale_to_original_distances(X, Y, trace_len=5)
    assert (s2, objective2, evaluations2) == (s, objective, evaluations) and np.array_equal(trace2, trace[:5])
    assert _native.scale_to_original_distances(X, Y)[:3] == (s, objective, evaluations)
    # k = ndim: the scores are a rotation of the map
    full = rd.pca_scores(X, rd.DimReductionConfig(n_components=ndim))
    s1, _, evaluations1, _ = _native.scale_to_original_distances(X, full)
    assert abs(s1 - 1.0) <= 3 * tol1_of(s1) and evaluations1 <= 64
    # other bounds and another tol reach the library
    s3, _, evaluations3, trace3 = _native.scale_to_original_distances(X, Y, lower=0.5, upper=4.0, tol=1e-6, trace_len=64)
    assert abs(s3 - exact) <= 3 * tol1_of(s3, 1e-6) and evaluations3 <= 64
    assert trace3[0, 0] == 0.5 + 0.5 * (3 - math.sqrt(5)) * 3.5


def test_reduce_dimensions_device_against_host():
    X = make_map(300, 5)
    bare = rd.DimReductionConfig(scale=False)
    assert np.array_equal(rd.reduce_dimensions(X, bare, device=0), rd.reduce_dimensions(X, bare))   # host code both
    Y = rd.pca_scores(X)
    host, dev = rd.reduce_dimensions(X), rd.reduce_dimensions(X, device=0)
    scaled, s, info = rd.scale_to_original_distances(Y, positions=X, device=0)
    assert np.array_equal(dev, scaled) and np.array_equal(dev, Y * s)
    assert info["evaluations"] <= 64 and info["objective"] == info["trace"][:, 1].min()
    assert (np.abs(dev - host) <= 6 * tol1_of(s) * np.abs(Y)).all()
    three = rd.DimReductionConfig(n_components=3)
    assert (np.abs(rd.reduce_dimensions(X, three, device=0) - rd.reduce_dimensions(X, three))
            <= 6 * tol1_of(s) * np.abs(rd.pca_scores(X, three))).all()


def test_temporal_map_data_device_against_host():
    """n = 257, ndim 5, a clade dictionary, bandwidths given so that every summed exponent stays below 40 (the range
    the velocity bands are derived for; the defaults are compared on their own first).

    The n-D pass has the same inputs in both forms and is held to the bands of tests/test_gpu_velocity.py directly.
    The plot pass has not: the two forms' scales are two runs of Brent's fmin and agree within 6 tol1, about 2.5e-4
    relative, which moves every plot position and through the weights every plot velocity by far more than a
    rounding band.  So the plot columns are held to the scale band, and the plot velocities to the velocity bands
    against the host kernel_velocity of the device form's own plot columns; the arrow threshold is placed in the
    widest gap of those host magnitudes, which must exceed the band a thousand times."""
    n, ndim = 257, 5
    rng = np.random.default_rng(11)
    X = rng.normal(size=(n, ndim)) * np.array([1.6, 1.3, 1.0, 0.8, 0.6])
    t = rng.integers(2000, 2016, size=n).astype(float)
    names = ["S%03d" % i for i in range(n)]
    tree = [names[i] for i in range(n) if i % 5]
    clades = {names[i]: [names[j] for j in range(n) if (i + j) % 3] for i in range(0, n, 2)}
    clade = dict(names=names, clade_members=clades, tree_present_points=tree)
    excluded = vel.exclusion_matrix(names, clades, tree)

    # default bandwidths: host code on both sides; the plot bandwidth follows the scale
    h0, d0 = rd.temporal_map_data(X, t, **clade), rd.temporal_map_data(X, t, device=0, **clade)
    assert d0["sigma_t"] == h0["sigma_t"] and d0["sigma_x_nd"] == h0["sigma_x_nd"]
    Y = rd.pca_scores(X)
    s_host, s_dev = h0["reduced"][0, 0] / Y[0, 0], d0["reduced"][0, 0] / Y[0, 0]
    assert abs(s_dev - s_host) <= 6 * tol1_of(s_dev)
    assert abs(d0["sigma_x"] / h0["sigma_x"] - s_dev / s_host) <= 1e-12

    given = dict(sigma_t=3.0, sigma_x=2.0, sigma_x_nd=2.0)
    h, d = rd.temporal_map_data(X, t, **given, **clade), rd.temporal_map_data(X, t, device=0, **given, **clade)
    assert (np.abs(d["reduced"] - h["reduced"]) <= 6 * tol1_of(s_dev) * np.abs(Y)).all()
    assert np.array_equal(d["plot_x"], d["reduced"][:, 1]) and np.array_equal(d["plot_y"], d["reduced"][:, 0])
    # the n-D pass against the host form
    V, W, A, emax = velocity_host(X, t, excluded, 3.0, 2.0)
    assert np.array_equal(V, h["velocity"], equal_nan=True)
    Wd = _native.kernel_velocity(X, t, 3.0, 2.0, vel.pack_exclusion_bits(excluded), device=0)[1]
    velocity_in_band(d["velocity"], Wd, V, W, A, emax, label="n-D pass")
    # the plot pass against the host velocity of the same plot columns
    P = np.column_stack([d["plot_x"], d["plot_y"]])
    Vp, Wp, Ap, emaxp = velocity_host(P, t, excluded, 3.0, 2.0)
    Wpd = _native.kernel_velocity(P, t, 3.0, 2.0, vel.pack_exclusion_bits(excluded), device=0)[1]
    velocity_in_band(np.column_stack([d["v_plot_x"], d["v_plot_y"]]), Wpd, Vp, Wp, Ap, emaxp, label="plot pass")
    ok = Wp > 0
    mag = np.sqrt((Vp ** 2).sum(axis=1))
    assert np.array_equal(np.isnan(d["plot_velocity_magnitude"]), np.isnan(mag))
    tolV = 1e-12 * (Ap[ok] / Wp[ok, None] + np.abs(Vp[ok]))
    band = (np.sqrt((tolV ** 2).sum(axis=1)) + 8 * np.spacing(mag[ok])).max()
    assert (np.abs(d["plot_velocity_magnitude"][ok] - mag[ok]) <= band).all()
    # arrows: a threshold in the widest gap of the middle half of the magnitudes
    srt = np.sort(mag[ok])
    mid = srt[srt.size // 4: 3 * srt.size // 4]
    g = int(np.argmax(np.diff(mid)))
    threshold = float(0.5 * (mid[g] + mid[g + 1]))
    assert 0.5 * (mid[g + 1] - mid[g]) > 1000 * band
    arrows = rd.temporal_map_data(X, t, device=0, arrow_plot_threshold=threshold, **given, **clade)["arrows"]
    assert np.array_equal(arrows, np.flatnonzero(mag >= threshold)) and 0 < arrows.size < ok.sum()


def test_timing_entry_and_unsupported_ndim():
    X = np.ones((8, 17)) * np.arange(8.0)[:, None]
    with pytest.raises(_native.NativeError) as e:
        _native.scale_objective(X, X[:, :2], [1.0])
    assert e.value.code == _native.ERR_UNSUPPORTED
    with pytest.raises(_native.NativeError) as e:
        rd.scale_to_original_distances(X[:, :2], positions=X, device=0)
    assert e.value.code == _native.ERR_UNSUPPORTED
    secs = []
    _native.scale_objective(X[:, :3], X[:, :2], [1.0], timing=secs)
    assert len(secs) == 1 and 0.0 < secs[0] < float("inf")
