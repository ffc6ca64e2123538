"""topolow_kernel_velocity on the device (csrc/relax_velocity.h) against the host form of topolow_amd/velocity.py.

The kernel's widths: a tile of 64 columns (one exclusion word), 256 rows per workgroup, chunks of 256 columns (the
library's width up to 16 384 points; 64 and 128 through the _ex entry).

Band.  Every test asserts on its own inputs that each contributing pair's summed exponent e is <= 40 (normal
points, sigma_x = 2, sigma_t = 3 on years 2000 to 2015 keep it below about 30).  The kernel's arithmetic: x_i - x_j
(one rounding), its square and the running sum (ndim + 1 roundings of d2 at most, fewer where the compiler fuses),
times 1 / (2 sx^2) (the constant carries 1.5 ulp, the product one more); (t_i - t_j)^2 / (2 st^2) likewise 4.5; their
sum one more: e is off by at most (ndim + 6) units of 2^-53 relative, the host's e (two divisions in place of the
reciprocals) by no more, so the two exponents differ by at most 40 (ndim + 6) 2^-52 absolute -- and that is the
relative difference of the weights, plus 4 2^-52 for the exps and the host's product.  The issue's count of
ndim + 3 roundings misses the three of the reciprocal constants; with ndim + 6 the weight band is
(40 (ndim + 6) + 4) 2^-52 = 1.96e-13 at ndim 16, still below 2e-13, so the bounds the issue sets stand unchanged:
fixed-order adds contribute less than n 2^-53 (n <= 770: 8.6e-14), W is held to 1e-12 W, S_d to 1e-12 sum |term|
(taken from the host), and V = S / W to the propagated band 1e-12 (sum |term| / W + |V|).  The device returns V
and W, not S: S is taken as V W, which adds two roundings of S (4.4e-16 sum |term|, 1/2000 of the band).
A needle's single pair gives V = (w / dt) dx / w: four roundings against the one of dx / dt, so 4 ulp."""
import numpy as np
import pytest

from topolow_amd import _native
from topolow_amd import velocity as vel

pytestmark = pytest.mark.gpu

ST, SX = 3.0, 2.0


def host(X, t, excluded=None, st=ST, sx=SX):
    """The host form (topolow_amd.velocity._host_velocity, line for line) that also returns sum |term| per row and
    coordinate and the largest summed exponent of a contributing pair."""
    n, k = X.shape
    V, W, A, emax = np.full((n, k), np.nan), np.zeros(n), np.zeros((n, k)), 0.0
    for i in range(n):
        past = t < t[i]
        if excluded is not None:
            past &= ~excluded[i]
        idx = np.flatnonzero(past)
        if idx.size:
            dt = t[i] - t[idx]
            dX = X[i] - X[idx]
            d2 = (dX ** 2).sum(axis=1)
            w = np.exp(-d2 / (2 * sx ** 2)) * np.exp(-(dt ** 2) / (2 * st ** 2))
            emax = max(emax, float((d2 / (2 * sx ** 2) + dt ** 2 / (2 * st ** 2)).max()))
            W[i] = w.sum()
            A[i] = np.abs(w[:, None] * (dX / dt[:, None])).sum(axis=0)
            if W[i] > 0:
                V[i] = (w[:, None] * (dX / dt[:, None])).sum(axis=0) / W[i]
    Vh, Wh = vel._host_velocity(X, t, st, sx, excluded)
    assert np.array_equal(V, Vh, equal_nan=True) and np.array_equal(W, Wh)
    return V, W, A, emax


def in_band(Vd, Wd, V, W, A, emax, label=""):
    assert emax <= 40.0, emax
    assert np.array_equal(np.isnan(Vd), np.isnan(V)), label
    assert np.array_equal(Wd == 0, W == 0), label
    ok = W > 0
    relW = np.abs(Wd[ok] - W[ok]) / W[ok]
    S, Sd = V[ok] * W[ok, None], Vd[ok] * Wd[ok, None]
    relS = np.abs(Sd - S) / A[ok]
    tolV = 1e-12 * (A[ok] / W[ok, None] + np.abs(V[ok]))
    relV = np.abs(Vd[ok] - V[ok]) / tolV
    if ok.any():
        print(f"{label}: max |dW|/W {relW.max():.2e}, max |dS|/sum|term| {relS.max():.2e}, max |dV|/band {relV.max():.2e}, "
              f"max exponent {emax:.1f}")
    assert (relW <= 1e-12).all(), label
    assert (relS <= 1e-12).all(), label
    assert (relV <= 1.0).all(), label


def make(n, ndim, seed, years=True):
    """Normal points; integer years 2000 to 2015 (many ties) or distinct float times, in no particular order."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, ndim))
    t = rng.integers(2000, 2016, size=n).astype(float) if years else rng.uniform(2000, 2015, size=n)
    return rng, X, t


# n: 1, 2, and one below, at and one above the tile (64), the chunk and the rows of a workgroup (256), and two and three
# chunks; ndim: every instance class (11 runs as 12, 13 as 16)
BAND_CASES = [(1, 2, None), (2, 2, None), (63, 1, None), (64, 2, None), (65, 3, None), (255, 5, None), (256, 10, None),
              (257, 16, None), (511, 2, None), (513, 5, None), (770, 3, None), (300, 11, None), (130, 13, None),
              (127, 5, 64), (128, 2, 64), (129, 10, 64), (127, 3, 128), (128, 16, 128), (129, 1, 128), (300, 4, 128),
              (300, 6, 64), (200, 7, None), (200, 8, 64), (200, 9, 128), (200, 12, None)]


def band_case(n, ndim, chunk, years):
    rng, X, t = make(n, ndim, 100 * n + ndim, years)
    excluded = rng.random((n, n)) < 0.3
    for mask in (None, excluded):
        bits = vel.pack_exclusion_bits(mask) if mask is not None else None
        Vd, Wd = _native.kernel_velocity(X, t, ST, SX, bits, chunk_cols=chunk)
        in_band(Vd, Wd, *host(X, t, mask), label=f"n={n} ndim={ndim} chunk={chunk} years={years} bits={mask is not None}")


@pytest.mark.parametrize("n,ndim,chunk", BAND_CASES)
def test_band_against_the_host_form(n, ndim, chunk):
    band_case(n, ndim, chunk, True)


@pytest.mark.parametrize("n,ndim,chunk", [(257, 5, None), (513, 2, None), (129, 10, 64), (300, 3, 128)])
def test_band_with_distinct_float_times(n, ndim, chunk):
    """No ties: every row but one has a past, the prefix grows by one column per row, and the sort is a real
    permutation of the caller's order."""
    band_case(n, ndim, chunk, False)


def needle_check(X, t, rows, Vd, Wd):
    """rows: {row: needle column or None}.  One pair: V = dx / dt to 4 ulp, W the single weight; None: NaN and 0."""
    for i, j in rows.items():
        if j is None:
            assert np.isnan(Vd[i]).all() and Wd[i] == 0.0, (i, Vd[i], Wd[i])
            continue
        want = (X[i] - X[j]) / (t[i] - t[j])
        assert (np.abs(Vd[i] - want) <= 4 * np.spacing(np.abs(want))).all(), (i, j, Vd[i], want)
        d2, dt = ((X[i] - X[j]) ** 2).sum(), t[i] - t[j]
        e = d2 / (2 * SX ** 2) + dt ** 2 / (2 * ST ** 2)
        assert e <= 40.0
        w = np.exp(-d2 / (2 * SX ** 2)) * np.exp(-(dt ** 2) / (2 * ST ** 2))
        assert abs(Wd[i] - w) <= 1e-12 * w, (i, j, Wd[i], w)


@pytest.mark.parametrize("chunk", [None, 64, 128])
def test_needles_placed_by_exclusion_bits(chunk):
    """770 points of distinct ascending times (the sorted order is the caller's): the last rows have everyone before
    them in their past and bits that exclude all but ONE column -- the first and last column of a tile, of an
    exclusion word (bit 0, bit 63, and the two sides of a word boundary) and of every chunk width, the first column
    of all and the row's last past column."""
    n = 770
    rng = np.random.default_rng(5)
    X = rng.normal(size=(n, 3))
    t = 2000.0 + 0.01 * np.arange(n)
    columns = [767, 513, 512, 511, 257, 256, 255, 192, 191, 128, 127, 65, 64, 63, 62, 1, 0]
    rows = {n - 1 - r: j for r, j in enumerate(columns)}
    rows[n - 1 - len(columns)] = n - 2 - len(columns)            # the row's last past column
    rows[n - 2 - len(columns)] = None                             # every past column excluded
    rows[300] = 299                                               # ... of a row in the second workgroup
    rows[256] = 255
    rows[257] = 256
    excluded = np.zeros((n, n), dtype=bool)
    for i, j in rows.items():
        excluded[i] = True
        if j is not None:
            assert j < i
            excluded[i, j] = False
    Vd, Wd = _native.kernel_velocity(X, t, ST, SX, vel.pack_exclusion_bits(excluded), chunk_cols=chunk)
    needle_check(X, t, rows, Vd, Wd)
    # the complement: ONE column excluded, every other one eligible -- the host form with and without that column
    excluded = np.zeros((n, n), dtype=bool)
    for i, j in rows.items():
        if j is not None:
            excluded[i, j] = True
    Vd, Wd = _native.kernel_velocity(X, t, ST, SX, vel.pack_exclusion_bits(excluded), chunk_cols=chunk)
    V, W, A, emax = host(X, t, excluded)
    in_band(Vd, Wd, V, W, A, emax, label=f"one excluded column, chunk={chunk}")
    _, W0, _, _ = host(X, t)
    some = [i for i, j in rows.items() if j is not None]
    assert (np.abs(W0[some] - W[some]) > 1e-6 * W[some]).all()      # the excluded column's weight shows


@pytest.mark.parametrize("chunk", [None, 64])
def test_needles_placed_by_time(chunk):
    """Ties.  Points 256..260 share one time and so do 513..517: their past ends at sorted column 255 (the last of a
    chunk) and at 512 (the first of one), and the first tied column is sorted column 256 and 513 (the library orders
    tied points by their coordinates, so which point stands there is worked out below).  With every earlier column
    but the last excluded the needle is the last past column.  The NaN rows have every strictly earlier column
    excluded and tied columns CLEAR -- the first tied column alone (rows 260, 517), or every tied and later column
    (row 257): a tied column taken for past would pass its bit, divide by dt = 0 and show in W and V.  Without bits:
    everyone but point 0 tied, so column 0 is every row's single pair."""
    n = 600
    rng = np.random.default_rng(9)
    X = rng.normal(size=(n, 2))
    t = 2000.0 + 0.01 * np.arange(n)
    t[256:261] = t[256]
    t[513:518] = t[513]
    rows = {256: 255, 258: 255, 260: None, 257: None, 513: 512, 515: 512, 517: None, 261: 260, 518: 517}
    first_tied = {g: g + int(np.lexsort((X[g:g + 5, 1], X[g:g + 5, 0]))[0]) for g in (256, 513)}
    excluded = np.zeros((n, n), dtype=bool)
    for i, j in rows.items():
        excluded[i] = True
        if j is not None:
            excluded[i, j] = False
    excluded[260, first_tied[256]] = False
    excluded[517, first_tied[513]] = False
    excluded[257, 256:] = False
    assert not excluded[260, 256:261].all() and excluded[260, :256].all() and excluded[257, :256].all()
    Vd, Wd = _native.kernel_velocity(X, t, ST, SX, vel.pack_exclusion_bits(excluded), chunk_cols=chunk)
    needle_check(X, t, rows, Vd, Wd)
    t2 = np.full(n, 2001.0)
    t2[0] = 2000.0
    Vd, Wd = _native.kernel_velocity(X, t2, ST, SX, chunk_cols=chunk)
    needle_check(X, t2, {i: 0 for i in range(1, n)}, Vd, Wd)
    assert np.isnan(Vd[0]).all() and Wd[0] == 0.0
    # NaN times: nobody's past, no past of their own, wherever the caller lists them
    t3 = t.copy()
    t3[[0, 100, 599]] = np.nan
    Vd, Wd = _native.kernel_velocity(X, t3, ST, SX, chunk_cols=chunk)
    assert np.isnan(Vd[[0, 100, 599]]).all() and (Wd[[0, 100, 599]] == 0).all()
    keep = ~np.isnan(t3)
    Vk, Wk = _native.kernel_velocity(X[keep], t3[keep], ST, SX, chunk_cols=chunk)
    assert np.array_equal(Vd[keep], Vk, equal_nan=True) and np.array_equal(Wd[keep], Wk)
    in_band(Vd, Wd, *host(X, t3), label="NaN times")


def test_underflow_gives_nan_from_both_forms():
    """Row 2's past points are 100 away: exponent 10^4 / 8 = 1250 > 800, every weight 0 in both forms, V NaN.  (No
    test input has a contributing exponent between 700 and 760, where the two forms may differ on an exact 0.)"""
    X = np.array([[0.0, 0.0], [0.5, 0.0], [100.0, 0.0], [100.5, 0.0]])
    t = np.array([2000.0, 2001.0, 2002.0, 2003.0])
    Vd, Wd = _native.kernel_velocity(X, t, ST, SX)
    Vh, Wh = vel._host_velocity(X, t, ST, SX, None)
    assert np.isnan(Vd[2]).all() and np.isnan(Vh[2]).all() and Wd[2] == 0.0 and Wh[2] == 0.0
    assert np.array_equal(np.isnan(Vd), np.isnan(Vh))
    np.testing.assert_allclose(Wd, Wh, rtol=1e-12, atol=0)
    np.testing.assert_allclose(Vd[[1, 3]], Vh[[1, 3]], rtol=1e-12, atol=0)


def test_reproducible_bits():
    """A second call returns the same bits; the library's width is 256 columns at this size (two widths group a
    row's additions differently and are not promised to agree in the last bits: include/topolow_relax.h states the
    width); a shuffled caller order gives the same rows after unshuffling, ties in time and exclusion bits included."""
    n, ndim = 700, 5
    rng, X, t = make(n, ndim, 77)                                 # integer years: many ties
    excluded = rng.random((n, n)) < 0.3
    bits = vel.pack_exclusion_bits(excluded)
    for b in (None, bits):
        V1, W1 = _native.kernel_velocity(X, t, ST, SX, b)
        V2, W2 = _native.kernel_velocity(X, t, ST, SX, b)
        V3, W3 = _native.kernel_velocity(X, t, ST, SX, b, chunk_cols=256)
        assert np.array_equal(V1, V2, equal_nan=True) and np.array_equal(W1, W2)
        assert np.array_equal(V1, V3, equal_nan=True) and np.array_equal(W1, W3)
        V4, W4 = _native.kernel_velocity(X, t, ST, SX, b, chunk_cols=64)
        ok = W1 > 0
        np.testing.assert_allclose(W4[ok], W1[ok], rtol=1e-12, atol=0)
    p = rng.permutation(n)
    for mask in (None, excluded):
        V1, W1 = _native.kernel_velocity(X, t, ST, SX, vel.pack_exclusion_bits(mask) if mask is not None else None)
        shuffled = vel.pack_exclusion_bits(mask[np.ix_(p, p)]) if mask is not None else None
        Vs, Ws = _native.kernel_velocity(X[p], t[p], ST, SX, shuffled)
        assert np.array_equal(Vs, V1[p], equal_nan=True) and np.array_equal(Ws, W1[p])


def test_python_surface_device_against_host():
    """kernel_velocity(device=0) against kernel_velocity(device=None), field for field, with a clade dictionary."""
    n, ndim = 320, 3
    rng, X, t = make(n, ndim, 31)
    names = ["S%03d" % i for i in range(n)]
    tree = [names[i] for i in range(n) if i % 5]
    clades = {names[i]: [names[j] for j in range(n) if (i + j) % 3] for i in range(0, n, 2)}
    args = dict(names=names, clade_members=clades, tree_present_points=tree)
    for kw in ({}, args):
        Vh, mh, Wh = vel.kernel_velocity(X, t, ST, SX, **kw)
        Vd, md, Wd = vel.kernel_velocity(X, t, ST, SX, device=0, **kw)
        excluded = vel.exclusion_matrix(names, clades, tree) if kw else None
        V, W, A, emax = host(X, t, excluded)
        assert np.array_equal(V, Vh, equal_nan=True) and np.array_equal(W, Wh)
        in_band(Vd, Wd, V, W, A, emax, label=f"surface clades={bool(kw)}")
        assert Vd.shape == Vh.shape and md.shape == mh.shape and Wd.shape == Wh.shape
        assert np.array_equal(np.isnan(md), np.isnan(mh))
        ok = W > 0
        tolV = 1e-12 * (A[ok] / W[ok, None] + np.abs(V[ok]))
        # |mag_d - mag_h| <= ||V_d - V_h||, plus the roundings of the magnitude itself (ndim + 2 of them)
        assert (np.abs(md[ok] - mh[ok]) <= np.sqrt((tolV ** 2).sum(axis=1)) + 8 * np.spacing(mh[ok])).all()
    if excluded is not None:
        assert excluded.any() and not np.array_equal(Wh, vel.kernel_velocity(X, t, ST, SX)[2])


def test_timing_entry_and_unsupported_ndim():
    X, t = np.zeros((8, 17)), np.arange(8.0)
    with pytest.raises(_native.NativeError) as e:
        _native.kernel_velocity(X, t, ST, SX)
    assert e.value.code == _native.ERR_UNSUPPORTED
    secs = []
    _native.kernel_velocity(X[:, :2], t, ST, SX, timing=secs)
    assert len(secs) == 1 and 0.0 < secs[0] < float("inf")
