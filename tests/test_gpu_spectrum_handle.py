"""The data assessment of a resident matrix (run with -m gpu): PreparedHandle.spectrum and
spectrum.data_characteristics(handle=) against the host form in NumPy, which is the specification
(topolow_amd/spectrum.py; kernels: topolow_amd/csrc/relax_spectrum.h).

The host quantities of every case are computed once (tests/spectrum_helpers.py) and shared."""
import functools

import numpy as np
import pytest

from topolow_amd import _native, spectrum
from topolow_amd.core import CodedMatrix

from tests.spectrum_helpers import U, eig_tol, handle_cases, host_quantities

pytestmark = pytest.mark.gpu

CASES = handle_cases()


@functools.lru_cache(maxsize=None)
def host(name):
    values, codes = CASES[name]
    return host_quantities(values, codes)


def run(values, codes, layout, **kw):
    with _native.PreparedHandle(values, codes, layout=layout, **kw) as h:
        info, eig, cen = h.spectrum(want_eigenvalues=True, want_centered=True)
        return info, eig, cen, h.declined


def check_against_host(name, info, eig, cen):
    q = host(name)
    n = q["B"].shape[0]
    lam = q["lam"]
    tol = eig_tol(n, lam)
    score, dims, n_pos, n_neg = q["scores"]
    # -- median and counts: exact
    assert info["median"] == q["median"]
    assert info["n_numeric"] == q["n_numeric"] and info["n_filled"] == n * n - q["n_numeric"]
    # -- B on the lower triangle: the means are sums of non-negative terms, chains no longer than 2n + 200 either side
    d2max = float(np.max(q["x"] ** 2))
    low = np.tril_indices(n)
    err_b = float(np.max(np.abs(cen - q["B"])[low]))
    print("%s: B error %.3g (bound %.3g)" % (name, err_b, (2 * n + 200) * U * d2max))
    assert err_b <= (2 * n + 200) * U * d2max
    assert abs(info["trace"] - np.trace(q["B"])) <= n * (2 * n + 200) * U * d2max
    # -- eigenvalues
    err = float(np.max(np.abs(eig - lam)))
    print("%s: n = %d, eigenvalue error / (n u max|lambda|) = %.4f" % (name, n, err / (n * U * np.max(np.abs(lam)))))
    assert eig.shape == (n,) and np.all(np.diff(eig) <= 0)
    assert err <= tol
    # -- the scores
    sum_pos = float(lam[lam > 1e-12].sum())
    assert abs(info["deviation_score"] - score) <= n * tol * (1.0 + score) / sum_pos
    share = np.cumsum(lam[lam > 1e-12]) / sum_pos
    for at in (dims - 2, dims - 1):      # the cumulative shares at dims_90 - 1 and dims_90 (1-based) stand clear of 0.90
        if at >= 0:
            assert abs(share[at] - 0.90) >= 1e-6, (at, share[at])
    assert info["dims_90"] == dims
    borderline = int(np.sum(np.abs(lam) <= tol + 1e-12))
    # B of a symmetric x has one eigenvalue at rounding level (its rows sum to 0); these inputs have no other, and
    # where x is not symmetric the lower triangle alone has none
    assert borderline == (1 if np.array_equal(q["x"], q["x"].T) else 0)
    assert abs(info["n_positive"] - n_pos) <= borderline and abs(info["n_negative"] - n_neg) <= borderline
    assert abs(info["sum_positive"] - sum_pos) <= n * tol
    assert len(info["seconds"]) == 4 and all(s >= 0 for s in info["seconds"])


@pytest.mark.parametrize("name", list(CASES))
def test_case_in_both_layouts(name):
    values, codes = CASES[name]
    got = {}
    for layout in ("C", "F"):
        info, eig, cen, _ = run(values, codes, layout, preserve_order=True)
        check_against_host(name, info, eig, cen)
        got[layout] = (info, eig, cen)
    # the same matrix handed over row-major and column-major: the same bits
    assert np.array_equal(got["C"][1], got["F"][1])
    assert np.array_equal(got["C"][2], got["F"][2])
    for key in ("median", "trace", "deviation_score", "dims_90", "n_positive", "n_negative", "sum_positive"):
        assert got["C"][0][key] == got["F"][0][key], key


def test_the_medians_fall_where_the_cases_say():
    odd, even = host("tied_one_bucket"), host("tied_two_buckets")
    assert odd["n_numeric"] % 2 == 1 and odd["median"] in (1.0, 2.0, 3.0, 4.0, 6.0)
    assert even["n_numeric"] % 2 == 0 and even["median"] == 2.5             # between two levels
    assert host("negative")["x"].min() < 0
    assert host("thresholds")["n_numeric"] < int(np.sum(~np.isnan(CASES["thresholds"][0])))


def test_a_handle_that_declined_its_ordering_serves():
    values, codes = CASES["negative"]
    info, eig, cen, declined = run(values, codes, "C")
    assert declined
    check_against_host("negative", info, eig, cen)


def test_the_handle_s_own_ordering_does_not_show():
    values, codes = CASES["problem200"]
    kept = run(values, codes, "C", preserve_order=True)
    with _native.PreparedHandle(values, codes, order=np.random.default_rng(1).permutation(200)) as h:
        assert h.info["reordered"] and not h.declined
        info, eig, cen = h.spectrum(want_centered=True)
    assert np.array_equal(eig, kept[1]) and np.array_equal(cen, kept[2]) and info["median"] == kept[0]["median"]


def test_shuffled_labels_give_the_same_spectrum():
    values, _ = CASES["problem200"]
    perm = np.random.default_rng(5).permutation(200)
    info, eig, _, _ = run(values[np.ix_(perm, perm)], None, "C", preserve_order=True)
    q = host("problem200")
    assert info["median"] == q["median"]
    assert np.max(np.abs(eig - q["lam"])) <= eig_tol(200, q["lam"])
    assert info["dims_90"] == q["scores"][1]


def test_two_calls_return_the_same_bits_and_fetch_is_unchanged():
    values, codes = CASES["thresholds"]
    with _native.PreparedHandle(values, codes) as h:
        before = h.fetch()
        a = h.spectrum(want_centered=True)
        b = h.spectrum(want_centered=True)
        after = h.fetch()
        res = h.connectivity()
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert {k: v for k, v in a[0].items() if k != "seconds"} == {k: v for k, v in b[0].items() if k != "seconds"}
    for key in ("order", "degrees", "edge_i", "edge_j", "edge_dist", "edge_thresh", "dense", "tdense",
                "values_reordered", "codes_reordered"):
        x, y = getattr(before, key), getattr(after, key)
        assert (x is None and y is None) or np.array_equal(x, y, equal_nan=True), key
    assert before.info == after.info and res[0] >= 1


def test_data_characteristics_with_a_handle():
    values, codes = CASES["thresholds"]
    q = host("thresholds")
    with _native.PreparedHandle(values, codes) as h:
        c = spectrum.data_characteristics(None, handle=h)
    ref = spectrum.data_characteristics(CodedMatrix(values, codes))
    assert c.median == ref.median == q["median"]
    assert np.max(np.abs(c.eigenvalues - ref.eigenvalues)) <= eig_tol(130, ref.eigenvalues)
    assert c.dims_90_percent == ref.dims_90_percent
    assert abs(c.n_positive - ref.n_positive) <= 1 and abs(c.n_negative - ref.n_negative) <= 1
    assert spectrum.adjust_ndim_range((2, 200), c.dims_90_percent) == ((2, c.dims_90_percent + 2), "adjusted")


def test_error_cases():
    D = np.ones((5, 5)) - np.eye(5)
    codes = np.ones((5, 5), dtype=np.int8)
    with _native.PreparedHandle(D, codes, preserve_order=True) as h:          # every cell is a threshold
        with pytest.raises(_native.NativeError, match="infinite or missing values in 'x'.*no numeric cell") as exc:
            h.spectrum()
        assert exc.value.code == _native.ERR_BAD_ARGUMENT
        with pytest.raises(ValueError, match="infinite or missing values in 'x'"):
            spectrum.data_characteristics(None, handle=h)
    D[1, 3] = np.inf
    with _native.PreparedHandle(D, preserve_order=True) as h:
        with pytest.raises(_native.NativeError, match="infinite or missing values in 'x'") as exc:
            h.spectrum()
        assert exc.value.code == _native.ERR_BAD_ARGUMENT
    codes = np.zeros((5, 5), dtype=np.int8)
    codes[1, 3] = 1                                   # the infinite cell as a threshold is filled like any NA
    with _native.PreparedHandle(D, codes, preserve_order=True) as h:
        info, eig, _ = h.spectrum()
    x, median = spectrum.filled_numeric(CodedMatrix(D, codes))
    assert info["median"] == median == 1.0 and info["n_filled"] == 1
    assert np.max(np.abs(eig - np.linalg.eigvalsh(spectrum.centered(x))[::-1])) <= eig_tol(5, eig)
