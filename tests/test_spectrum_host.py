"""The data assessment of Euclidify() (R/core.R:983-1032) on the host: topolow_amd.spectrum's NumPy form -- the
specification of the device form -- on matrices whose spectrum is known in closed form, its median fill, its error
cases, adjust_ndim_range, and the NumPy model of the device's algorithm (tests/models/spectrum_model.py) against
np.linalg.eigvalsh.  No device."""
import numpy as np
import pytest

import topolow_amd
from topolow_amd import spectrum
from topolow_amd.core import CodedMatrix

from tests.models import spectrum_model
from tests.spectrum_helpers import NA, U, dense_tridiagonal, eig_tol, random_symmetric


def test_exported():
    assert topolow_amd.data_characteristics is spectrum.data_characteristics
    assert topolow_amd.adjust_ndim_range is spectrum.adjust_ndim_range


def test_all_off_diagonals_one():
    n = 12
    c = spectrum.data_characteristics(np.ones((n, n)) - np.eye(n))
    assert c.eigenvalues.shape == (n,) and np.all(np.diff(c.eigenvalues) <= 0)
    assert np.allclose(c.eigenvalues[:11], 0.5, rtol=0, atol=eig_tol(n, c.eigenvalues))
    assert abs(c.eigenvalues[11]) <= eig_tol(n, c.eigenvalues)
    assert c.deviation_score == 0.0 and c.n_positive == 11 and c.n_negative == 0
    assert c.dims_90_percent == 10      # 10/11 >= 0.90 > 9/11
    assert c.median == 1.0


def test_four_cycle_metric():
    D = np.array([[0, 1, 2, 1], [1, 0, 1, 2], [2, 1, 0, 1], [1, 2, 1, 0]], dtype=float)
    c = spectrum.data_characteristics(D)
    assert np.allclose(c.eigenvalues, [2.0, 2.0, 0.0, -1.0], rtol=0, atol=eig_tol(4, c.eigenvalues))
    assert abs(c.deviation_score - 0.25) <= 4 * eig_tol(4, c.eigenvalues)
    assert c.dims_90_percent == 2 and (c.n_positive, c.n_negative) == (2, 1)


def test_points_in_three_dimensions():
    n = 60
    X = np.random.default_rng(2).normal(size=(n, 3)) * [3.0, 2.0, 1.0]
    D = np.sqrt(((X[:, None] - X[None]) ** 2).sum(-1))
    c = spectrum.data_characteristics(D)
    sv = np.linalg.svd(X - X.mean(axis=0), compute_uv=False) ** 2
    # D itself carries a rounding error of a few u per cell from the square root: B is off by about 4 u max(D^2)
    tol = eig_tol(n, c.eigenvalues) + 8 * n * U * float(np.max(D * D))
    assert np.allclose(c.eigenvalues[:3], sv, rtol=0, atol=tol)
    assert np.all(np.abs(c.eigenvalues[3:]) <= tol)
    assert c.deviation_score <= n * tol / float(np.sum(sv))
    assert c.dims_90_percent in (2, 3) and c.dims_90_percent == int(np.nonzero(np.cumsum(sv) / sv.sum() >= 0.9)[0][0]) + 1


def test_median_counts_the_diagonal_and_ignores_thresholds():
    values = np.array([[0.0, 5.0, NA, 9.0],
                       [5.0, 0.0, 7.0, 40.0],
                       [NA, 7.0, 0.0, 80.0],
                       [9.0, 40.0, 80.0, 0.0]])
    codes = np.zeros((4, 4), dtype=np.int8)
    codes[1, 3] = codes[3, 1] = 1         # ">40"
    codes[2, 3] = codes[3, 2] = -1        # "<80"
    x, median = spectrum.filled_numeric(CodedMatrix(values, codes))
    # numeric cells: four zeros, 5 5 7 7 9 9 -> the median of ten values is (5 + 5) / 2
    assert median == 5.0 == np.median([0, 0, 0, 0, 5, 5, 7, 7, 9, 9])
    assert x[0, 2] == x[2, 0] == x[1, 3] == x[3, 1] == x[2, 3] == x[3, 2] == 5.0
    assert x[0, 3] == 9.0 and x[1, 2] == 7.0
    c = spectrum.data_characteristics(CodedMatrix(values, codes))
    assert c.median == 5.0
    assert np.allclose(c.eigenvalues, np.linalg.eigvalsh(spectrum.centered(x))[::-1], rtol=0, atol=0)


def test_median_of_an_even_count_with_two_different_middle_values():
    values = np.array([[NA, 1.0, 4.0], [2.0, NA, 8.0], [NA, NA, NA]])      # 1 2 | 4 8
    x, median = spectrum.filled_numeric(values)
    assert median == 3.0
    assert np.array_equal(x, [[3.0, 1.0, 4.0], [2.0, 3.0, 8.0], [3.0, 3.0, 3.0]])


def test_a_character_matrix_is_parsed_once():
    M = np.array([["0", "2", ">8"], ["2", "0", "NA"], ["<1", "4", "0"]], dtype=object)
    x, median = spectrum.filled_numeric(M)
    assert median == 1.0 == np.median([0, 0, 0, 2, 2, 4])      # (0 + 2) / 2: neither threshold's number counts
    assert x[0, 2] == x[1, 2] == x[2, 0] == 1.0 and x[2, 1] == 4.0


def test_literal_transcription_agrees_with_the_mean_subtraction_form():
    n = 150
    from topolow_amd import synthetic
    x, _ = spectrum.filled_numeric(synthetic.make_problem(n, 5, 0.5).dissimilarity)
    J = np.eye(n) - np.ones((n, n)) / n
    literal = np.linalg.eigvalsh(-0.5 * J @ (x * x) @ J)[::-1]
    form = np.linalg.eigvalsh(spectrum.centered(x))[::-1]
    assert np.all(np.abs(literal - form) <= eig_tol(n, form))


def test_error_cases_carry_r_message():
    with pytest.raises(ValueError, match="infinite or missing values in 'x'"):
        spectrum.data_characteristics(np.full((3, 3), NA))
    D = np.ones((3, 3)) - np.eye(3)
    D[0, 1] = np.inf
    with pytest.raises(ValueError, match="infinite or missing values in 'x'"):
        spectrum.data_characteristics(D)
    codes = np.zeros((3, 3), dtype=np.int8)
    codes[0, 1] = 1      # the infinite cell is a threshold: as.numeric makes it NA, and it is filled
    assert spectrum.data_characteristics(CodedMatrix(D, codes)).median == 1.0
    codes[:] = 1         # nothing numeric is left
    with pytest.raises(ValueError, match="infinite or missing values in 'x'"):
        spectrum.data_characteristics(CodedMatrix(D, codes))


def test_spectrum_scores_edge_rules():
    assert spectrum.spectrum_scores([0.0, -1.0]) == (1.0, 1, 0, 1)          # nothing positive: 1.0, at least 1 dimension
    assert spectrum.spectrum_scores([1e-13, -1e-13]) == (1.0, 1, 0, 0)      # inside the thresholds: neither
    assert spectrum.spectrum_scores([9.0, 1.0, -2.0]) == (0.2, 1, 2, 1)


def test_adjust_ndim_range_three_branches():
    assert spectrum.adjust_ndim_range((2, 10), 3) == ((2, 5), "adjusted")       # 5 < 10
    assert spectrum.adjust_ndim_range((8, 10), 3) == ((8, 10), "warning")       # 5 < 8: the range stays
    assert spectrum.adjust_ndim_range((2, 10), 8) == ((2, 10), None)            # 10 is not below 10
    assert spectrum.adjust_ndim_range((2, 10), 20) == ((2, 10), None)
    assert spectrum.adjust_ndim_range([5, 10], 3) == ((5, 5), "adjusted")       # 5 is not below the minimum 5


def test_device_form_is_taken_only_with_a_handle():
    class Fake:
        def spectrum(self, want_eigenvalues=True, want_centered=False):
            return (dict(median=1.5, deviation_score=0.25, dims_90=2, n_positive=2, n_negative=1),
                    np.array([2.0, 2.0, 0.0, -1.0]), None)

    c = spectrum.data_characteristics(None, handle=Fake())
    assert (c.median, c.deviation_score, c.dims_90_percent, c.n_positive, c.n_negative) == (1.5, 0.25, 2, 2, 1)


# ---- the NumPy model of the device's algorithm ----
@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 65])
def test_model_against_eigvalsh(n):
    a = random_symmetric(n)
    d, e = spectrum_model.tridiagonalize(a)
    ref = np.linalg.eigvalsh(a)[::-1]
    assert abs(d.sum() - np.trace(a)) <= 4 * n * U * np.abs(np.diag(a)).sum() + eig_tol(n, ref)
    for got in (np.linalg.eigvalsh(dense_tridiagonal(d, e))[::-1], spectrum_model.bisect(d, e)):
        assert np.all(np.abs(got - ref) <= eig_tol(n, ref))


def test_model_takes_no_reflection_on_a_zero_sub_column():
    a = dense_tridiagonal([1.0, 2.0, 3.0, 4.0], [0.5, 0.0, -0.25])
    d, e = spectrum_model.tridiagonalize(a)
    assert np.array_equal(d, [1.0, 2.0, 3.0, 4.0]) and np.array_equal(e, [0.5, 0.0, -0.25])
    assert np.array_equal(spectrum_model.bisect(np.zeros(5), np.zeros(4)), np.zeros(5))
