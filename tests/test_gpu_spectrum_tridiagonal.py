"""The symmetric eigenvalue path on the device (run with -m gpu; topolow_amd/csrc/relax_spectrum.h): Sturm bisection
alone through _native.tridiagonal_eigenvalues, and the Householder tridiagonalisation through
_native.symmetric_eigenvalues, against closed forms and np.linalg.eigvalsh.

Sizes: one workgroup and the edges of its 64-lane waves (63, 64, 65), more than one column chunk of 256 (257), more
than one block of 64 lines per partial sum (65, 257) and a ragged last one of a single line (1 025), and n = 1, 2, 3
where no or one reflection is taken."""
import numpy as np
import pytest

from topolow_amd import _native

from tests.spectrum_helpers import U, dense_tridiagonal, eig_tol, lower_symmetrised, symmetric_cases

pytestmark = pytest.mark.gpu


def bisection_bound(d, e):
    """8 u ||T||_inf: floating-point Sturm counts are exact for entries perturbed by a few u relative, which moves an
    eigenvalue by at most about 3 (few u) ||T||_inf; the interval ends at a width of 2 u |lambda|."""
    return 8.0 * U * float(np.max(np.abs(dense_tridiagonal(d, e)).sum(axis=1)))


# ---- bisection alone ----
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1025])
def test_toeplitz_against_the_closed_form(n):
    d, e = np.full(n, 2.0), np.full(n - 1, -1.0)
    got = _native.tridiagonal_eigenvalues(d, e)
    want = np.sort(2.0 - 2.0 * np.cos(np.arange(1, n + 1) * np.pi / (n + 1)))[::-1]
    err = float(np.max(np.abs(got - want)))
    print("toeplitz n = %d: max error %.3g, bound %.3g" % (n, err, bisection_bound(d, e)))
    assert got.shape == (n,) and np.all(np.diff(got) <= 0)
    assert err <= bisection_bound(d, e)


def test_wilkinson_w21_plus():
    d, e = np.abs(np.arange(21) - 10.0), np.ones(20)
    got = _native.tridiagonal_eigenvalues(d, e)
    want = np.linalg.eigvalsh(dense_tridiagonal(d, e))[::-1]
    err = float(np.max(np.abs(got - want)))
    print("W21+: max error %.3g, bound %.3g; closest pair %.3g apart" % (err, bisection_bound(d, e), got[0] - got[1]))
    assert err <= bisection_bound(d, e)
    assert np.all(np.diff(got) <= 0) and 0 <= got[0] - got[1] < 1e-12      # the largest pair agrees to about 14 digits


def test_a_split_matrix_and_an_all_zero_one():
    rng = np.random.default_rng(3)
    d, e = rng.normal(size=40), rng.normal(size=39)
    e[19] = 0.0
    got = _native.tridiagonal_eigenvalues(d, e)
    want = np.sort(np.concatenate([np.linalg.eigvalsh(dense_tridiagonal(d[:20], e[:19])),
                                   np.linalg.eigvalsh(dense_tridiagonal(d[20:], e[20:]))]))[::-1]
    err = float(np.max(np.abs(got - want)))
    print("split: max error %.3g, bound %.3g" % (err, bisection_bound(d, e)))
    assert err <= bisection_bound(d, e)
    for n in (1, 5, 64):
        assert np.array_equal(_native.tridiagonal_eigenvalues(np.zeros(n), np.zeros(n - 1)), np.zeros(n))
    diag = np.array([3.0, -1.0, 2.0, 2.0])
    assert np.max(np.abs(_native.tridiagonal_eigenvalues(diag, np.zeros(3)) - [3.0, 2.0, 2.0, -1.0])) <= 8 * U * 3.0


# ---- tridiagonalisation ----
CASES = symmetric_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_tridiagonal_form_and_eigenvalues(name):
    a = CASES[name]
    n = a.shape[0]
    sym = lower_symmetrised(a)
    ref = np.linalg.eigvalsh(a)[::-1]           # UPLO = "L"
    tol = eig_tol(n, ref)
    eig, d, e = _native.symmetric_eigenvalues(a, want_tridiagonal=True)
    assert d.shape == (n,) and e.shape == (n - 1,) and eig.shape == (n,)
    # sum(d) and sum(d^2) + 2 sum(e^2) are the first two power sums of T's eigenvalues, each within tol of A's, plus
    # the rounding of the sums themselves
    scale = float(np.max(np.abs(ref)))
    assert abs(d.sum() - np.trace(sym)) <= n * tol + 2 * n * U * float(np.abs(np.diag(sym)).sum() + np.abs(d).sum())
    frob = float((sym * sym).sum())
    assert abs(float((d * d).sum() + 2.0 * (e * e).sum()) - frob) <= 2 * n * scale * tol + 4 * n * U * frob
    via_numpy = np.linalg.eigvalsh(dense_tridiagonal(d, e))[::-1]
    print("%s n = %d: eigenvalue error / (n u max|lambda|): tridiagonal + eigvalsh %.4f, device %.4f" %
          (name, n, np.max(np.abs(via_numpy - ref)) / (n * U * scale), np.max(np.abs(eig - ref)) / (n * U * scale)))
    assert np.all(np.abs(via_numpy - ref) <= tol)
    assert np.all(np.abs(eig - ref) <= tol)
    assert np.all(np.diff(eig) <= 0)
    again = _native.symmetric_eigenvalues(a, want_tridiagonal=True)
    assert all(np.array_equal(x, y) for x, y in zip((eig, d, e), again))      # the same bits


def test_a_zero_sub_column_takes_no_reflection():
    eig, d, e = _native.symmetric_eigenvalues(np.eye(6) * 3.0, want_tridiagonal=True)
    assert np.array_equal(d, np.full(6, 3.0)) and np.array_equal(e, np.zeros(5))
    assert np.max(np.abs(eig - 3.0)) <= 8 * U * 3.0
    t = dense_tridiagonal([1.0, 2.0, 3.0, 4.0], [0.5, 0.0, -0.25])           # tridiagonal already: kept as it is
    _, d, e = _native.symmetric_eigenvalues(t, want_tridiagonal=True, want_eigenvalues=False)
    assert np.array_equal(d, [1.0, 2.0, 3.0, 4.0]) and np.array_equal(np.abs(e), [0.5, 0.0, 0.25])


def test_outputs_are_optional_and_the_upper_triangle_is_ignored():
    a = CASES["random65"].copy()
    want = _native.symmetric_eigenvalues(a)
    a[np.triu_indices(65, 1)] = np.nan                    # not even read
    assert np.array_equal(_native.symmetric_eigenvalues(a), want)
    none, d, e = _native.symmetric_eigenvalues(a, want_tridiagonal=True, want_eigenvalues=False)
    assert none is None and np.array_equal(_native.tridiagonal_eigenvalues(d, e), want)
    one = _native.symmetric_eigenvalues(np.array([[-2.5]]), want_tridiagonal=True)     # n = 1: no step at all
    assert np.array_equal(one[1], [-2.5]) and one[2].shape == (0,) and abs(one[0][0] + 2.5) <= 8 * U * 2.5
