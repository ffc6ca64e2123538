"""What the spectrum tests share: their problems, the eigenvalue tolerance and the host quantities of a case.

Eigenvalue tolerance: tol = EIG_TOL_C * n * u * max|lambda|, u = 2^-52 -- the form of the worst-case bound for two
backward-stable solvers (Weyl, ||E||_2 <= p(n) u ||B||_2).  The constant was set on the CPU, without the code under
test: tests/models/spectrum_model.py (the device's algorithm in NumPy) against np.linalg.eigvalsh over the problems
below (`python -m tests.spectrum_helpers` prints the ratios), 8 times the largest ratio seen -- the margin because the
device adds in another order than the model.  Largest ratio: 0.5015 (the 3 x 3 random matrix; the 2-point handle case
0.44; the handle problems of n >= 64 0.015 .. 0.10, the symmetric ones of n >= 63 0.045 .. 0.25); 8 x 0.5015 = 4.012."""
import numpy as np

from topolow_amd import synthetic

U = 2.0 ** -52
EIG_TOL_C = 4.012
NA = np.nan


def eig_tol(n, lam):
    return EIG_TOL_C * n * U * float(np.max(np.abs(lam)))


# ---- symmetric matrices (tests/test_gpu_spectrum_tridiagonal.py) ----
def random_symmetric(n, seed=None):
    a = np.random.default_rng(1000 + n if seed is None else seed).normal(size=(n, n))
    return a + a.T


def dense_tridiagonal(d, e):
    d, e = np.asarray(d, dtype=np.float64), np.asarray(e, dtype=np.float64)
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


def symmetric_cases():
    """name -> matrix; only the lower triangle counts."""
    rng = np.random.default_rng(7)
    cases = {"identity": np.eye(40), "diagonal": np.diag(rng.normal(size=70) * 10.0),
             "tridiagonal": dense_tridiagonal(rng.normal(size=90), rng.normal(size=89))}
    x = rng.normal(size=100)
    cases["rank1"] = np.outer(x, x)
    for n in (2, 3, 5, 63, 64, 65, 257, 1025):
        cases["random%d" % n] = random_symmetric(n)
    g = random_symmetric(130, seed=5)
    g[np.triu_indices(130, 1)] = rng.normal(size=130 * 129 // 2) * 1e6     # garbage above the diagonal
    cases["garbage_upper"] = g
    return cases


def lower_symmetrised(a):
    return np.tril(a) + np.tril(a, -1).T


# ---- dissimilarity matrices (tests/test_gpu_spectrum_handle.py) ----
def titre_levels(n, seed, even):
    """A symmetric matrix of a handful of titre-like levels.  Odd count of numeric cells, the middle rank deep inside
    one level: both ranks of the select fall in one bucket.  `even`: the count is even and the two middle ranks are
    the last cell of one level and the first of the next (the median lies between two levels)."""
    rng = np.random.default_rng(seed)
    levels = np.array([1.0, 2.0, 3.0, 4.0, 6.0])
    D = levels[rng.integers(0, 5, size=(n, n))]
    D = np.triu(D, 1)
    D = D + D.T
    if not even:
        D[0, 1] = D[1, 0] = NA      # n^2 - 2 numeric cells: odd when n is odd
        return D
    # an even count split exactly between "<= 2" (the diagonal zeros among them) and ">= 3": the surplus of the larger
    # side becomes NA (holes in one triangle only are fine: the matrix need not be symmetric)
    flat = D.reshape(-1)
    small = np.nonzero((flat <= 2.0) & (flat > 0.0))[0]
    large = np.nonzero(flat >= 3.0)[0]
    surplus = (small.shape[0] + n) - large.shape[0]
    if surplus > 0:
        flat[small[:surplus]] = NA
    else:
        flat[large[:-surplus]] = NA
    return D


def handle_cases():
    """name -> (values, codes or None)."""
    cases = {}
    for n, missing in ((64, 0.0), (200, 0.3), (333, 0.7)):
        cases["problem%d" % n] = (synthetic.make_problem(n, 5, missing).dissimilarity, None)
    cases["tied_one_bucket"] = (titre_levels(75, 3, even=False), None)
    cases["tied_two_buckets"] = (titre_levels(70, 4, even=True), None)
    D = synthetic.make_problem(90, 5, 0.2).dissimilarity.copy()
    rng = np.random.default_rng(11)
    neg = np.triu(rng.random((90, 90)) < 0.05, 1)
    D[neg | neg.T] *= -1.0
    cases["negative"] = (D, None)
    D = synthetic.make_problem(130, 5, 0.4).dissimilarity.copy()
    u = np.triu(rng.random((130, 130)), 1)
    u = u + u.T
    codes = np.zeros((130, 130), dtype=np.int8)
    codes[(u > 0) & (u < 0.10) & ~np.isnan(D)] = 1
    codes[(u >= 0.10) & (u < 0.15) & ~np.isnan(D)] = -1
    cases["thresholds"] = (D, codes)
    D = synthetic.make_problem(101, 5, 0.3).dissimilarity.copy()
    D = D * (1.0 + 0.2 * rng.random((101, 101)))       # every pair measured twice, differently
    D[rng.random((101, 101)) < 0.1] = NA               # and holes in one triangle only
    cases["asymmetric"] = (D, None)
    cases["two_points"] = (np.array([[0.0, 3.0], [3.0, 0.0]]), None)
    return cases


def host_quantities(values, codes):
    """The host form's median, filled matrix, B, spectrum (descending) and scores of a case."""
    from topolow_amd import spectrum
    from topolow_amd.core import CodedMatrix
    cm = CodedMatrix(np.asarray(values, dtype=np.float64),
                     np.zeros(np.shape(values), dtype=np.int8) if codes is None else np.asarray(codes))
    x, median = spectrum.filled_numeric(cm)
    B = spectrum.centered(x)
    lam = np.linalg.eigvalsh(B)[::-1].copy()
    return dict(median=median, x=x, B=B, lam=lam, scores=spectrum.spectrum_scores(lam),
                n_numeric=int(np.sum((cm.codes == 0) & ~np.isnan(cm.values))))


if __name__ == "__main__":   # the calibration of EIG_TOL_C: the model against eigvalsh, no device
    from tests.models import spectrum_model
    worst = 0.0
    for name, a in symmetric_cases().items():
        ref = np.linalg.eigvalsh(a)[::-1]
        got = spectrum_model.eigenvalues(a)
        ratio = float(np.max(np.abs(got - ref))) / (a.shape[0] * U * max(float(np.max(np.abs(ref))), 1e-300))
        worst = max(worst, ratio)
        print("symmetric %-16s n = %4d  ratio %.4f" % (name, a.shape[0], ratio), flush=True)
    for name, (values, codes) in handle_cases().items():
        q = host_quantities(values, codes)
        got = spectrum_model.eigenvalues(q["B"])
        n = q["B"].shape[0]
        ratio = float(np.max(np.abs(got - q["lam"]))) / (n * U * float(np.max(np.abs(q["lam"]))))
        worst = max(worst, ratio)
        print("handle    %-16s n = %4d  ratio %.4f  dims_90 %d" % (name, n, ratio, q["scores"][1]), flush=True)
    print("largest ratio %.4f -> EIG_TOL_C = 8 x = %.3f" % (worst, 8.0 * worst))
