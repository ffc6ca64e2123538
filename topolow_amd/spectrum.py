"""Step 1 of the reference's Euclidify() wizard, "Assessing data characteristics" (R/core.R:983-1032): the spectrum of
the double-centred, median-filled, squared dissimilarity matrix, the non-Euclidean deviation score, the number of
dimensions that carry 90 % of the positive spectrum, and the cap they put on ndim_range.

`data_characteristics(D)` is the host form in NumPy and the specification of the device form,
`data_characteristics(D, handle=h)`, which runs on the matrix a PreparedHandle keeps on the device
(topolow_layout_prep_spectrum, include/topolow_relax.h).  The device form is taken only when a handle is passed."""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import _native
from .core import coded_matrix

POSITIVE, NEGATIVE = 1e-12, -1e-12       # R/core.R:994-995
R_MESSAGE = "infinite or missing values in 'x'"   # what R's eigen() stops with


@dataclass
class DataCharacteristics:
    median: float
    eigenvalues: np.ndarray      # descending, as R's eigen()
    deviation_score: float
    dims_90_percent: int
    n_positive: int
    n_negative: int


def spectrum_scores(eigenvalues) -> Tuple[float, int, int, int]:
    """R/core.R:994-1007 on eigenvalues in descending order: (deviation_score, dims_90_percent, n_positive, n_negative)."""
    lam = np.asarray(eigenvalues, dtype=np.float64)
    pos, neg = lam[lam > POSITIVE], lam[lam < NEGATIVE]
    score = float(np.sum(np.abs(neg)) / np.sum(pos)) if pos.size > 0 else 1.0
    dims = int(pos.size)
    if pos.size > 0:
        hit = np.nonzero(np.cumsum(pos) / np.sum(pos) >= 0.90)[0]
        if hit.size > 0:
            dims = int(hit[0]) + 1
    return score, max(1, dims), int(pos.size), int(neg.size)


def filled_numeric(dissimilarity_matrix) -> Tuple[np.ndarray, float]:
    """as.numeric(matrix) with every NA -- threshold strings among them -- filled with the median of the numeric cells
    (diagonal and both triangles count): (the filled matrix, the median).  ValueError with R's message when no cell is
    numeric or a numeric cell is infinite."""
    cm = coded_matrix(dissimilarity_matrix)
    if cm is None:
        raise ValueError("dissimilarity_matrix must be a matrix")
    x = np.array(cm.as_numeric(), dtype=np.float64)
    numeric = ~np.isnan(x)
    if not numeric.any() or np.isinf(x[numeric]).any():
        raise ValueError(R_MESSAGE)
    median = float(np.median(x[numeric]))
    x[~numeric] = median
    return x, median


def centered(x: np.ndarray) -> np.ndarray:
    """B = -0.5 J x^2 J in its mean-subtraction form: -0.5 (x^2 - row means - column means + grand mean)."""
    d2 = x * x
    return -0.5 * (d2 - d2.mean(axis=1, keepdims=True) - d2.mean(axis=0, keepdims=True) + d2.mean())


def data_characteristics(dissimilarity_matrix, handle: Optional["_native.PreparedHandle"] = None) -> DataCharacteristics:
    """Median, spectrum, deviation_score and dims_90_percent of a dissimilarity matrix.  Without `handle`: NumPy on the
    host.  With `handle` (a PreparedHandle of this matrix; `dissimilarity_matrix` may then be None): on the device,
    from what the handle holds."""
    if handle is not None:
        try:
            info, eig, _ = handle.spectrum(want_eigenvalues=True, want_centered=False)
        except _native.NativeError as exc:
            if exc.code == _native.ERR_BAD_ARGUMENT and R_MESSAGE in str(exc):
                raise ValueError(R_MESSAGE) from exc
            raise
        return DataCharacteristics(float(info["median"]), eig, float(info["deviation_score"]), int(info["dims_90"]),
                                   int(info["n_positive"]), int(info["n_negative"]))
    x, median = filled_numeric(dissimilarity_matrix)
    eig = np.linalg.eigvalsh(centered(x))[::-1].copy()     # UPLO = "L": the lower triangle, as eigen(symmetric = TRUE)
    score, dims, n_pos, n_neg = spectrum_scores(eig)
    return DataCharacteristics(median, eig, score, dims, n_pos, n_neg)


def adjust_ndim_range(ndim_range, dims_90_percent: int):
    """R/core.R:1016-1032: (ndim_range, message).  suggested = dims_90_percent + 2; below the range's minimum the range
    stays and the message is "warning"; below its maximum the maximum is lowered to it and the message is "adjusted";
    otherwise the range stays and the message is None."""
    lo, hi = int(ndim_range[0]), int(ndim_range[1])
    suggested = int(dims_90_percent) + 2
    if suggested < lo:
        return (lo, hi), "warning"
    if suggested < hi:
        return (lo, suggested), "adjusted"
    return (lo, hi), None
