"""Host driver of the relaxation path: a Python mirror of the reference's R driver.

Mirrors, step by step, `euclidean_embedding()` (R/core.R:184-528 of the reference),
`create_topolow_map()` (R/core.R:616-664) and the `topolow` S3 methods (R/core.R:684-719):
same argument names, defaults, validation messages and returned fields.  The native step
-- the reference's `.Call("_topolow_optimize_layout_exact_cpp", ...)` at R/core.R:439-456 --
goes to the HIP library through :mod:`topolow_amd._native`; there is no CPU fallback.

R matrices map to Python as follows:
  * numeric matrix with NA      -> 2-D float ndarray, NaN = NA
  * character matrix (">5",...) -> 2-D object/str ndarray, None/NaN = NA
  * dimnames                    -> a pandas DataFrame's index, or the `names=` of `RMatrix`
"""
from __future__ import annotations

import math
import os
import re
import warnings
from contextlib import ExitStack
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

_MISSING = object()


# --------------------------------------------------------------------------------------
# R-matrix adaptor
# --------------------------------------------------------------------------------------
@dataclass
class RMatrix:
    """A matrix with optional row names (R's `matrix` + `rownames`)."""
    values: np.ndarray
    names: Optional[List[str]] = None


def _as_rmatrix(x: Any) -> Optional[RMatrix]:
    """Return an RMatrix if `x` is matrix-like in the R sense (`is.matrix`), else None."""
    if isinstance(x, RMatrix):
        return RMatrix(np.asarray(x.values), list(x.names) if x.names is not None else None)
    if hasattr(x, "to_numpy") and hasattr(x, "index") and hasattr(x, "columns"):
        return RMatrix(x.to_numpy(), [str(v) for v in x.index])
    if isinstance(x, np.ndarray) and x.ndim == 2:
        return RMatrix(x, None)
    return None


def _is_character(v: np.ndarray) -> bool:
    return v.dtype.kind in ("U", "S", "O")


def _is_na_cell(c: Any) -> bool:
    if c is None:
        return True
    if isinstance(c, float) and math.isnan(c):
        return True
    if isinstance(c, str) and c == "NA":
        return True
    return False


_NUM_RE = re.compile(r"^\s*[-+]?(?:(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?|Inf|inf|NaN|nan)\s*$")


def _as_numeric_scalar(c: Any) -> float:
    """R's as.numeric() on one cell: unparsable strings become NA (NaN here)."""
    if _is_na_cell(c):
        return math.nan
    if isinstance(c, (int, float, np.integer, np.floating)):
        return float(c)
    s = str(c)
    if _NUM_RE.match(s):
        return float(s)
    return math.nan


def _as_numeric(v: np.ndarray) -> np.ndarray:
    if not _is_character(v):
        return np.asarray(v, dtype=np.float64)
    out = np.empty(v.shape, dtype=np.float64)
    flat = out.reshape(-1)
    for q, c in enumerate(v.reshape(-1)):
        flat[q] = _as_numeric_scalar(c)
    return out


def _is_na(v: np.ndarray) -> np.ndarray:
    if not _is_character(v):
        return np.isnan(np.asarray(v, dtype=np.float64))
    out = np.empty(v.shape, dtype=bool)
    flat = out.reshape(-1)
    for q, c in enumerate(v.reshape(-1)):
        flat[q] = _is_na_cell(c)
    return out


@dataclass
class CodedMatrix:
    """Numeric twin of R's character dissimilarity matrix: `values` holds the number of every
    cell with any "<"/">" prefix stripped (NaN = NA), `codes` the prefix (0 none, 1 ">", -1 "<").
    All of the driver's matrix logic runs on this form; strings are parsed once, up front."""
    values: np.ndarray
    codes: np.ndarray
    names: Optional[List[str]] = None
    character: bool = False   # was the source a character matrix? (is.character(), R/core.R:278)

    def as_numeric(self) -> np.ndarray:
        """as.numeric(matrix): threshold strings become NA."""
        return np.where(self.codes == 0, self.values, np.nan)

    def reordered(self, order: np.ndarray) -> "CodedMatrix":
        ix = np.ix_(order, order)
        return CodedMatrix(self.values[ix], self.codes[ix],
                           [self.names[q] for q in order] if self.names is not None else None,
                           self.character)

    def masked(self, rows: np.ndarray, cols: np.ndarray) -> "CodedMatrix":
        v, c = self.values.copy(), self.codes.copy()
        v[rows, cols] = np.nan
        v[cols, rows] = np.nan
        c[rows, cols] = 0
        c[cols, rows] = 0
        return CodedMatrix(v, c, self.names, self.character)


def coded_matrix(x: Any) -> Optional[CodedMatrix]:
    """Any accepted matrix-like -> CodedMatrix (None if `x` is not a matrix in R's sense)."""
    if isinstance(x, CodedMatrix):
        return x
    m = _as_rmatrix(x)
    if m is None:
        return None
    v = m.values
    if not _is_character(v):
        vals = np.array(v, dtype=np.float64)
        return CodedMatrix(vals, np.zeros(vals.shape, dtype=np.int8), m.names, False)
    vals = np.full(v.shape, np.nan)
    codes = np.zeros(v.shape, dtype=np.int8)
    fv, fc = vals.reshape(-1), codes.reshape(-1)
    for q, c in enumerate(v.reshape(-1)):
        if _is_na_cell(c):
            continue
        if isinstance(c, str):
            if c.startswith(">"):
                fc[q] = 1
                fv[q] = _as_numeric_scalar(c[1:])
            elif c.startswith("<"):
                fc[q] = -1
                fv[q] = _as_numeric_scalar(c[1:])
            else:
                fv[q] = _as_numeric_scalar(c)
        else:
            fv[q] = _as_numeric_scalar(c)
    return CodedMatrix(vals, codes, m.names, True)


# --------------------------------------------------------------------------------------
# result object (R/core.R:505-527) and its S3 methods (R/core.R:684-719)
# --------------------------------------------------------------------------------------
@dataclass
class Topolow:
    positions: np.ndarray
    est_distances: np.ndarray
    mae: float
    iter: int
    parameters: Dict[str, Any]
    convergence: Dict[str, Any]
    names: Optional[List[str]] = None
    # side channel (not part of the reference object): timing / schedule of the native run
    native_info: Dict[str, Any] = field(default_factory=dict, repr=False)

    r_class = "topolow"

    def __getitem__(self, key: str):
        if key in ("positions", "est_distances", "mae", "iter", "parameters", "convergence"):
            return getattr(self, key)
        raise KeyError(key)

    def keys(self):
        return ["positions", "est_distances", "mae", "iter", "parameters", "convergence"]

    def __contains__(self, key):
        return key in self.keys()

    def format(self) -> str:
        """Text of print.topolow (R/core.R:684-692)."""
        achieved = "TRUE" if self.convergence["achieved"] else "FALSE"
        return ("topolow optimization result:\n"
                f"Dimensions: {int(self.parameters['ndim'])}\n"
                f"Iterations: {int(self.iter)}\n"
                f"MAE: {self.mae:.4f}\n"
                f"Convergence achieved: {achieved}\n"
                f"Final convergence error: {self.convergence['error']:.4f}\n")

    def __str__(self) -> str:
        return self.format()

    def summary(self) -> str:
        """Text of summary.topolow (R/core.R:713-719)."""
        return (self.format() + "\nParameters:\n"
                f"k0: {self.parameters['k0']:.4f}\n"
                f"cooling_rate: {self.parameters['cooling_rate']:.4f}\n"
                f"c_repulsion: {self.parameters['c_repulsion']:.4f}\n")


def print_topolow(x: Topolow) -> Topolow:
    print(x.format(), end="")
    return x


def summary_topolow(x: Topolow) -> None:
    print(x.summary(), end="")


# --------------------------------------------------------------------------------------
# the .Call payload
# --------------------------------------------------------------------------------------
@dataclass
class LayoutCall:
    """Arguments of `optimize_layout_exact_cpp` exactly as R/core.R:439-456 passes them."""
    initial_positions: np.ndarray      # n x ndim float64
    dissimilarity_matrix: np.ndarray   # n x n float64, Inf = unmeasured, symmetric
    threshold_matrix: np.ndarray       # n x n int32 {0, 1, -1}, symmetric
    degrees: np.ndarray                # n int32
    edge_i: np.ndarray                 # E int32, 0-based
    edge_j: np.ndarray
    edge_dist: np.ndarray              # E float64
    edge_thresh: np.ndarray            # E int32
    n_iter: int
    k0: float
    cooling_rate: float
    c_repulsion: float
    relative_epsilon: float
    convergence_window: int
    convergence_check_freq: int
    verbose: bool
    # bookkeeping for the post-processing half
    names: Optional[List[str]] = None
    order: Optional[np.ndarray] = None            # permutation applied (None = identity)
    reordered_matrix: Optional[Any] = None         # the (reordered) input as a CodedMatrix


def _stop(msg: str):
    raise ValueError(msg)


_NO_EDGES = "No valid off-diagonal measurements found in dissimilarity matrix"


def _is_number(x: Any) -> bool:
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool)


def _validate(m: Optional[CodedMatrix], ndim, mapping_max_iter, k0, cooling_rate, c_repulsion,
              relative_epsilon, convergence_counter, convergence_check_freq,
              initial_positions, n_finite_nonzero: Optional[int] = None) -> None:
    """R/core.R:202-264, messages verbatim.  n_finite_nonzero: the count of finite non-zero dissimilarities where
    the caller has it already (the device form); otherwise it is taken from the matrix."""
    if m is None:
        _stop("dissimilarity_matrix must be a matrix")
    v = m.values
    if v.shape[0] != v.shape[1]:
        _stop("dissimilarity_matrix must be square")
    if n_finite_nonzero is None:
        finite = m.as_numeric().copy()
        finite[np.isinf(finite)] = np.nan
        n_finite_nonzero = int(np.sum(~np.isnan(finite) & (finite != 0)))
    if n_finite_nonzero == 0:
        warnings.warn("No finite non-zero dissimilarities found. Results may be unreliable.",
                      UserWarning, stacklevel=3)
    if not _is_number(ndim) or ndim < 1 or ndim != round(ndim):
        _stop("ndim must be a positive integer")
    if not _is_number(mapping_max_iter) or mapping_max_iter < 1 or \
            mapping_max_iter != round(mapping_max_iter):
        _stop("mapping_max_iter must be a positive integer")
    if not _is_number(k0) or k0 <= 0:
        _stop("k0 must be a positive number")
    if k0 > 30:
        warnings.warn("High k0 value (> 30) may lead to instability", UserWarning, stacklevel=3)
    if not _is_number(cooling_rate) or cooling_rate <= 0 or cooling_rate >= 1:
        _stop("cooling_rate must be between 0 and 1")
    if not _is_number(c_repulsion) or c_repulsion <= 0:
        _stop("c_repulsion must be a positive number")
    if not _is_number(relative_epsilon) or relative_epsilon <= 0:
        _stop("relative_epsilon must be a positive number")
    if not _is_number(convergence_counter) or convergence_counter < 1 or \
            convergence_counter != round(convergence_counter):
        _stop("convergence_counter must be a positive integer")
    if not _is_number(convergence_check_freq) or convergence_check_freq < 1:
        _stop("convergence_check_freq must be a positive integer")
    if initial_positions is not None:
        ip = _as_rmatrix(initial_positions)
        if ip is None:
            _stop("initial_positions must be a matrix")
        if ip.values.shape[0] != v.shape[0]:
            _stop("initial_positions must have same number of rows as dissimilarity_matrix")
        if ip.values.shape[1] != ndim:
            _stop("initial_positions must have ndim columns")
    if v.shape[0] < 2:
        _stop("dissimilarity_matrix must have at least 2 rows/columns")


def spectral_order(stripped: np.ndarray) -> Optional[np.ndarray]:
    """R/core.R:269-319: ascending order of each point's mean dissimilarity
    (mean of row mean and column mean over non-NA off-diagonal cells; threshold prefixes
    stripped -- `stripped` is CodedMatrix.values).  Returns None where the reference keeps
    the input order."""
    try:
        numeric = np.array(stripped, dtype=np.float64)
        np.fill_diagonal(numeric, np.nan)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            row_means = np.nanmean(numeric, axis=1)
            col_means = np.nanmean(numeric, axis=0)
        avg = (row_means + col_means) / 2.0
        avg[np.isnan(avg)] = 0.0
        if int(np.sum(avg > 0)) > 1:
            return np.argsort(avg, kind="stable")
    except Exception:  # the reference wraps this block in tryCatch and skips reordering
        return None
    return None


def _announce_order(preserve_order, reordered: bool, verbose) -> None:
    """The verbose line of the reordering step (R/core.R:269-322)."""
    if not verbose:
        return
    if preserve_order:
        print("Preserving original row/column order (preserve_order = TRUE)")
    elif reordered:
        print("Matrix reordered for spectral pattern (largest values in corners)")
    else:
        print("Insufficient data for meaningful spectral ordering")


def _align_initial_positions(initial_positions, names) -> Optional[np.ndarray]:
    """The caller's start positions in the order of `names` -- they follow the matrix only through row names
    (R/core.R:325-333) -- or None where there are none."""
    if initial_positions is None:
        return None
    ip = _as_rmatrix(initial_positions)
    init = np.asarray(ip.values, dtype=np.float64)
    if ip.names is not None and names is not None and list(ip.names) != list(names):
        lookup = {nm: q for q, nm in enumerate(ip.names)}
        try:
            init = init[[lookup[nm] for nm in names], :]
        except KeyError:
            raise IndexError("subscript out of bounds") from None
    return init


def _start_walk(numeric_max, n: int, ndim: int, rng: Optional[np.random.Generator] = None,
                unit_draw: Optional[np.ndarray] = None) -> np.ndarray:
    """Start positions (R/core.R:407-415): a random walk from the origin with steps uniform(0, 2 numeric_max / n).
    The numbers are drawn here (rng; None: a fresh generator) or handed in (unit_draw: the (ndim, n - 1) array
    rng.random would have returned at this point of the stream -- uniform(0, 2a) is 2a * random(), bit for bit)."""
    init_step = np.float64(numeric_max) / n
    if unit_draw is None:
        gen = rng if rng is not None else np.random.default_rng()
        # runif fills the (n-1) x ndim matrix column by column
        steps = gen.uniform(0.0, 2.0 * init_step, size=(ndim, n - 1)).T
    else:
        steps = (0.0 + (2.0 * init_step - 0.0) * unit_draw).T      # Generator.uniform's arithmetic
    return np.vstack([np.zeros((1, ndim)), np.cumsum(steps, axis=0)])


def _layout_call(init, dense, tdense, degrees, edge_i, edge_j, edge_dist, edge_thresh, mapping_max_iter, k0,
                 cooling_rate, c_repulsion, relative_epsilon, convergence_counter, convergence_check_freq, verbose,
                 names, order, reordered_matrix) -> LayoutCall:
    return LayoutCall(
        initial_positions=np.ascontiguousarray(init, dtype=np.float64),
        dissimilarity_matrix=dense, threshold_matrix=tdense, degrees=degrees,
        edge_i=edge_i, edge_j=edge_j, edge_dist=edge_dist, edge_thresh=edge_thresh,
        n_iter=int(mapping_max_iter), k0=float(k0), cooling_rate=float(cooling_rate),
        c_repulsion=float(c_repulsion), relative_epsilon=float(relative_epsilon),
        convergence_window=int(convergence_counter),
        convergence_check_freq=int(convergence_check_freq), verbose=bool(verbose),
        names=names, order=order, reordered_matrix=reordered_matrix)


def prepare_layout_call(dissimilarity_matrix, ndim, mapping_max_iter, k0, cooling_rate,
                        c_repulsion, relative_epsilon, convergence_counter, initial_positions,
                        verbose, convergence_check_freq, preserve_order,
                        rng: Optional[np.random.Generator] = None) -> LayoutCall:
    """Everything `euclidean_embedding` does before the `.Call` (R/core.R:202-436)."""
    m = coded_matrix(dissimilarity_matrix)
    _validate(m, ndim, mapping_max_iter, k0, cooling_rate, c_repulsion, relative_epsilon,
              convergence_counter, convergence_check_freq, initial_positions)
    n = m.values.shape[0]
    ndim = int(ndim)

    # -- reordering (R/core.R:269-322)
    order = None
    if n > 1 and not preserve_order:
        order = spectral_order(m.values)
        if order is not None:
            m = m.reordered(order)
    if n > 1 or preserve_order:
        _announce_order(preserve_order, order is not None, verbose)
    names = m.names
    init = _align_initial_positions(initial_positions, names)

    # -- degrees and parsing (R/core.R:340-374)
    non_na = ~np.isnan(m.values)
    degrees = non_na.sum(axis=1).astype(np.int32)
    distances = np.where(non_na, m.values, np.inf)
    codes = np.where(non_na, m.codes, 0).astype(np.int32)

    # -- COO edge list, upper triangle, column-major scan like which(arr.ind=TRUE)
    #    (R/core.R:383-402)
    with np.errstate(invalid="ignore"):
        valid = np.triu(np.ones((n, n), dtype=bool), k=1) & (distances != np.inf)
    cols, rows = np.nonzero(valid.T)  # column-major enumeration
    if rows.shape[0] == 0:
        _stop(_NO_EDGES)
    edge_dist = distances[rows, cols].astype(np.float64)
    edge_thresh = codes[rows, cols].astype(np.int32)

    if init is None:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            numeric_max = np.nanmax(m.as_numeric())
        init = _start_walk(numeric_max, n, ndim, rng)

    # -- symmetric dense fill: lower triangle <- transpose of upper (R/core.R:429-436)
    low = np.tril(np.ones((n, n), dtype=bool), k=-1)
    dense = distances.copy()
    dense[low] = distances.T[low]
    tdense = codes.copy()
    tdense[low] = codes.T[low]

    return _layout_call(init, dense, tdense, degrees, rows.astype(np.int32), cols.astype(np.int32), edge_dist,
                        edge_thresh, mapping_max_iter, k0, cooling_rate, c_repulsion, relative_epsilon,
                        convergence_counter, convergence_check_freq, verbose, names, order, m)


# Smallest matrix for which euclidean_embedding() prepares on the device; None: never by default.  Measured on the
# MI355X (profiles/r08_prepare_layout.txt): the host form wins at n = 300 (2.2 ms against 3.9 ms), the device form at
# n = 1 000 (10.9 ms against 26.8 ms) and from there on (106 ms against 3.59 s at n = 10 000).
# TOPOLOW_DEVICE_PREP=0 / =1 in the environment forces the choice, read per call.
_DEVICE_PREP_MIN_N: Optional[int] = 1000


def _device_front(open_fn, dissimilarity_matrix, ndim, mapping_max_iter, k0, cooling_rate, c_repulsion,
                  relative_epsilon, convergence_counter, initial_positions, verbose, convergence_check_freq,
                  preserve_order):
    """What prepare_layout_call_device and _embed_resident do alike, up to the start positions: the matrix as a
    CodedMatrix without a copy, the checks that need no upload, the matrix opened on the device, `_validate` with the
    device's count, the order and its verbose line, the caller's start positions by row names, the stop for a matrix
    without measurements.

    open_fn(values, codes, preserve_order, order=...) opens the matrix (_native.prepare_layout, or a
    _native.PreparedHandle); `.info` and `.order` are read of what it returns.  Where the device declines to order
    (order_route 3) spectral_order runs here and open_fn is called a second time with its order.

    Returns None -- nothing has been uploaded, printed or warned of by then -- where the call is not for the device: a
    character matrix, or one that `_validate` rejects for its shape or a scalar argument.  Otherwise (m, codes, own,
    opened, names, order, init, n): own, whether the caller handed a CodedMatrix in; names and order, those of the
    ordered matrix (order None where the input order is kept); init, the aligned start positions or None."""
    from . import _native
    m, codes, own = None, None, False
    if isinstance(dissimilarity_matrix, CodedMatrix):
        m = dissimilarity_matrix
        own = True
        codes = m.codes if m.codes.any() else None
    else:
        r = _as_rmatrix(dissimilarity_matrix)
        if r is not None and not _is_character(r.values):   # the matrix itself, not a copy: nothing here writes to it
            vals = np.asarray(r.values, dtype=np.float64)
            m = CodedMatrix(vals, np.zeros(vals.shape, dtype=np.int8), r.names, False)
    if m is None or m.values.ndim != 2 or m.values.shape[0] != m.values.shape[1] or m.values.shape[0] < 2:
        return None
    try:   # the checks that do not need the matrix, before anything is uploaded
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _validate(m, ndim, mapping_max_iter, k0, cooling_rate, c_repulsion, relative_epsilon,
                      convergence_counter, convergence_check_freq, initial_positions, n_finite_nonzero=1)
    except Exception:
        return None
    opened = open_fn(m.values, codes, bool(preserve_order))
    if opened.info["order_route"] == _native.ORDER_DECLINED:
        host_order = spectral_order(m.values)
        opened = open_fn(m.values, codes, False, order=host_order if host_order is not None else [-1])
    _validate(m, ndim, mapping_max_iter, k0, cooling_rate, c_repulsion, relative_epsilon,
              convergence_counter, convergence_check_freq, initial_positions,
              n_finite_nonzero=int(opened.info["n_finite_nonzero"]))
    names = m.names
    order = None if preserve_order else opened.order
    if order is not None and names is not None:
        names = [names[q] for q in order]
    _announce_order(preserve_order, order is not None, verbose)
    init = _align_initial_positions(initial_positions, names)
    if int(opened.info["n_edges"]) == 0:
        _stop(_NO_EDGES)
    return m, codes, own, opened, names, order, init, m.values.shape[0]


def prepare_layout_call_device(dissimilarity_matrix, ndim, mapping_max_iter, k0, cooling_rate,
                               c_repulsion, relative_epsilon, convergence_counter, initial_positions,
                               verbose, convergence_check_freq, preserve_order,
                               rng: Optional[np.random.Generator] = None, route: Optional[list] = None) -> LayoutCall:
    """`prepare_layout_call` with the matrix work on the GPU (_native.prepare_layout): the same LayoutCall, field for
    field, the same warnings, errors and verbose lines, and the same draws from `rng`.

    The device orders the points where its keys provably sort as spectral_order's do; where it declines
    (order_route 3) spectral_order runs here and the device takes its order.  `route`, when given, receives the
    order_route that was used.  A character matrix goes to `prepare_layout_call` as it is: parsing its strings cell
    by cell on the host costs more than everything the device would then spare, so the simpler form is kept (a
    CodedMatrix, parsed already, goes to the device).  So does every call that `_validate` rejects, for its shape
    or for a scalar argument: the host form raises the reference's message, and nothing goes to the device first.

    Every n x n array of the result is laid out as prepare_layout_call's is -- C-contiguous, whatever the layout of
    the input (a Fortran-contiguous matrix is read where it lies).  A plain array that keeps its order is copied into
    `reordered_matrix` by the same np.array() call that prepare_layout_call copies it with; a CodedMatrix is passed
    through by both.

    Where the device declines (route 3) the matrix is uploaded a second time with the host's order: twice the
    transfer and the first pass, on data that is rare in practice (tied inexact keys, negative or infinite cells)."""
    from . import _native
    front = _device_front(_native.prepare_layout, dissimilarity_matrix, ndim, mapping_max_iter, k0, cooling_rate,
                          c_repulsion, relative_epsilon, convergence_counter, initial_positions, verbose,
                          convergence_check_freq, preserve_order)
    if front is None:
        return prepare_layout_call(dissimilarity_matrix, ndim, mapping_max_iter, k0, cooling_rate, c_repulsion,
                                   relative_epsilon, convergence_counter, initial_positions, verbose,
                                   convergence_check_freq, preserve_order, rng)
    m, codes, own, prep, names, order, init, n = front
    if route is not None:
        route[:] = [prep.info["order_route"]]
    if order is not None:
        order = order.astype(np.intp)
        rcodes = prep.codes_reordered if codes is not None else np.zeros((n, n), dtype=np.int8)
        m = CodedMatrix(np.ascontiguousarray(prep.values_reordered), np.ascontiguousarray(rcodes), names, m.character)
    elif not own:
        m = CodedMatrix(np.array(m.values, dtype=np.float64), m.codes, m.names, False)
    # dense and tdense are symmetric bit for bit: the transpose of a Fortran-ordered one is the C-ordered one
    dense, tdense = prep.dense, prep.tdense
    if not dense.flags.c_contiguous:
        dense, tdense = dense.T, tdense.T
    if init is None:   # the maximum is the same before and after the reordering
        init = _start_walk(prep.info["numeric_max"], n, int(ndim), rng)
    return _layout_call(init, dense, tdense, prep.degrees, prep.edge_i, prep.edge_j, prep.edge_dist, prep.edge_thresh,
                        mapping_max_iter, k0, cooling_rate, c_repulsion, relative_epsilon, convergence_counter,
                        convergence_check_freq, verbose, names, order, m)


def _gate(env_name: str, min_n: Optional[int], dissimilarity_matrix) -> bool:
    """The environment's "0" / "1" where it is set; otherwise: is the matrix of at least min_n points (None: never)?"""
    forced = os.environ.get(env_name)
    if forced in ("0", "1"):
        return forced == "1"
    if min_n is None:
        return False
    v = dissimilarity_matrix.values if isinstance(dissimilarity_matrix, (CodedMatrix, RMatrix)) else dissimilarity_matrix
    shape = getattr(v, "shape", None)
    return shape is not None and len(shape) == 2 and shape[0] >= min_n


def _device_prep_wanted(dissimilarity_matrix) -> bool:
    return _gate("TOPOLOW_DEVICE_PREP", _DEVICE_PREP_MIN_N, dissimilarity_matrix)


def _declines(e) -> bool:
    """Does this _native.NativeError say "not here", so that the host form, or the present route, is to run instead?"""
    from . import _native
    return e.code in (_native.ERR_UNSUPPORTED, _native.ERR_NO_DEVICE)


def _prepare_layout_call_auto(dissimilarity_matrix, *args, **kw) -> LayoutCall:
    """The pre-processing of euclidean_embedding(): on the device for matrices of at least _DEVICE_PREP_MIN_N points
    (TOPOLOW_DEVICE_PREP forces the choice), on the host otherwise and wherever the device form answers
    ERR_UNSUPPORTED or ERR_NO_DEVICE.  Both forms give the same LayoutCall."""
    if _device_prep_wanted(dissimilarity_matrix):
        from . import _native
        try:
            return prepare_layout_call_device(dissimilarity_matrix, *args, **kw)
        except _native.NativeError as e:
            if not _declines(e):
                raise
    return prepare_layout_call(dissimilarity_matrix, *args, **kw)


def post_mae(reordered_matrix, est_distances: np.ndarray) -> float:
    """R/core.R:479-481: mean |as.numeric(D) - est| over every non-NA cell."""
    raw = coded_matrix(reordered_matrix).as_numeric()
    valid = ~np.isnan(raw)
    if not valid.any():
        return float("nan")
    return float(np.mean(np.abs(raw[valid] - est_distances[valid])))


def _fmt_csv_number(x: float) -> str:
    return repr(float(f"{x:.15g}")) if math.isfinite(x) else ("NA" if math.isnan(x) else
                                                               ("Inf" if x > 0 else "-Inf"))


def write_positions_csv(path: str, positions: np.ndarray, names: Optional[Sequence[str]]):
    """utils::write.csv(positions, row.names=TRUE) of an unnamed-column matrix."""
    n, d = positions.shape
    with open(path, "w") as fh:
        fh.write(",".join(['""'] + [f'"V{c + 1}"' for c in range(d)]) + "\n")
        for r in range(n):
            label = names[r] if names is not None else str(r + 1)
            fh.write(",".join([f'"{label}"'] + [_fmt_csv_number(x) for x in positions[r]]) + "\n")


# --------------------------------------------------------------------------------------
# public entry points
# --------------------------------------------------------------------------------------
def device_post(call: LayoutCall, positions: np.ndarray):
    """R/core.R:474-481 in one fused pass on the GPU (_native.post_metrics): (est_distances, mae).
    est_distances is what _native.est_distances returns, bit for bit; mae is post_mae's to 1e-12 (the sum is
    grouped by columns).  One deviation: a cell that holds +-Inf is left out, as the relaxation leaves it out
    (post_mae counts it, and returns Inf or NaN)."""
    from . import _native
    est, sum_abs, count = _native.post_metrics(positions, call.reordered_matrix.as_numeric())
    return est, _native.mae_of(sum_abs, count)


def _finish(call: LayoutCall, native_result, ndim, k0, cooling_rate, c_repulsion,
            write_positions_to_csv, output_dir, verbose, pdist_fn, post_fn=None) -> Topolow:
    positions = np.asarray(native_result.positions, dtype=np.float64)
    if post_fn is None:
        est = pdist_fn(positions)
        mae = post_mae(call.reordered_matrix, est)
    else:
        est, mae = post_fn(call, positions)
    if write_positions_to_csv:
        if output_dir is None or output_dir is _MISSING:
            raise ValueError("An 'output_dir' must be provided when 'write_positions_to_csv' "
                             "is TRUE.")
        os.makedirs(output_dir, exist_ok=True)
        fname = "Positions_dim_%d_k0_%.4f_cooling_%.4f_c_repulsion_%.4f.csv" % (
            int(ndim), k0, cooling_rate, c_repulsion)
        full = os.path.join(output_dir, fname)
        write_positions_csv(full, positions, call.names)
        if verbose:
            print("Positions saved to:", full)
    return Topolow(
        positions=positions, est_distances=est, mae=mae, iter=int(native_result.iterations),
        parameters=dict(ndim=ndim, k0=k0, cooling_rate=cooling_rate, c_repulsion=c_repulsion,
                        method="cpp_exact_full_pairwise"),
        convergence=dict(achieved=bool(native_result.converged),
                         error=float(native_result.final_mae),
                         final_k=float(native_result.final_k)),
        names=call.names, native_info=dict(getattr(native_result, "info", {}) or {}))


def _require(**arguments) -> None:
    """R's error for an argument without a default that the caller left out."""
    for nm, val in arguments.items():
        if val is _MISSING:
            raise TypeError(f'argument "{nm}" is missing, with no default')


def _embed_with(native_fn, pdist_fn, dissimilarity_matrix, ndim, mapping_max_iter, k0,
                cooling_rate, c_repulsion, relative_epsilon, convergence_counter,
                initial_positions, write_positions_to_csv, output_dir, verbose,
                convergence_check_freq, preserve_order, rng=None, post_fn=None,
                prepare_fn=prepare_layout_call) -> Topolow:
    """post_fn(call, positions) -> (est_distances, mae) replaces pdist_fn + post_mae when given; prepare_fn has the
    signature of prepare_layout_call and returns what it returns."""
    _require(k0=k0, cooling_rate=cooling_rate, c_repulsion=c_repulsion)
    call = prepare_fn(dissimilarity_matrix, ndim, mapping_max_iter, k0, cooling_rate,
                      c_repulsion, relative_epsilon, convergence_counter,
                      initial_positions, verbose, convergence_check_freq,
                      preserve_order, rng)
    if verbose:
        print("Starting C++ optimization...")
    import time
    t0 = time.time()
    res = native_fn(call)
    if verbose:
        print("Optimization finished in %.2f seconds." % (time.time() - t0))
    return _finish(call, res, ndim, k0, cooling_rate, c_repulsion, write_positions_to_csv,
                   output_dir, verbose, pdist_fn, post_fn)


# Smallest matrix for which euclidean_embedding() runs resident -- prepare, relax and score from one upload
# (_native.PreparedHandle) -- wherever it prepares on the device at all; None: only with TOPOLOW_RESIDENT=1.
# TOPOLOW_RESIDENT=0 / =1 in the environment forces the choice, read per call.  The resident route returns the bits of
# the present one (tests/test_gpu_resident_embedding.py), so the gate is a matter of time alone; it has not been
# measured on the MI355X yet (tests/study/resident_embedding_timing.py is the measurement), hence None.
_RESIDENT_MIN_N: Optional[int] = None


def _resident_wanted(dissimilarity_matrix) -> bool:
    return _device_prep_wanted(dissimilarity_matrix) and _gate("TOPOLOW_RESIDENT", _RESIDENT_MIN_N, dissimilarity_matrix)


@dataclass
class _ResidentCall:
    """What _finish reads of a LayoutCall, for a call whose arrays never left the device."""
    names: Optional[List[str]] = None


def _embed_resident(dissimilarity_matrix, ndim, mapping_max_iter, k0, cooling_rate, c_repulsion, relative_epsilon,
                    convergence_counter, initial_positions, write_positions_to_csv, output_dir, verbose,
                    convergence_check_freq, preserve_order, rng=None) -> Optional[Topolow]:
    """euclidean_embedding() from one upload: the matrix goes to a _native.PreparedHandle, the relaxation and the
    post-processing read it there; est_distances, the positions and n-sized vectors come back.  The same Topolow as
    prepare_layout_call_device + optimize_layout_exact + device_post give, the same warnings, errors and verbose
    lines, the same draws from `rng` and from the seed stream.

    Returns None -- nothing has been uploaded, drawn or printed by then -- where the present route is to run instead:
    a character matrix, a call that `_validate` rejects (the host form raises the reference's message), a run sharded
    over devices, and a handle that answers ERR_UNSUPPORTED / ERR_NO_DEVICE.  If .optimize itself answers one of the
    two, the present route runs with the start positions and the seed already chosen: nothing is drawn twice."""
    from . import _native
    _require(k0=k0, cooling_rate=cooling_rate, c_repulsion=c_repulsion)
    if _native.options.get("devices") is not None:
        return None
    with ExitStack() as stack:
        def open_handle(*a, **kw):
            stack.close()   # a handle that declined to order is closed before the second one is created
            return stack.enter_context(_native.PreparedHandle(*a, **kw))

        try:
            front = _device_front(open_handle, dissimilarity_matrix, ndim, mapping_max_iter, k0, cooling_rate, c_repulsion,
                                  relative_epsilon, convergence_counter, initial_positions, verbose,
                                  convergence_check_freq, preserve_order)
        except _native.NativeError as e:
            if not _declines(e):
                raise
            return None
        if front is None:
            return None
        _, _, _, handle, names, _, init, n = front
        ndim_i = int(ndim)
        if init is None:   # the maximum is the same before and after the reordering
            init = _start_walk(handle.info["numeric_max"], n, ndim_i, rng)
        init = np.ascontiguousarray(init, dtype=np.float64)

        if verbose:
            print("Starting C++ optimization...")
        import time
        t0 = time.time()
        seed = _native.options.get("seed")
        if seed is None:   # make_options' own draw, made here so that a fallback below runs on the same seed
            seed = int(_native.host_rng().integers(0, 2 ** 63 - 1))
        try:
            res = handle.optimize(init, ndim_i, int(mapping_max_iter), float(k0), float(cooling_rate), float(c_repulsion),
                                  float(relative_epsilon), int(convergence_counter), int(convergence_check_freq),
                                  bool(verbose), seed=seed)
        except _native.NativeError as e:
            if not _declines(e):
                raise
            res = None
        if res is not None:
            if verbose:
                print("Optimization finished in %.2f seconds." % (time.time() - t0))

            def post(_call, positions):
                est, sum_abs, count = handle.post_metrics(positions)
                return est, _native.mae_of(sum_abs, count)

            return _finish(_ResidentCall(names), res, ndim, k0, cooling_rate, c_repulsion, write_positions_to_csv,
                           output_dir, verbose, None, post)

    # .optimize declined after the start positions and the seed were chosen: the present route with both, and with
    # what has been said already -- warnings, the reordering line, the starting line -- not said again
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        call = _prepare_layout_call_auto(dissimilarity_matrix, ndim, mapping_max_iter, k0, cooling_rate, c_repulsion,
                                         relative_epsilon, convergence_counter, init, False, convergence_check_freq,
                                         preserve_order, rng)
    res = _native.optimize_layout_exact_arrays(
        call.initial_positions, call.dissimilarity_matrix, call.threshold_matrix, call.degrees, call.edge_i,
        call.edge_j, call.edge_dist, call.edge_thresh, call.n_iter, call.k0, call.cooling_rate, call.c_repulsion,
        call.relative_epsilon, call.convergence_window, call.convergence_check_freq, bool(verbose), seed=seed)
    if verbose:
        print("Optimization finished in %.2f seconds." % (time.time() - t0))
    return _finish(call, res, ndim, k0, cooling_rate, c_repulsion, write_positions_to_csv, output_dir, verbose,
                   _native.est_distances, device_post)


def euclidean_embedding(dissimilarity_matrix, ndim, mapping_max_iter=1000, k0=_MISSING,
                        cooling_rate=_MISSING, c_repulsion=_MISSING, relative_epsilon=1e-4,
                        convergence_counter=5, initial_positions=None,
                        write_positions_to_csv=False, output_dir=_MISSING, verbose=False,
                        convergence_check_freq=3, preserve_order=False) -> Topolow:
    """Drop-in for the reference's `euclidean_embedding()` (R/core.R:184-197); the native
    relaxation runs on the MI355X through libtopolow_relax.so (no CPU fallback)."""
    from . import _native
    if _resident_wanted(dissimilarity_matrix):
        out = _embed_resident(dissimilarity_matrix, ndim, mapping_max_iter, k0, cooling_rate, c_repulsion,
                              relative_epsilon, convergence_counter, initial_positions, write_positions_to_csv,
                              output_dir, verbose, convergence_check_freq, preserve_order, _native.host_rng())
        if out is not None:
            return out
    return _embed_with(_native.optimize_layout_exact, _native.est_distances,
                       dissimilarity_matrix, ndim, mapping_max_iter, k0, cooling_rate,
                       c_repulsion, relative_epsilon, convergence_counter, initial_positions,
                       write_positions_to_csv, output_dir, verbose, convergence_check_freq,
                       preserve_order, _native.host_rng(), post_fn=device_post,
                       prepare_fn=_prepare_layout_call_auto)


def create_topolow_map(distance_matrix, ndim, mapping_max_iter=1000, k0=_MISSING,
                       cooling_rate=_MISSING, c_repulsion=_MISSING, relative_epsilon=1e-4,
                       convergence_counter=3, initial_positions=None,
                       write_positions_to_csv=False, output_dir=_MISSING,
                       verbose=False) -> Topolow:
    """Deprecated alias (R/core.R:616-664): warns, then forwards with convergence_counter
    defaulting to 3 and the default convergence_check_freq / preserve_order."""
    warnings.warn("`create_topolow_map()` was deprecated in topolow 2.0.0.\n"
                  "Please use `euclidean_embedding()` instead.\n"
                  "i The new function provides the same functionality with improvements:\n"
                  "* Parameter name: 'distance_matrix' --> 'dissimilarity_matrix'\n"
                  "* Enhanced matrix reordering for better optimization",
                  DeprecationWarning, stacklevel=2)
    if write_positions_to_csv and output_dir is _MISSING:
        output_dir = os.getcwd()
        warnings.warn("output_dir not specified, using current working directory", UserWarning,
                      stacklevel=2)
    return euclidean_embedding(
        dissimilarity_matrix=distance_matrix, ndim=ndim, mapping_max_iter=mapping_max_iter,
        k0=k0, cooling_rate=cooling_rate, c_repulsion=c_repulsion,
        relative_epsilon=relative_epsilon, convergence_counter=convergence_counter,
        initial_positions=initial_positions, write_positions_to_csv=write_positions_to_csv,
        output_dir=output_dir if write_positions_to_csv else None, verbose=verbose)
