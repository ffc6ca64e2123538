"""Degrees and pruning of a sparse dissimilarity matrix: the twins of the reference's `analyze_network_structure`
(R/diagnostics.R:434-475) and `prune_sparse_matrix` (R/data_preprocessing.R:1225-1503) -- what its parameter search
tells users to run first on large, sparse data ("Consider pruning the dataset first", R/adaptive_sampling.R:305-341).

Each function has a host form (plain NumPy: the specification) and, with `handle=` an open `_native.PreparedHandle` of
the matrix, a device form that answers from what the handle keeps on the GPU (`handle.degrees`, `handle.prune`,
`handle.connectivity`, `handle.subsample`).  The device form is taken exactly when a handle is passed; both forms run
the same statements below around the one step that differs, so they warn, print and return alike.

Indices are 0-based here (`kept_indices`, `removed_indices`), 1-based in R."""
import warnings
from typing import Any, Dict, Iterator, Optional

import numpy as np

from . import core, subsample

CONVERGED, MIN_POINTS, MAX_ITERATIONS, ALL_REMOVED = 1, 2, 3, 4   # stop_reason; TOPOLOW_PRUNE_* of the C header
MAX_ATTEMPTS = 10

_RULE = "=" * 80


def _adjacency(values: np.ndarray) -> np.ndarray:
    """`!is.na` with the diagonal False: threshold-coded cells and +-Inf are measured."""
    adj = ~np.isnan(np.asarray(values, dtype=np.float64))
    np.fill_diagonal(adj, False)
    return adj


def _as_given(x):
    """(values, names) of a matrix-like as it lies, nothing copied or parsed; (None, None) for what is no matrix."""
    if isinstance(x, core.CodedMatrix):
        return x.values, x.names
    r = core._as_rmatrix(x)
    return (None, None) if r is None else (r.values, r.names)


def analyze_network_structure(dissimilarity_matrix, handle=None, want_adjacency: Optional[bool] = None) -> Dict[str, Any]:
    """`analyze_network_structure` (R/diagnostics.R:434-475).  Returns the reference's three fields:
      adjacency      bool n x n, `!is.na` with the diagonal False.  With a handle it is None unless
                     want_adjacency=True (it is then made on the host); without one it is always made.
      connectivity   dict(node = the names or "Node1".., degree (int64), completeness = degree / (n - 1))
      summary        dict(n_points, n_measurements = sum(adjacency) / 2, completeness = sum(adjacency) / (n (n - 1)))
    degree[i] counts along matrix ROW i (`rowSums`); threshold-coded cells ("<40", ">1280") and +-Inf count as
    measured, as in `subsample.component_labels`.  The two input errors are the reference's stop() texts as ValueError.
    `handle`: an open _native.PreparedHandle of this matrix -- the degrees come from the device (handle.degrees())."""
    values, names = _as_given(dissimilarity_matrix)
    if values is None or np.ndim(values) != 2 or values.shape[0] != values.shape[1]:
        raise ValueError("Input must be a square matrix")
    n = values.shape[0]
    if n < 2:
        raise ValueError("Matrix must have at least 2 rows/columns")
    names = list(names) if names is not None else ["Node%d" % (q + 1) for q in range(n)]
    adjacency = None
    if handle is not None:                           # the matrix is neither copied nor parsed unless its adjacency is asked for
        if handle.n != n:
            raise ValueError("handle holds a matrix of another size")
        degree, n_cells = handle.degrees()
        degree = degree.astype(np.int64)
        if want_adjacency:
            adjacency = _adjacency(core.coded_matrix(dissimilarity_matrix).values)
    else:
        adjacency = _adjacency(core.coded_matrix(dissimilarity_matrix).values)
        degree = adjacency.sum(axis=1).astype(np.int64)
        n_cells = int(degree.sum())
    return dict(adjacency=adjacency,
                connectivity=dict(node=names, degree=degree, completeness=degree / (n - 1)),
                summary=dict(n_points=n, n_measurements=n_cells / 2, completeness=n_cells / (n * (n - 1))))


def _completeness(cells: int, size: int) -> float:
    """cells / (s (s - 1)) in double, one division of two exact integers -- the C entry computes the same bits, so a
    `>=` against a target cannot differ between the routes.  Fewer than 2 points: NaN (R's 0 / 0)."""
    return cells / (size * (size - 1)) if size >= 2 else float("nan")


def _rounds(adj: np.ndarray, min_connections, max_iterations, min_points, verbose: bool) -> Dict[str, Any]:
    """The loop of R/data_preprocessing.R:1371-1415 on the adjacency: one attempt's record.  count[i] = the measured
    cells (i, c), c != i kept, along row i; the counts are kept up to date by subtracting the removed columns, which
    gives the integers a recount of the kept submatrix gives."""
    n = adj.shape[0]
    keep = np.ones(n, dtype=bool)
    counts = adj.sum(axis=1).astype(np.int64)
    size, iteration, last_remove, reason = n, 0, 0, 0
    while reason == 0 and iteration < max_iterations:
        iteration += 1                               # counted before the test
        poor = keep & (counts < min_connections)
        last_remove = int(poor.sum())
        if last_remove == 0:
            reason = CONVERGED
            if verbose:
                print("Iteration %d: All %d points have >= %d connections" % (iteration, size, min_connections))
        elif size - last_remove < min_points:
            reason = MIN_POINTS                      # removes nothing: the round's candidates stay in
        else:
            keep &= ~poor
            counts -= adj[:, poor].sum(axis=1)
            size -= last_remove
            if verbose and iteration % 10 == 0:
                print("Iteration %d: Removed %d points, %d remaining" % (iteration, last_remove, size))
            if size == 0:
                reason = ALL_REMOVED
    return dict(kept=keep, iterations=iteration, stop_reason=reason or MAX_ITERATIONS, last_remove=last_remove,
                final_size=size, final_cells=int(counts[keep].sum()), min_connections=min_connections)


def _host_attempts(adj, thresholds, max_iterations, min_points, verbose) -> Iterator[Dict[str, Any]]:
    for threshold in thresholds:                     # lazily: the caller stops asking when the search ends
        yield _rounds(adj, threshold, max_iterations, min_points, verbose)


def _device_attempts(kept, info, min_connections, verbose) -> Iterator[Dict[str, Any]]:
    """The attempts of ONE handle.prune call (the search runs inside it), as the records _rounds gives; only the last
    one carries the mask.  min_connections: the caller's threshold, or None for the search's 4, 6, 8, ..."""
    last = info["attempts"] - 1
    for a in range(info["attempts"]):
        rec = dict(kept=kept if a == last else None, iterations=info["attempt_iterations"][a],
                   stop_reason=info["attempt_stop_reason"][a], last_remove=info["attempt_last_remove"][a],
                   final_size=info["attempt_final_size"][a], final_cells=info["attempt_final_cells"][a],
                   min_connections=min_connections if min_connections is not None else 4 + 2 * a)
        if verbose and rec["stop_reason"] == CONVERGED:
            print("Iteration %d: All %d points have >= %d connections"
                  % (rec["iterations"], rec["final_size"], rec["min_connections"]))
        yield rec


def _attempt_warnings(rec, max_iterations, min_points) -> None:
    """What one run of the loop warns and raises, in the reference's order (:1393-1397, :1412-1414, :1417-1419)."""
    if rec["stop_reason"] == MIN_POINTS:
        warnings.warn("Stopping at iteration %d: removing %d points would leave only %d points (min_points = %d)"
                      % (rec["iterations"], rec["last_remove"], rec["final_size"] - rec["last_remove"], min_points))
    if rec["stop_reason"] == ALL_REMOVED:
        raise ValueError("All points removed during pruning. Try lower min_connections.")
    if rec["iterations"] >= max_iterations:
        warnings.warn("Reached max_iterations (%d) before convergence" % max_iterations)


def _whole(x: float) -> str:
    return "%d" % x if float(x).is_integer() else repr(x)


def _connectivity(m, kept_idx, rec, min_completeness, handle):
    """check_matrix_connectivity of the pruned matrix: (is_connected, n_components), its sparse warning included."""
    size = rec["final_size"]
    if size < 2:
        raise ValueError("dissimilarity_matrix must have at least 2 points")
    if handle is not None:
        n_components, n_cells, _ = handle.connectivity(kept_idx)
    else:
        labels, n_cells = subsample.component_labels(m.values[np.ix_(kept_idx, kept_idx)])
        n_components = int(np.sum(labels == np.arange(size)))
    con = subsample._summary(n_components, n_cells, size, min_completeness)
    return con["is_connected"], con["n_components"]


def prune_sparse_matrix(dissimilarity_matrix, min_connections=4, target_completeness=None, max_iterations=100,
                        min_points=10, ensure_connected: bool = True, verbose: bool = True, handle=None,
                        want_matrix: bool = True) -> Dict[str, Any]:
    """`prune_sparse_matrix` (R/data_preprocessing.R:1225-1503): remove, round after round, every point with fewer
    than `min_connections` measurements among the points still kept, until a round removes nothing.  The control flow
    is the reference's, statement for statement:
      - its validation texts as ValueError;
      - the loop: `iterations` is counted before the test (a run that converges reports the round that found nothing
        to remove); the min_points stop removes nothing and warns; "Reached max_iterations" warns whenever
        iterations >= max_iterations on exit, even if that round converged; "All points removed during pruning"
        (ValueError) is reachable with min_points = 0;
      - `target_completeness`: the search as the reference's CODE has it, not its doc comment -- thresholds 4, 6, 8, ...
        (increment 2), at most 10 attempts, each from the original matrix without a connectivity check; an attempt with
        final_completeness >= target is returned (after a connectivity check with min_completeness = target when
        ensure_connected); one with final_size <= min_points is returned with a warning; otherwise ValueError
        "Could not reach target completeness after maximum attempts".  `min_connections` is not used then;
      - `ensure_connected`: check_matrix_connectivity of the result (min_completeness = 0.01), a warning on a
        disconnected result; stats gain is_connected and n_components.
    Returns pruned_matrix (an RMatrix where the input has names), kept_indices and removed_indices (0-based, ascending),
    kept_names, and stats: original_size, final_size, points_removed, percent_removed, original_completeness,
    final_completeness, original_measurements, final_measurements (cells / 2: a pair measured in one triangle only
    counts one half), completeness_increase, iterations, min_connections_used.  Completeness is
    cells / (s (s - 1)) in double, cells the non-NaN off-diagonal cells over both triangles.  Warnings go through
    warnings.warn and the verbose lines through print, with the reference's texts.

    One deliberate deviation.  The reference counts a row's connections with `sum(!is.na(row) & row != row[1])`: it
    compares every cell with the row's FIRST cell, not with the diagonal.  Where that cell is measured and its value
    does not recur in the row this is the number of measured off-diagonal cells; where it is NA the count is NA and R
    carries NA into the mask and the indices; where the value recurs (common with titre-derived distances) it
    undercounts.  Implemented here is what its documentation says ("Counting observed measurements per point"):
    count[i] = #{c != i, c still kept : cell (i, c) is not NaN}, along matrix row i -- analyze_network_structure's
    degree restricted to the kept points.  Threshold-coded cells and +-Inf count as measured; the matrix need not be
    symmetric.  (An attempt that ends with one point has completeness NaN, R's 0 / 0, which compares False.)

    `handle`: an open _native.PreparedHandle of this matrix.  Mask and stats then come from the device
    (handle.prune: the whole search in one call), `ensure_connected` runs through handle.connectivity(kept), and the
    pruned matrix is also returned as a child handle under the extra key "handle" (handle.subsample(kept,
    preserve_order=True)), which the caller closes.  pruned_matrix is still filled by the host gather;
    want_matrix=False skips it (None).  Of the per-iteration verbose lines the device form prints the converged one
    only.  An error of the device is raised, never turned into a warning."""
    values, names = _as_given(dissimilarity_matrix)
    if values is None or np.ndim(values) != 2:
        raise ValueError("dissimilarity_matrix must be a matrix")
    if values.shape[0] != values.shape[1]:
        raise ValueError("dissimilarity_matrix must be square")
    n = values.shape[0]
    if n < min_points:
        raise ValueError("Matrix size (%d) is smaller than min_points (%d)" % (n, min_points))
    numeric = (int, float, np.integer, np.floating)
    if isinstance(min_connections, bool) or not isinstance(min_connections, numeric) or not min_connections >= 1:
        raise ValueError("min_connections must be a positive integer")
    if target_completeness is not None:
        if isinstance(target_completeness, bool) or not isinstance(target_completeness, numeric) \
                or not 0 < target_completeness <= 1:
            raise ValueError("target_completeness must be between 0 and 1")
    if handle is not None and handle.n != n:
        raise ValueError("handle holds a matrix of another size")

    # the host form parses the matrix (strings, codes) once; with a handle it is used as it lies, for names and the gather
    m = core.coded_matrix(dissimilarity_matrix) if handle is None else core.RMatrix(values, names)
    adj = _adjacency(m.values) if handle is None else None
    if handle is not None:
        searching = target_completeness is not None
        kept, info = handle.prune(4 if searching else min_connections, target_completeness, max_iterations, min_points)
        attempts = _device_attempts(kept, info, None if searching else min_connections, verbose and not searching)
        original_cells = info["original_cells"]
    else:
        original_cells = int(adj.sum())
        if target_completeness is None:
            attempts = _host_attempts(adj, [min_connections], max_iterations, min_points, verbose)
        else:
            attempts = _host_attempts(adj, range(4, 4 + 2 * MAX_ATTEMPTS, 2), max_iterations, min_points, False)
    original_measurements = original_cells / 2
    original_completeness = _completeness(original_cells, n)
    if verbose:
        print("\n%s\nSPARSE MATRIX PRUNING\n%s" % (_RULE, _RULE))
        print("\nOriginal matrix: %d x %d" % (n, n))
        print("Original measurements: %s" % _whole(original_measurements))
        print("Original completeness: %.3f (%.1f%%)" % (original_completeness, original_completeness * 100))

    def result(rec, checked, quiet):
        """The reference's :1424-1502 for one finished attempt; `checked`: min_completeness of the connectivity
        check, or None for none; `quiet`: the inner call of the search prints nothing."""
        kept_idx = np.flatnonzero(rec["kept"])
        removed_idx = np.flatnonzero(~np.asarray(rec["kept"], dtype=bool))
        size = rec["final_size"]
        final_completeness = _completeness(rec["final_cells"], size)
        with np.errstate(divide="ignore", invalid="ignore"):
            increase = float(np.float64(final_completeness) / np.float64(original_completeness))
        stats = dict(original_size=n, final_size=size, points_removed=len(removed_idx),
                     percent_removed=len(removed_idx) / n * 100, original_completeness=original_completeness,
                     final_completeness=final_completeness, original_measurements=original_measurements,
                     final_measurements=rec["final_cells"] / 2, completeness_increase=increase,
                     iterations=rec["iterations"], min_connections_used=rec["min_connections"])
        if checked is not None:
            if not quiet:
                if verbose:
                    print("\nChecking connectivity...")
                try:
                    stats["is_connected"], stats["n_components"] = _connectivity(m, kept_idx, rec, checked, handle)
                except ValueError as e:              # the reference's tryCatch around its own check's stop()
                    warnings.warn("Connectivity check failed: %s" % e)
                    stats["is_connected"], stats["n_components"] = None, None
                if stats["is_connected"] is False:
                    warnings.warn("Final matrix has %d disconnected components. Consider increasing min_connections."
                                  % stats["n_components"])
            else:
                stats["is_connected"], stats["n_components"] = _connectivity(m, kept_idx, rec, checked, handle)
        pruned, names = (None, [m.names[q] for q in kept_idx] if m.names is not None else None)
        if want_matrix or handle is None:
            pruned, names = subsample._gather(m, dissimilarity_matrix, kept_idx)
        if verbose and not quiet:
            print("\n%s\nPRUNING COMPLETE\n%s" % (_RULE, _RULE))
            print("\nFinal matrix: %d x %d (%d points removed, %.1f%%)"
                  % (size, size, stats["points_removed"], stats["percent_removed"]))
            print("Final measurements: %s" % _whole(stats["final_measurements"]))
            print("Final completeness: %.3f (%.1f%%) - %.1fx increase"
                  % (final_completeness, final_completeness * 100, increase))
            if stats.get("is_connected") is not None:
                print("Connected: %s%s" % ("TRUE" if stats["is_connected"] else "FALSE",
                                           "" if stats["is_connected"] else " (%d components)" % stats["n_components"]))
            print()
        out = dict(pruned_matrix=pruned, kept_indices=kept_idx, kept_names=names, removed_indices=removed_idx,
                   stats=stats)
        if handle is not None:
            out["handle"] = handle.subsample(kept_idx, preserve_order=True)
        return out

    if target_completeness is None:
        if verbose:
            print("\nPruning with min_connections = %s\n%s" % (_whole(min_connections), "-" * 80))
        rec = next(iter(attempts))
        _attempt_warnings(rec, max_iterations, min_points)
        return result(rec, 0.01 if ensure_connected else None, False)

    if verbose:
        print("\nUsing adaptive thresholding to reach %.1f%% completeness..." % (target_completeness * 100))
    for number, rec in enumerate(attempts, start=1):
        if verbose:
            print("\nAttempt %d: min_connections = %d" % (number, rec["min_connections"]))
        _attempt_warnings(rec, max_iterations, min_points)
        final_completeness = _completeness(rec["final_cells"], rec["final_size"])
        if final_completeness >= target_completeness:
            if verbose:
                print("  Target reached: %.3f >= %.3f" % (final_completeness, target_completeness))
            return result(rec, target_completeness if ensure_connected else None, True)
        if rec["final_size"] <= min_points:
            warnings.warn("Reached min_points (%d) before target completeness. Final completeness: %.3f, Target: %.3f"
                          % (min_points, final_completeness, target_completeness))
            return result(rec, None, True)
        if verbose:
            print("  Completeness: %.3f < %.3f, increasing threshold..." % (final_completeness, target_completeness))
    raise ValueError("Could not reach target completeness after maximum attempts")
