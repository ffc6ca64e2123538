"""Connected subsamples of a dissimilarity matrix: the twins of the reference's `check_matrix_connectivity`
(R/utils.R:199-253, over the adjacency of `analyze_network_structure`, R/diagnostics.R:442-468) and
`subsample_dissimilarity_matrix` (R/utils.R:321-463) -- what its parameter search runs on instead of a large matrix
(`opt_subsample`, R/adaptive_sampling.R).

Each function has a host form (plain NumPy, no graph library) and, with `handle=` an open `_native.PreparedHandle` of
the matrix, a device form that answers from what the handle keeps on the GPU: the components come from
`handle.connectivity`, the connected draw becomes a child handle (`handle.subsample`) without a second upload.  The
device form is taken exactly when a handle is passed.

Indices are 0-based here (`selected_indices`), 1-based in R."""
import math
import warnings
from typing import Any, Dict, Optional

import numpy as np

from . import core

_SPARSE = ("Network is connected but sparse (%.1f%% complete). This may lead to poor optimization. "
           "Consider using more data points.")
_FAILED = ("Failed to obtain a connected subsample after %d attempts.\n"
           "  Final sample size tried: %d (started at %d)\n"
           "  Original matrix size: %d\n"
           "  Last attempt had %s components with %.1f%% completeness\n\n"
           "Possible solutions:\n"
           "  1. Increase opt_subsample (current: %d)\n"
           "  2. Reduce number of CV folds\n"
           "  3. Use full dataset (opt_subsample = NULL)\n"
           "  4. Check if your data has inherent disconnected groups")


def _matrix(dissimilarity_matrix, at_least_2: bool) -> core.CodedMatrix:
    """The reference's input checks (R/utils.R:202-210, 331-337), its stop() texts as ValueError."""
    m = core.coded_matrix(dissimilarity_matrix)
    if m is None or np.ndim(m.values) != 2:
        raise ValueError("dissimilarity_matrix must be a matrix")
    if m.values.shape[0] != m.values.shape[1]:
        raise ValueError("dissimilarity_matrix must be square")
    if at_least_2 and m.values.shape[0] < 2:
        raise ValueError("dissimilarity_matrix must have at least 2 points")
    return m


def component_labels(values: np.ndarray):
    """The components of the measurement graph of `values` (NaN = NA) on the host: (labels, n_cells).  {a, b}, a != b,
    is an edge iff cell (a, b) or cell (b, a) is not NaN -- `!is.na` and igraph's mode = "undirected"; the diagonal
    makes no edge.  labels[q] is the smallest index of q's component (what topolow_layout_prep_connectivity returns);
    n_cells the non-NaN off-diagonal cells over both triangles, `sum(adjacency)`.
    Repeated min-label with pointer jumping: a round gives every point the smallest label among itself and its
    neighbours, hooks its old label to that, and flattens; the rounds end when none changes anything."""
    adj = ~np.isnan(np.asarray(values, dtype=np.float64))
    n = adj.shape[0]
    np.fill_diagonal(adj, False)
    n_cells = int(adj.sum())
    adj |= adj.T
    lab = np.arange(n, dtype=np.int64)
    rows = max(1, (1 << 24) // max(n, 1))          # 16 M cells of the masked label table at a time
    while True:
        low = lab.copy()
        for r0 in range(0, n, rows):
            block = np.where(adj[r0:r0 + rows], lab[None, :], n)
            np.minimum(low[r0:r0 + rows], block.min(axis=1), out=low[r0:r0 + rows])
        if np.array_equal(low, lab):
            return lab.astype(np.int32), n_cells
        hooked = low.copy()
        np.minimum.at(hooked, lab, low)            # the old label of a point follows it down
        while True:
            up = hooked[hooked]
            if np.array_equal(up, hooked):
                break
            hooked = up
        lab = hooked


def _summary(n_components: int, n_cells: int, n: int, min_completeness: float) -> Dict[str, Any]:
    completeness = n_cells / (n * (n - 1))
    connected = n_components == 1
    if connected and completeness < min_completeness:
        warnings.warn(_SPARSE % (completeness * 100))
    return dict(is_connected=connected, n_components=int(n_components), completeness=completeness, n_points=int(n),
                n_measurements=n_cells / 2)


def check_matrix_connectivity(dissimilarity_matrix, min_completeness: float = 0.1, handle=None) -> Dict[str, Any]:
    """`check_matrix_connectivity` (R/utils.R:199-253): is the graph of the measured pairs connected?  Returns the
    reference's five fields: is_connected, n_components, completeness, n_points, n_measurements (sum(adjacency) / 2,
    so a pair measured in one triangle only counts one half).  A connected graph below `min_completeness` warns with
    the reference's text; the three input errors are its stop() texts as ValueError.
    `handle`: an open _native.PreparedHandle of this matrix -- the components and the cell count then come from the
    device (handle.connectivity()), and the matrix argument is used for nothing but the input checks."""
    m = _matrix(dissimilarity_matrix, True)
    n = m.values.shape[0]
    if handle is not None:
        if handle.n != n:
            raise ValueError("handle holds a matrix of another size")
        n_components, n_cells, _ = handle.connectivity()
    else:
        labels, n_cells = component_labels(m.values)
        n_components = int(np.sum(labels == np.arange(n)))
    return _summary(n_components, n_cells, n, min_completeness)


def _gather(m: core.CodedMatrix, source, idx: np.ndarray):
    """source[idx, idx] with the names carried: the caller's own cells (strings stay strings)."""
    r = core._as_rmatrix(source)
    vals = (r.values if r is not None else m.values)[np.ix_(idx, idx)]
    names = [m.names[q] for q in idx] if m.names is not None else None
    return (core.RMatrix(vals, names) if names is not None else vals), names


def subsample_dissimilarity_matrix(dissimilarity_matrix, sample_size, max_attempts: int = 5,
                                   min_completeness: float = 0.1, rng: Optional[np.random.Generator] = None,
                                   verbose: bool = False, preserve_order: bool = False, handle=None) -> Dict[str, Any]:
    """`subsample_dissimilarity_matrix` (R/utils.R:321-463): `floor(sample_size)` points drawn at random whose
    submatrix is a connected graph, in at most `max_attempts` draws.  Returns the reference's seven fields:
    subsampled_matrix (an RMatrix where the input has names, else an array), selected_indices (0-based),
    selected_names, is_connected, n_components, completeness, attempt_number.  sample_size >= n returns the matrix
    itself, whatever its connectivity, as the reference does.  `preserve_order` sorts the drawn indices.  No connected
    draw: ValueError with the reference's text.  The verbose lines are the reference's (its "Using full matrix" line
    and the component count of its final error are formatted as they were evidently meant: as written there, sprintf
    is handed a string for a %d).

    The draw is `rng.choice(n, size, replace=False)` on a NumPy generator, as cv.make_folds draws: the subsamples are
    not those of R's sample() under the same seed -- reproducing R's stream is out of scope; `rng` replaces
    `random_seed`.

    `handle`: an open _native.PreparedHandle of this matrix (the parent).  Every attempt is then tested on the device
    (handle.connectivity(indices)) before anything is gathered; only the connected attempt becomes a child handle
    (handle.subsample(indices, preserve_order=True): its labels are the caller's, as cv.likelihood_sweep(...,
    path="resident", handle=child) takes it), returned under the extra key "handle" -- the caller closes it.  With
    sample_size >= n the child is a copy of the whole parent.  subsampled_matrix is the host gather either way.  An
    error of the device is raised, not counted as a failed attempt."""
    m = _matrix(dissimilarity_matrix, False)
    n = m.values.shape[0]
    if isinstance(sample_size, bool) or not isinstance(sample_size, (int, float, np.integer, np.floating)) \
            or not sample_size >= 2:
        raise ValueError("sample_size must be a numeric value >= 2")
    if handle is not None and handle.n != n:
        raise ValueError("handle holds a matrix of another size")
    sample_size = int(math.floor(sample_size))
    if sample_size >= n:
        if verbose:
            print("Requested sample_size (%d) >= matrix size (%d). Using full matrix." % (sample_size, n))
        con = check_matrix_connectivity(dissimilarity_matrix, min_completeness, handle=handle)
        out = dict(subsampled_matrix=dissimilarity_matrix, selected_indices=np.arange(n),
                   selected_names=list(m.names) if m.names is not None else None, is_connected=con["is_connected"],
                   n_components=con["n_components"], completeness=con["completeness"], attempt_number=1)
        if handle is not None:
            out["handle"] = handle.subsample(None, preserve_order=True)
        return out
    if rng is None:
        from . import _native
        rng = _native.host_rng()
    if not hasattr(rng, "choice"):   # R-stream generator: the draw uses a NumPy stream seeded from it
        rng = np.random.default_rng(rng.integers(0, 2 ** 53))
    con = None
    for attempt in range(1, int(max_attempts) + 1):
        if verbose and attempt > 1:
            print("  Attempt %d/%d..." % (attempt, max_attempts))
        idx = rng.choice(n, size=sample_size, replace=False)
        if preserve_order:
            idx = np.sort(idx)
        if handle is not None:
            n_components, n_cells, _ = handle.connectivity(idx)
        else:
            labels, n_cells = component_labels(m.values[np.ix_(idx, idx)])
            n_components = int(np.sum(labels == np.arange(sample_size)))
        con = _summary(n_components, n_cells, sample_size, min_completeness)
        if con["is_connected"]:
            if verbose:
                print("  [OK] Connected subsample obtained (attempt %d, size %d, %.1f%% complete)"
                      % (attempt, sample_size, con["completeness"] * 100))
            sub, names = _gather(m, dissimilarity_matrix, idx)
            out = dict(subsampled_matrix=sub, selected_indices=idx, selected_names=names, is_connected=True,
                       n_components=con["n_components"], completeness=con["completeness"], attempt_number=attempt)
            if handle is not None:
                out["handle"] = handle.subsample(idx, preserve_order=True)
            return out
        if verbose:
            print("  X Not connected (%s components, %.1f%% complete)" % (con["n_components"], con["completeness"] * 100))
    raise ValueError(_FAILED % (max_attempts, sample_size, sample_size, n, con["n_components"] if con else -1,
                                (con["completeness"] if con else 0.0) * 100, sample_size))
