"""Plot coordinates of a finished map: the reference's reduce_dimensions (R/visualization.R:544-611) in its default
configuration -- PCA to two components, scaled to match the original distances (scale_to_original_distances,
:624-640) -- and what plot_temporal_mapping computes from them before it draws (:999-1001, :1157-1218).

The PCA is an n x ndim problem and stays on the host.  The scale step is where the reference forms two n x n
distance matrices: `scale_to_original_distances(..., device=None)` does the same in NumPy and is the specification;
with a device it runs topolow_scale_to_original_distances (csrc/relax_reduce.h), which forms no matrix and has no host
fallback.  Both minimise with Brent's fmin, the algorithm behind R's optimize; the host's copy is `brent_fmin` below.
UMAP and t-SNE need packages this project does not carry.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _native
from .velocity import kernel_velocity, pair_difference_bandwidth, silverman_bandwidth

_EPS = float(np.finfo(np.float64).eps)


@dataclass
class DimReductionConfig:
    """new_dim_reduction_config (:361-410) for the PCA path: pca_tol and rank are its pca_params tol and rank.."""
    method: str = "pca"
    n_components: int = 2
    scale: bool = True
    center: bool = True
    pca_tol: Optional[float] = math.sqrt(_EPS)
    rank: Optional[int] = None

    def __post_init__(self):
        if self.method not in ("pca", "umap", "tsne"):
            raise ValueError("method must be one of 'pca', 'umap', 'tsne'")
        if self.method != "pca":
            raise NotImplementedError(f"method '{self.method}' needs a package this project does not carry "
                                      "(the reference calls umap::umap / Rtsne::Rtsne); only 'pca' is implemented")
        if isinstance(self.n_components, bool) or not isinstance(self.n_components, (int, float, np.integer, np.floating)) \
                or not self.n_components > 0:
            raise ValueError("n_components must be a number > 0")
        if self.n_components != int(self.n_components):
            raise ValueError("n_components must be a whole number")
        self.n_components = int(self.n_components)
        if not isinstance(self.scale, (bool, np.bool_)) or not isinstance(self.center, (bool, np.bool_)):
            raise ValueError("scale and center must be logical")
        if self.pca_tol is not None and not (isinstance(self.pca_tol, (int, float)) and math.isfinite(self.pca_tol)):
            raise ValueError("pca_tol must be None or a finite number")
        if self.rank is not None and not (isinstance(self.rank, (int, np.integer)) and self.rank > 0):
            raise ValueError("rank must be None or a whole number > 0")


def _matrix(a, what):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError(f"{what} must be a matrix with one row per point")
    return a


def pca_scores(X, config: Optional[DimReductionConfig] = None) -> np.ndarray:
    """prcomp(x, center = TRUE, scale. = FALSE, tol =, rank. =)$x[, 1:n_components]: the scores of the centred matrix
    on its first principal axes, from the SVD of the centred matrix (as prcomp does it).  A component whose standard
    deviation is <= tol * the first one's is dropped, and asking for more components than remain raises ValueError
    (R: subscript out of bounds).  reduce_dimensions always centres (:561-565), so config.center is not read here.
    The sign of a column is the one numpy.linalg.svd returns; the reference's is LAPACK's too and carries no meaning:
    two builds of either may flip a column."""
    config = DimReductionConfig() if config is None else config
    X = _matrix(X, "X")
    n, p = X.shape
    if n < 2:
        raise ValueError("need at least 2 points")
    if not np.isfinite(X).all():
        raise ValueError("X must be finite")
    centred = X - X.mean(axis=0)
    _, sv, vt = np.linalg.svd(centred, full_matrices=False)
    keep = min(n, p) if config.rank is None else min(int(config.rank), n, p)
    if config.pca_tol is not None:
        sdev = sv / math.sqrt(n - 1)
        keep = min(keep, int((sdev > sdev[0] * max(0.0, config.pca_tol)).sum()))
    if config.n_components > keep:
        raise ValueError(f"{config.n_components} components asked for, {keep} remain (subscript out of bounds)")
    return centred @ vt[:config.n_components].T


def brent_fmin(f, lower: float, upper: float, tol: float):
    """Brent's fmin (Algorithms for Minimization without Derivatives, 1973, ch. 5), the algorithm behind R's optimize:
    golden section with parabolic steps, eps = sqrt(machine epsilon), tol1 = eps |x| + tol / 3.  Returns (x, f(x),
    trace) with trace the list of evaluated (s, f(s)) pairs in order; f(x) is the smallest value evaluated.  The
    library's copy (csrc/topolow_reduce.hip) takes the same steps."""
    if not (math.isfinite(lower) and math.isfinite(upper) and math.isfinite(tol)):
        raise ValueError("lower, upper and tol must be finite")
    if not lower < upper:
        raise ValueError("needs lower < upper")
    if not tol > 0:
        raise ValueError("tol must be > 0")
    trace = []

    def evaluate(s):
        value = float(f(s))
        trace.append((s, value))
        return value

    golden = 0.5 * (3.0 - math.sqrt(5.0))
    eps, tol3 = math.sqrt(_EPS), tol / 3.0
    a, b = float(lower), float(upper)
    x = w = v = a + golden * (b - a)
    d = e = 0.0
    fx = fw = fv = evaluate(x)
    while True:
        xm = 0.5 * (a + b)
        tol1 = eps * abs(x) + tol3
        t2 = 2.0 * tol1
        if abs(x - xm) <= t2 - 0.5 * (b - a):
            break
        p = q = r = 0.0
        if abs(e) > tol1:                                   # fit a parabola through x, w, v
            r = (x - w) * (fx - fv)
            q = (x - v) * (fx - fw)
            p = (x - v) * q - (x - w) * r
            q = 2.0 * (q - r)
            if q > 0.0:
                p = -p
            else:
                q = -q
            r, e = e, d
        if abs(p) >= abs(0.5 * q * r) or p <= q * (a - x) or p >= q * (b - x):
            e = b - x if x < xm else a - x                  # a golden-section step into the larger part
            d = golden * e
        else:
            d = p / q                                       # the parabola's step
            u = x + d
            if u - a < t2 or b - u < t2:                    # not too close to the ends
                d = tol1 if x < xm else -tol1
        # f is never evaluated closer than tol1 to x
        u = x + d if abs(d) >= tol1 else (x + tol1 if d > 0.0 else x - tol1)
        fu = evaluate(u)
        if fu <= fx:
            if u < x:
                b = x
            else:
                a = x
            v, fv, w, fw, x, fx = w, fw, x, fx, u, fu
        else:
            if u < x:
                a = u
            else:
                b = u
            if fu <= fw or w == x:
                v, fv, w, fw = w, fw, u, fu
            elif fu <= fv or v == x or v == w:
                v, fv = u, fu
    return x, fx, trace


def distance_matrix(X) -> np.ndarray:
    """as.matrix(dist(X)): the full n x n matrix of Euclidean distances, differences squared and summed coordinate
    by coordinate (n^2 doubles; 800 MB at 10 000 points)."""
    X = _matrix(X, "X")
    sq = np.zeros((X.shape[0], X.shape[0]))
    for d in range(X.shape[1]):
        diff = X[:, d, None] - X[None, :, d]
        diff *= diff
        sq += diff
    return np.sqrt(sq, out=sq)


def scale_to_original_distances(reduced, positions=None, orig_dist=None, device: Optional[int] = None,
                                interval=(0.01, 40.0), tol: float = _EPS ** 0.25):
    """The reference's scale_to_original_distances: returns (reduced * scale, scale, info) with scale the minimiser of
    F(s) = sum(abs(orig_dist - dist(reduced) * s)) over `interval`, found as R's optimize finds it (its default tol).
    info: objective (F at the scale), evaluations, trace (the evaluated (s, F) pairs, evaluations x 2).

    device=None is the specification: the two n x n matrices are formed as the reference forms them (orig_dist as
    given, or dist(positions)) and brent_fmin minimises.  A device ordinal needs `positions` -- the library
    recomputes every distance from the coordinates and takes no matrix -- and raises where the reference would have
    failed (a coordinate that is not finite)."""
    Y = _matrix(reduced, "reduced")
    lower, upper = (float(v) for v in interval)
    if device is None:
        if orig_dist is None:
            if positions is None:
                raise ValueError("give positions or orig_dist")
            if not np.isfinite(_matrix(positions, "positions")).all():
                raise ValueError("positions must be finite (the reference's optimize fails on a distance that is not)")
            orig_dist = distance_matrix(positions)
        D = _matrix(orig_dist, "orig_dist")
        if D.shape != (Y.shape[0], Y.shape[0]):
            raise ValueError("orig_dist must be n x n for the n rows of reduced")
        R = distance_matrix(Y)
        if not (np.isfinite(D).all() and np.isfinite(R).all()):
            raise ValueError("the distances must be finite (the reference's optimize fails on one that is not)")
        scale, objective, trace = brent_fmin(lambda s: np.abs(D - R * s).sum(), lower, upper, tol)
        trace = np.array(trace, dtype=np.float64).reshape(-1, 2)
    else:
        if positions is None:
            raise ValueError("the device form computes the original distances from positions: give positions")
        if orig_dist is not None:
            raise ValueError("the device form takes no distance matrix: give positions alone")
        X = _matrix(positions, "positions")
        scale, objective, evaluations, trace = _native.scale_to_original_distances(
            X, Y, lower, upper, tol, device=device, trace_len=256)
        if evaluations > trace.shape[0]:
            raise RuntimeError(f"{evaluations} evaluations: Brent's fmin did not settle")
    info = dict(objective=float(objective), evaluations=int(trace.shape[0]), trace=trace)
    return Y * scale, float(scale), info


def reduce_dimensions(positions, config: Optional[DimReductionConfig] = None, device: Optional[int] = None) -> np.ndarray:
    """The reference's reduce_dimensions for the coordinates of a map: an n x n_components array whose columns are
    the reference's dim1, dim2, ...: the PCA scores (pca_scores), multiplied by the distance-matching scale when
    config.scale is set (scale_to_original_distances; on `device` when one is given, else on the host)."""
    config = DimReductionConfig() if config is None else config
    X = _matrix(positions, "positions")
    comps = pca_scores(X, config)
    if not config.scale:
        return comps
    return scale_to_original_distances(comps, positions=X, device=device)[0]


def temporal_map_data(positions, times, names=None, clade_members=None, tree_present_points=None,
                      config: Optional[DimReductionConfig] = None, reverse_x: float = 1, reverse_y: float = 1,
                      sigma_t: Optional[float] = None, sigma_x: Optional[float] = None,
                      sigma_x_nd: Optional[float] = None, arrow_plot_threshold: float = 0.1,
                      device: Optional[int] = None) -> dict:
    """What plot_temporal_mapping computes before it draws (:999-1001, :1157-1218), for the antigens of a map (the
    reference filters on its `antigen` column first; pass those rows).  Returns a dictionary:
      reduced (n x n_components: dim1 ..), plot_x = dim2 * reverse_x, plot_y = dim1 * reverse_y;
      sigma_t = bw.nrd(dist(times)), sigma_x = sqrt((bw.nrd(plot_x)^2 + bw.nrd(plot_y)^2) / 2), sigma_x_nd = the root
      mean square of the per-coordinate bw.nrd -- each only where the caller gives none;
      velocity (n x ndim) and velocity_magnitude: kernel_velocity of the positions with sigma_x_nd;
      v_plot_x, v_plot_y and plot_velocity_magnitude: kernel_velocity of (plot_x, plot_y) with sigma_x;
      arrows: the indices whose plot magnitude is >= arrow_plot_threshold (a NaN magnitude is none).
    Both velocity passes and the scale run on `device` when one is given; the clade rule is kernel_velocity's."""
    config = DimReductionConfig() if config is None else config
    if config.n_components < 2:
        raise ValueError("a map plot needs n_components >= 2 (dim1 and dim2)")
    X = _matrix(positions, "positions")
    t = np.asarray(times, dtype=np.float64)
    if t.shape != (X.shape[0],):
        raise ValueError("times must hold one value per position")
    if not (isinstance(arrow_plot_threshold, (int, float)) and arrow_plot_threshold >= 0):
        raise ValueError("arrow_plot_threshold must be a number >= 0")
    reduced = reduce_dimensions(X, config, device=device)
    plot_x = reduced[:, 1] * reverse_x
    plot_y = reduced[:, 0] * reverse_y
    if sigma_t is None:
        sigma_t = pair_difference_bandwidth(t)
    if sigma_x is None:
        sigma_x = math.sqrt(0.5 * (silverman_bandwidth(plot_x) ** 2 + silverman_bandwidth(plot_y) ** 2))
    if sigma_x_nd is None:
        sigma_x_nd = math.sqrt(float(np.mean([silverman_bandwidth(X[:, d]) ** 2 for d in range(X.shape[1])])))
    clade = dict(names=names, clade_members=clade_members, tree_present_points=tree_present_points)
    V, magnitude, _ = kernel_velocity(X, t, sigma_t, sigma_x_nd, device=device, **clade)
    P, plot_magnitude, _ = kernel_velocity(np.column_stack([plot_x, plot_y]), t, sigma_t, sigma_x, device=device, **clade)
    return dict(reduced=reduced, plot_x=plot_x, plot_y=plot_y, sigma_t=float(sigma_t), sigma_x=float(sigma_x),
                sigma_x_nd=float(sigma_x_nd), velocity=V, velocity_magnitude=magnitude, v_plot_x=P[:, 0],
                v_plot_y=P[:, 1], plot_velocity_magnitude=plot_magnitude,
                arrows=np.flatnonzero(plot_magnitude >= arrow_plot_threshold))
