"""GPU study: the plot coordinates of a map (topolow_amd.reduce.reduce_dimensions), host form against device form.

One process, one GPU.  The points are the generating positions of `synthetic.make_problem(n, 5, 0.7)`; the default
configuration: PCA to two components (host code in both forms, timed on its own), then the distance-matching scale.
  * host form:   scale_to_original_distances(..., device=None) -- the specification: the two n x n distance matrices
                 in NumPy on the box's CPUs (800 MB each at n = 10 000, and two or three more temporaries of that size
                 per evaluation) and Brent's fmin in Python;
  * device form: scale_to_original_distances(..., device=0) -- topolow_scale_to_original_distances: the two uploads and
                 one launch pair and one 24-byte download per evaluation of Brent's fmin inside the library.
Wall clock (time.perf_counter) around each call; the kernel time of ONE evaluation from device events through the _ex
entry (m = 1 and m = 8) in calls of their own.  One warm-up of the device form, then the two forms ALTERNATED `repeats`
times; median and spread (max - min) of each; both scales, their evaluation counts and their distance to the exact
minimiser (the weighted median of d / r with weights r) in units of Brent's tol1.  A size whose host form does not fit
in memory is reported as such and the device form is timed alone.

usage: python tests/study/reduce_timing.py [--sizes 10000,3000] [--repeats 3]"""
import argparse
import math
import os
import sys
import time

import numpy as np

try:   # torch's HIP runtime has to be the first one a process loads (tests/conftest.py)
    import torch  # noqa: F401
except Exception:  # pragma: no cover
    torch = None

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from topolow_amd import _native, reduce as rd, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="10000,3000")
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()

EPS = float(np.finfo(np.float64).eps)


def tol1_of(s):
    return math.sqrt(EPS) * abs(s) + EPS ** 0.25 / 3


def weighted_median(X, Y):
    """The exact minimiser, from the upper triangles of the two distance matrices."""
    D, R = rd.distance_matrix(X), rd.distance_matrix(Y)
    upper = np.triu(np.ones(D.shape, dtype=bool), 1)
    d, r = D[upper], R[upper]
    del D, R, upper
    keep = r > 0
    q, w = d[keep] / r[keep], r[keep]
    order = np.argsort(q, kind="stable")
    cum = np.cumsum(w[order])
    return float(q[order][np.searchsorted(cum, 0.5 * cum[-1])])


print(f"# reduce_dimensions, default configuration (PCA to 2 components, scale = TRUE, interval [0.01, 40], tol eps^0.25); "
      f"wall clock, {args.repeats} alternated repeats after one device warm-up; median (spread = max - min); CPUs for "
      f"NumPy: {os.environ.get('OMP_NUM_THREADS', '?')}")
for n in [int(s) for s in args.sizes.split(",")]:
    prob = synthetic.make_problem(n, latent_dim=5, missing=0.7, seed=n)
    X = np.asarray(prob.true_coordinates, dtype=np.float64)
    t0 = time.perf_counter()
    Y = rd.pca_scores(X)
    pca_t = time.perf_counter() - t0
    rd.scale_to_original_distances(Y, positions=X, device=0)
    host_t, dev_t, k1_t, k8_t = [], [], [], []
    host, dev, host_fits = None, None, True
    for _ in range(args.repeats):
        if host_fits:
            try:
                t0 = time.perf_counter()
                host = rd.scale_to_original_distances(Y, positions=X)
                host_t.append(time.perf_counter() - t0)
            except MemoryError:
                host_fits = False
        t1 = time.perf_counter()
        dev = rd.scale_to_original_distances(Y, positions=X, device=0)
        dev_t.append(time.perf_counter() - t1)
        secs = []
        _native.scale_objective(X, Y, [dev[1]], device=0, timing=secs)
        k1_t.append(secs[0])
        _native.scale_objective(X, Y, np.geomspace(0.01, 40.0, 8), device=0, timing=secs)
        k8_t.append(secs[0])
    try:
        exact = weighted_median(X, Y)
    except MemoryError:
        exact = None
    print(f"n = {n:6d}  ndim {X.shape[1]}  pca_scores {pca_t * 1e3:.2f} ms")
    if host_fits:
        print(f"    host form   {np.median(host_t):9.3f} s ({max(host_t) - min(host_t):7.3f})   scale {host[1]:.10f}  "
              f"{host[2]['evaluations']} evaluations")
    else:
        print("    host form   did not fit in memory (MemoryError)")
    print(f"    device form {np.median(dev_t) * 1e3:9.2f} ms ({(max(dev_t) - min(dev_t)) * 1e3:7.2f})   scale {dev[1]:.10f}  "
          f"{dev[2]['evaluations']} evaluations;  the two kernels of one evaluation {np.median(k1_t) * 1e3:.3f} ms, of one "
          f"with 8 scales {np.median(k8_t) * 1e3:.3f} ms")
    if exact is not None:
        line = f"    weighted median {exact:.10f}:  device {abs(dev[1] - exact) / tol1_of(dev[1]):.3f} tol1 away"
        if host_fits:
            line += (f", host {abs(host[1] - exact) / tol1_of(host[1]):.3f} tol1 away, the two forms "
                     f"{abs(dev[1] - host[1]) / tol1_of(dev[1]):.3f} tol1 apart")
        print(line)
    if host_fits:
        print(f"    host / device {np.median(host_t) / np.median(dev_t):8.1f}", flush=True)
