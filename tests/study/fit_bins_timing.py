"""GPU study: the data behind the fit's diagnostic plots (topolow_amd.error_metrics.embedding_quality_data), host form
against device form, and each device pass on its own.

One process, one GPU.  The problem is fit_report_timing.py's: `synthetic.make_problem(n, 5, 0.7)` with threshold codes
on 15 % of the pairs and a 5 % hold-out of its measured cells, open as a PreparedHandle (its upload is NOT part of either
form); the positions are the generating points, disturbed.
  * host form:   distances by _native.est_distances on the device (timed apart, not counted), then
                 embedding_quality_data(D, est, holdout=picks) -- NumPy on the box's CPUs over n x n temporaries;
  * device form: embedding_quality_data(handle=h, positions=P, holdout=picks) -- fit_statistics as it is, one fit_extent,
                 one fit_order_stats, three fit_hist2d (64 x 64) and one fit_linear_bins (512) on the resident matrix.
Wall clock (time.perf_counter) around each call; every device call ends with its numbers on the host.  One warm-up of
the device form, then the two forms ALTERNATED `repeats` times; median and spread (max - min) of each, then the median
of every single pass, and whether the two forms' counts and densities are equal.

The second problem is the worst case of the LDS counters: a constant matrix with all points at one position, so every
lane of every wave adds to the same counter (the passes only; there is nothing to compare them with).

usage: python tests/study/fit_bins_timing.py [--sizes 10000] [--repeats 3]"""
import argparse
import os
import sys
import time

import numpy as np

try:   # torch's HIP runtime has to be the first one a process loads (tests/conftest.py)
    import torch  # noqa: F401
except Exception:  # pragma: no cover
    torch = None

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from topolow_amd import _native, core, error_metrics, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="10000")
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def passes(h, P, picks, series, extent, repeats):
    """Median milliseconds of every single pass, at the edges and the grid embedding_quality_data uses."""
    tx = np.linspace(0.0, max(extent["true"][1], 1.0), 65)
    px = np.linspace(0.0, max(extent["predicted"][1], 1.0), 65)
    ry = error_metrics._plot_edges(*extent["residual"], 64)
    ey = error_metrics._plot_edges(*extent["error"], 64)
    lo, up = extent["residual"][0] - 1.0, extent["residual"][1] + 1.0
    calls = (("fit_extent", lambda: h.fit_extent(P, series, picks)),
             ("fit_hist2d true x predicted 64 x 64", lambda: h.fit_hist2d(P, series, "true", tx, "predicted", px, picks)),
             ("fit_hist2d true x residual 64 x 64", lambda: h.fit_hist2d(P, series, "true", tx, "residual", ry, picks)),
             ("fit_hist2d predicted x error 64 x 64", lambda: h.fit_hist2d(P, series, "predicted", px, "error", ey, picks)),
             ("fit_hist2d error x true 8192 x 1", lambda: h.fit_hist2d(P, series, "error", error_metrics._plot_edges(*extent["error"], 8192), "true", tx[[0, -1]], picks)),
             ("fit_linear_bins residual 512", lambda: h.fit_linear_bins(P, series, "residual", lo, up, 512, picks)),
             ("fit_linear_bins residual 4096", lambda: h.fit_linear_bins(P, series, "residual", lo, up, 4096, picks)))
    for name, call in calls:
        call()
        ts = [timed(call)[1] for _ in range(repeats)]
        print(f"    {name:40s} {np.median(ts) * 1e3:8.2f} ms ({(max(ts) - min(ts)) * 1e3:6.2f})")


def same(a, b):
    clouds = all(np.array_equal(getattr(a, k).counts, getattr(b, k).counts) and getattr(a, k).outside == getattr(b, k).outside
                 for k in ("scatter", "residual_vs_true", "residual_vs_fitted"))
    return clouds, bool(np.array_equal(a.residual_density.y, b.residual_density.y))


print(f"# embedding_quality_data of make_problem(n, 5, 0.7), 15 % threshold codes, 5 % hold-out, series \"all\", bins "
      f"64 x 64; handle open; wall clock, {args.repeats} alternated repeats after one device warm-up; median (spread = "
      f"max - min); CPUs for NumPy: {os.environ.get('OMP_NUM_THREADS', '?')}")
for n in [int(s) for s in args.sizes.split(",")]:
    prob = synthetic.make_problem(n, latent_dim=5, missing=0.7, seed=n)
    D = np.ascontiguousarray(prob.dissimilarity)
    rng = np.random.default_rng(n + 1)
    u = np.triu(rng.random((n, n), dtype=np.float32), 1)
    u = u + u.T
    codes = np.zeros((n, n), dtype=np.int8)
    codes[(u > 0) & (u < 0.10)] = 1
    codes[(u >= 0.10) & (u < 0.15)] = -1
    del u
    avail = np.flatnonzero(~np.isnan(D).ravel(order="F"))
    picks = np.ascontiguousarray(rng.choice(avail, size=avail.size // 40, replace=False), dtype=np.int64)
    del avail
    P = np.asarray(prob.true_coordinates, dtype=np.float64)
    P = P + 0.05 * rng.normal(size=P.shape)
    truth = core.CodedMatrix(D, codes)
    with _native.PreparedHandle(D, codes, preserve_order=True) as h:
        error_metrics.embedding_quality_data(handle=h, positions=P, holdout=picks)
        host_t, dev_t, est_t, stats_t = [], [], [], []
        for _ in range(args.repeats):
            est, t_est = timed(lambda: _native.est_distances(P))
            host, t_host = timed(lambda: error_metrics.embedding_quality_data(truth, est, holdout=picks))
            del est
            dev, t_dev = timed(lambda: error_metrics.embedding_quality_data(handle=h, positions=P, holdout=picks))
            _, t_stats = timed(lambda: error_metrics.fit_statistics(None, handle=h, positions=P, holdout=picks))
            est_t.append(t_est), host_t.append(t_host), dev_t.append(t_dev), stats_t.append(t_stats)
        clouds, density = same(dev, host)
        print(f"n = {n:6d}  picks {picks.size}  series all: {dev.n} cells; counts equal: {clouds}; density equal: {density}; "
              f"bw {dev.residual_density.bw:.6g}")
        print(f"    host form   {np.median(host_t):9.3f} s ({max(host_t) - min(host_t):7.3f})   "
              f"[est_distances before it, not counted: {np.median(est_t):.3f} s]")
        print(f"    device form {np.median(dev_t):9.3f} s ({max(dev_t) - min(dev_t):7.3f})   of which fit_statistics "
              f"{np.median(stats_t) * 1e3:.1f} ms")
        print(f"    host / device {np.median(host_t) / np.median(dev_t):6.2f}")
        for series in ("all", "out"):
            extent, m = h.fit_extent(P, series, picks)
            print(f"  single passes, series {series} ({m} cells):")
            passes(h, P, picks, series, extent, args.repeats)
    del D, codes, truth, host, dev
    with _native.PreparedHandle(np.full((n, n), 2.5), None, preserve_order=True) as h:
        Z = np.zeros((n, 5))
        extent, m = h.fit_extent(Z, "all")
        print(f"  single passes, all ties (constant matrix, one position; {m} cells, every lane on one counter):")
        passes(h, Z, None, "all", extent, args.repeats)
    sys.stdout.flush()
