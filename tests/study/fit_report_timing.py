"""GPU study: the evaluation of a fit (topolow_amd.error_metrics.fit_statistics), host form against device form.

One process, one GPU.  The problem is `synthetic.make_problem(n, 5, 0.7)` with threshold codes on 15 % of the pairs
and a 5 % hold-out of its measured cells, open as a PreparedHandle (its upload is NOT part of either form: it happened
before the embedding ran).  The positions are the generating points, disturbed -- a fit, so the errors are spread like
a real one's.
  * host form:   distances by _native.est_distances on the device, then fit_statistics(D, est, holdout=picks) -- NumPy
                 on the box's CPUs over n x n temporaries (the est_distances call is timed apart and not counted);
  * device form: fit_statistics(None, handle=h, positions=P, holdout=picks) -- one topolow_layout_prep_fit_report and
                 two topolow_layout_prep_fit_order_stats calls on the resident matrix.
Wall clock (time.perf_counter) around each call; every device call ends with its numbers on the host.  One warm-up of
the device form, then the two forms ALTERNATED `repeats` times; median and spread (max - min) of each, the medians of
the report's two pass times, of the report call and of one order-statistics call, and the largest relative difference
between the two forms' fields.

usage: python tests/study/fit_report_timing.py [--sizes 10000] [--repeats 3]"""
import argparse
import dataclasses
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


def apart(dev, host):
    worst = 0.0
    for a, b in ((dev.in_sample, host.in_sample), (dev.out_sample, host.out_sample), (dev, host)):
        for f in dataclasses.fields(a):
            x, y = getattr(a, f.name), getattr(b, f.name)
            if isinstance(x, (float, np.ndarray)) and f.name != "seconds":
                x, y = np.atleast_1d(x), np.atleast_1d(y)
                worst = max(worst, float(np.max(np.abs(x - y) / np.maximum(np.abs(y), 1e-300))))
    return worst


print(f"# fit_statistics of make_problem(n, 5, 0.7), 15 % threshold codes, 5 % hold-out; handle open; wall clock, "
      f"{args.repeats} alternated repeats after one device warm-up; median (spread = max - min); CPUs for NumPy: "
      f"{os.environ.get('OMP_NUM_THREADS', '?')}")
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
    # one fold as cv.make_folds draws it: 2.5 % of the measured cells, which with their mirrors are 5 % of them
    avail = np.flatnonzero(~np.isnan(D).ravel(order="F"))
    picks = np.ascontiguousarray(rng.choice(avail, size=avail.size // 40, replace=False), dtype=np.int64)
    del avail
    P = np.asarray(prob.true_coordinates, dtype=np.float64)
    P = P + 0.05 * rng.normal(size=P.shape)
    truth = core.CodedMatrix(D, codes)
    with _native.PreparedHandle(D, codes, preserve_order=True) as h:
        error_metrics.fit_statistics(None, handle=h, positions=P, holdout=picks)
        host_t, dev_t, est_t, passes, stats_t = [], [], [], [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            est = _native.est_distances(P)
            t1 = time.perf_counter()
            host = error_metrics.fit_statistics(truth, est, holdout=picks)
            t2 = time.perf_counter()
            del est                               # 800 MB at n = 10 000: freed outside either form's clock
            t2b = time.perf_counter()
            dev = error_metrics.fit_statistics(None, handle=h, positions=P, holdout=picks)
            t3 = time.perf_counter()
            h.fit_order_stats(P, "in", [0, 1, 2, 3, 4, 5, 6, 7], picks)
            t4 = time.perf_counter()
            est_t.append(t1 - t0)
            host_t.append(t2 - t1)
            dev_t.append(t3 - t2b)
            stats_t.append(t4 - t3)
            passes.append(dev.seconds)
        ps = [float(np.median(c)) for c in zip(*passes)]
        print(f"n = {n:6d}  picks {picks.size}  IN {dev.in_sample.n}  OUT {dev.out_sample.n}  ALL {dev.n}  "
              f"fields apart at most {apart(dev, host):.2e} relative")
        print(f"    host form   {np.median(host_t):9.3f} s ({max(host_t) - min(host_t):7.3f})   "
              f"[est_distances before it, not counted: {np.median(est_t):.3f} s]")
        print(f"    device form {np.median(dev_t):9.3f} s ({max(dev_t) - min(dev_t):7.3f})   report {ps[2] * 1e3:.1f} ms "
              f"(pass 1 with upload and marking {ps[0] * 1e3:.1f} ms, pass 2 {ps[1] * 1e3:.1f} ms), one order-statistics "
              f"call of eight passes {np.median(stats_t) * 1e3:.1f} ms")
        print(f"    host / device {np.median(host_t) / np.median(dev_t):6.2f}", flush=True)
