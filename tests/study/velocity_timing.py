"""GPU study: the antigenic velocity (topolow_amd.velocity.kernel_velocity), host form against device form.

One process, one GPU.  The points are the generating positions of `synthetic.make_problem(n, 5, 0.7)` (for ndim 2 and
10: normal points of the same spread), the times integer years 2000 to 2015, sigma_x and sigma_t from
`default_bandwidths`, no clades.
  * host form:   kernel_velocity(..., device=None) -- the specification: a row loop of NumPy operations on the box's CPUs;
  * device form: kernel_velocity(..., device=0) -- topolow_kernel_velocity: the host's sort, the uploads, the two
                 kernels and the downloads.
Wall clock (time.perf_counter) around each call; the device form's kernel time from device events through the _ex
entry in a call of its own.  One warm-up of the device form, then the two forms ALTERNATED `repeats` times; median
and spread (max - min) of each, and how far apart the two forms' weight sums and velocities are.

usage: python tests/study/velocity_timing.py [--sizes 10000] [--ndims 5,2,10] [--repeats 3]"""
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
from topolow_amd import _native, synthetic, velocity  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="10000")
ap.add_argument("--ndims", default="5,2,10")
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()

print(f"# kernel_velocity, integer years 2000-2015, default bandwidths, no clades; wall clock, {args.repeats} alternated "
      f"repeats after one device warm-up; median (spread = max - min); CPUs for NumPy: "
      f"{os.environ.get('OMP_NUM_THREADS', '?')}")
for n in [int(s) for s in args.sizes.split(",")]:
    prob = synthetic.make_problem(n, latent_dim=5, missing=0.7, seed=n)
    P5 = np.asarray(prob.true_coordinates, dtype=np.float64)
    rng = np.random.default_rng(n + 2)
    t = rng.integers(2000, 2016, size=n).astype(float)
    for ndim in [int(s) for s in args.ndims.split(",")]:
        P = P5 if ndim == P5.shape[1] else rng.normal(scale=P5.std(), size=(n, ndim))
        t0 = time.perf_counter()
        sx, st = velocity.default_bandwidths(P, t)
        bw_t = time.perf_counter() - t0
        velocity.kernel_velocity(P, t, st, sx, device=0)
        host_t, dev_t, kern_t = [], [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            Vh, mh, Wh = velocity.kernel_velocity(P, t, st, sx)
            t1 = time.perf_counter()
            Vd, md, Wd = velocity.kernel_velocity(P, t, st, sx, device=0)
            t2 = time.perf_counter()
            secs = []
            _native.kernel_velocity(P, t, st, sx, device=0, timing=secs)
            host_t.append(t1 - t0)
            dev_t.append(t2 - t1)
            kern_t.append(secs[0])
        ok = Wh > 0
        relW = float(np.max(np.abs(Wd[ok] - Wh[ok]) / Wh[ok]))
        relV = float(np.max(np.abs(Vd[ok] - Vh[ok]) / np.maximum(np.abs(Vh[ok]).max(axis=0), 1e-300)))
        same_nan = bool(np.array_equal(np.isnan(Vd), np.isnan(Vh)))
        print(f"n = {n:6d}  ndim {ndim:2d}  sigma_x {sx:.4f}  sigma_t {st:.4f}  (default_bandwidths {bw_t:.3f} s)  rows with a "
              f"past {int(ok.sum())}  NaN rows equal {same_nan}  W apart at most {relW:.2e} relative, V {relV:.2e} of the "
              f"column's largest")
        print(f"    host form   {np.median(host_t):9.3f} s ({max(host_t) - min(host_t):7.3f})")
        print(f"    device form {np.median(dev_t) * 1e3:9.2f} ms ({(max(dev_t) - min(dev_t)) * 1e3:7.2f})   the two kernels "
              f"{np.median(kern_t) * 1e3:.3f} ms")
        print(f"    host / device {np.median(host_t) / np.median(dev_t):8.1f}", flush=True)
