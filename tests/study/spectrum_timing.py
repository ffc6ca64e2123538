"""GPU study: the data assessment of Euclidify() (R/core.R:983-1007), host form against device form.

One process, one GPU.  Per size n the problem is `synthetic.make_problem(n, 5, 0.7)`, open as a PreparedHandle (its
upload is NOT part of either form: it has happened before a parameter search begins).
  * host form:   spectrum.data_characteristics(D) -- NumPy on the box's CPUs (median, centring, eigvalsh);
  * device form: spectrum.data_characteristics(None, handle=h) -- topolow_layout_prep_spectrum.
Wall clock (time.perf_counter) around each call; the device call ends with its eigenvalues on the host.  One warm-up of
the device form at the size, then the two forms ALTERNATED `repeats` times; median and spread (max - min) of each, the
median of the device's four phase times, and how far the two spectra are apart in units of n u max|lambda|.

usage: python tests/study/spectrum_timing.py [--sizes 1000,3000,10000] [--repeats 3]"""
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
from topolow_amd import _native, spectrum, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1000,3000,10000")
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()

print(f"# data_characteristics of make_problem(n, 5, 0.7); handle open; wall clock, {args.repeats} alternated repeats "
      f"after one device warm-up; median (spread = max - min); CPUs for NumPy: {os.environ.get('OMP_NUM_THREADS', '?')}")
for n in [int(s) for s in args.sizes.split(",")]:
    D = np.ascontiguousarray(synthetic.make_problem(n, latent_dim=5, missing=0.7, seed=n).dissimilarity)
    with _native.PreparedHandle(D, preserve_order=True) as h:
        h.spectrum()
        host_t, dev_t, phases = [], [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            ref = spectrum.data_characteristics(D)
            t1 = time.perf_counter()
            info, eig, _ = h.spectrum()
            t2 = time.perf_counter()
            host_t.append(t1 - t0)
            dev_t.append(t2 - t1)
            phases.append(info["seconds"])
        apart = float(np.max(np.abs(eig - ref.eigenvalues))) / (n * 2.0 ** -52 * float(np.max(np.abs(ref.eigenvalues))))
        ph = [float(np.median(c)) for c in zip(*phases)]
        print(f"n = {n:6d}  median {info['median']:.6g} (host {ref.median:.6g})  deviation_score "
              f"{info['deviation_score']:.6f} (host {ref.deviation_score:.6f})  dims_90 {info['dims_90']} (host "
              f"{ref.dims_90_percent})  spectra apart {apart:.4f} n u max|lambda|")
        print(f"    host form   {np.median(host_t):9.3f} s ({max(host_t) - min(host_t):7.3f})")
        print(f"    device form {np.median(dev_t):9.3f} s ({max(dev_t) - min(dev_t):7.3f})   median {ph[0] * 1e3:.1f} ms, "
              f"centring {ph[1] * 1e3:.1f} ms, tridiagonalisation {ph[2] * 1e3:.1f} ms "
              f"({16 * n ** 3 / 3 / max(ph[2], 1e-9) / 1e12:.2f} TB/s of 16 n^3 / 3 bytes), bisection {ph[3] * 1e3:.1f} ms")
        print(f"    host / device {np.median(host_t) / np.median(dev_t):6.2f}", flush=True)
