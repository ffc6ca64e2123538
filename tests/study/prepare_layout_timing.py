"""GPU study: the pre-processing step (R/core.R:269-436) on the host and on the device.

Wall clock around each call (every call ends with its results on the host), one process, one GPU.  Per size
`synthetic.make_problem(n, 5, 0.7)` with preserve_order=False:
  * core.prepare_layout_call (the host form, NumPy) and core.prepare_layout_call_device, `repeats` timed calls each
    after one warm-up of the device form: median and spread (max - min); the two LayoutCalls are compared field by field
  * the phases of one device call: upload overlapped with the first pass, the ordering rule on the host, the second
    pass, fetch()'s compaction and reorder gather, and fetch()'s downloads -- wall clock inside the library (the pinned
    staging buffers and streams that create() and fetch() set up per call are inside the first and the fourth figure)
  * at the largest size, topolow_amd.euclidean_embedding end to end with TOPOLOW_DEVICE_PREP=0 and =1 (same seed)

usage: python tests/study/prepare_layout_timing.py [--sizes 100,300,1000,3000,10000] [--repeats 3] [--iters 20]"""
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
import topolow_amd  # noqa: E402
from topolow_amd import _native, core, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="100,300,1000,3000,10000")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--iters", type=int, default=20, help="mapping_max_iter of the end-to-end run")
ap.add_argument("--no-end-to-end", action="store_true")
args = ap.parse_args()
sizes = [int(s) for s in args.sizes.split(",")]

ARGS = (5, 20, 5.0, 0.01, 0.01, 1e-4, 5, None, False, 3, False)
FIELDS = ("initial_positions", "dissimilarity_matrix", "threshold_matrix", "degrees", "edge_i", "edge_j", "edge_dist",
          "edge_thresh")


def timed(fn, repeats):
    secs, out = [], None
    for _ in range(repeats):
        out = None
        t0 = time.perf_counter()
        out = fn()
        secs.append(time.perf_counter() - t0)
    return float(np.median(secs)), max(secs) - min(secs), out


print(f"# prepare_layout_call, host against device; make_problem(n, 5, 0.7), preserve_order=False; "
      f"{args.repeats} repeats, median (spread)")
D = None
for n in sizes:
    D = synthetic.make_problem(n, latent_dim=5, missing=0.7, seed=n).dissimilarity
    core.prepare_layout_call_device(D, *ARGS, np.random.default_rng(1))   # warm-up: runtime, first allocations
    h_med, h_sp, host = timed(lambda: core.prepare_layout_call(D, *ARGS, np.random.default_rng(1)), args.repeats)
    route = []
    d_med, d_sp, dev = timed(lambda: core.prepare_layout_call_device(D, *ARGS, np.random.default_rng(1), route=route),
                             args.repeats)
    same = all(np.array_equal(getattr(host, f), getattr(dev, f)) for f in FIELDS) and \
        np.array_equal(host.order, dev.order) and \
        np.array_equal(host.reordered_matrix.values, dev.reordered_matrix.values, equal_nan=True)
    print(f"n = {n:6d}  edges {host.edge_i.shape[0]:9d}  host {h_med * 1e3:9.1f} ms ({h_sp * 1e3:7.1f})   "
          f"device {d_med * 1e3:9.1f} ms ({d_sp * 1e3:7.1f})   host / device {h_med / d_med:6.2f}   route {route[0]}   "
          f"equal: {same}", flush=True)
    del host, dev
    p = _native.prepare_layout(D, None)
    ph = p.phase_seconds
    if p.info["order_route"] == _native.ORDER_DECLINED:
        print(f"            phases: upload + first pass {ph[0] * 1e3:.1f} ms, then declined (the caller orders and "
              f"creates again)", flush=True)
    else:
        print(f"            phases: upload + first pass {ph[0] * 1e3:.1f} ms, order {ph[1] * 1e3:.1f} ms, second pass "
              f"{ph[2] * 1e3:.1f} ms, compaction + reorder gather {ph[3] * 1e3:.1f} ms, download {ph[4] * 1e3:.1f} ms",
              flush=True)
    del p

if not args.no_end_to_end:
    n = sizes[-1]
    print(f"# euclidean_embedding end to end at n = {n}, ndim 5, {args.iters} iterations, set_seed(7)")
    results = {}
    for flag in ("0", "1", "0", "1"):
        os.environ["TOPOLOW_DEVICE_PREP"] = flag
        topolow_amd.set_seed(7)
        t0 = time.perf_counter()
        r = topolow_amd.euclidean_embedding(D, ndim=5, mapping_max_iter=args.iters, k0=5.0, cooling_rate=0.01,
                                            c_repulsion=0.01)
        dt = time.perf_counter() - t0
        print(f"  TOPOLOW_DEVICE_PREP={flag}: {dt:8.2f} s   mae {r.mae!r}", flush=True)
        if flag in results:
            assert np.array_equal(results[flag], r.positions)
        results[flag] = r.positions
        del r
    print(f"  positions equal either way: {np.array_equal(results['0'], results['1'])}")
