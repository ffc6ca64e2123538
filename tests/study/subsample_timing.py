"""GPU study: a connected subsample of a resident matrix, through the host and through the parent handle.

One process, one GPU.  The parent is `synthetic.make_problem(n, 5, 0.7)` with threshold codes on 15 % of the pairs,
open as a PreparedHandle (its upload is NOT part of either route: it has happened before a parameter search begins).
Per subsample size m, for one random draw of m points, the two routes a caller has to a handle of the submatrix:
  * host route: NumPy gather of the values and the codes (np.ix_), subsample.component_labels on the gathered values,
    then _native.PreparedHandle(sub, sub_codes) -- a fresh upload;
  * device route: parent.connectivity(indices), then parent.subsample(indices) -- nothing of size m x m crosses the
    host link.
Wall clock (time.perf_counter) around each step; every step ends with its result on the host or with a device
synchronise inside the library.  One warm-up of each route at the size, then the two routes ALTERNATED `repeats` times;
median and spread (max - min) of the totals, the median of each step.  The two handles are compared (info and the
fetched edge list), the two component counts too.
Then parent.connectivity() of the whole matrix, `repeats` times: wall clock, the library's own split into the bit pass
and the rounds, and the number of rounds.

usage: python tests/study/subsample_timing.py [--n 10000] [--sizes 2000,5000] [--repeats 3]"""
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
from topolow_amd import _native, subsample, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10000)
ap.add_argument("--sizes", default="2000,5000")
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()
n = args.n

D = np.ascontiguousarray(synthetic.make_problem(n, latent_dim=5, missing=0.7, seed=n).dissimilarity)
rng = np.random.default_rng(n + 1)
u = np.triu(rng.random((n, n)), 1)
u = u + u.T
codes = np.zeros((n, n), dtype=np.int8)
codes[(u > 0) & (u < 0.10)] = 1
codes[(u >= 0.10) & (u < 0.15)] = -1
del u


def host_route(idx):
    t0 = time.perf_counter()
    ix = np.ix_(idx, idx)
    sub, subc = D[ix], codes[ix]
    t1 = time.perf_counter()
    labels, _ = subsample.component_labels(sub)
    nc = int(np.sum(labels == np.arange(idx.shape[0])))
    t2 = time.perf_counter()
    h = _native.PreparedHandle(sub, subc)
    t3 = time.perf_counter()
    return h, nc, (t1 - t0, t2 - t1, t3 - t2)


def device_route(parent, idx):
    t0 = time.perf_counter()
    nc = parent.connectivity(idx)[0]
    t1 = time.perf_counter()
    h = parent.subsample(idx)
    t2 = time.perf_counter()
    return h, nc, (t1 - t0, t2 - t1)


def med(rows):
    return [float(np.median(c)) for c in zip(*rows)]


print(f"# connected subsample of make_problem({n}, 5, 0.7) + codes; parent handle open; wall clock, {args.repeats} "
      f"alternated repeats after one warm-up of each route; median (spread = max - min)")
with _native.PreparedHandle(D, codes, preserve_order=True) as parent:
    for m in [int(s) for s in args.sizes.split(",")]:
        idx = np.random.default_rng(m).permutation(n)[:m].astype(np.int32)
        for route in (lambda: host_route(idx), lambda: device_route(parent, idx)):
            route()[0].close()
        host_rows, dev_rows, same = [], [], True
        for _ in range(args.repeats):
            hh, hnc, hs = host_route(idx)
            dh, dnc, ds = device_route(parent, idx)
            host_rows.append(hs)
            dev_rows.append(ds)
            a, b = hh.fetch(want_dense=False, want_reordered=False), dh.fetch(want_dense=False, want_reordered=False)
            same = same and hnc == dnc and hh.info == dh.info and np.array_equal(a.edge_dist, b.edge_dist) and \
                np.array_equal(a.edge_i, b.edge_i) and np.array_equal(a.order, b.order)
            hh.close()
            dh.close()
        ht, dt = [sum(r) for r in host_rows], [sum(r) for r in dev_rows]
        hm, dm = med(host_rows), med(dev_rows)
        print(f"m = {m:6d}  components {dnc}  equal: {same}")
        print(f"    host route   {np.median(ht) * 1e3:9.1f} ms ({(max(ht) - min(ht)) * 1e3:7.1f})   gather {hm[0] * 1e3:.1f} ms, "
              f"components (NumPy) {hm[1] * 1e3:.1f} ms, PreparedHandle(sub) {hm[2] * 1e3:.1f} ms")
        print(f"    device route {np.median(dt) * 1e3:9.1f} ms ({(max(dt) - min(dt)) * 1e3:7.1f})   connectivity(indices) "
              f"{dm[0] * 1e3:.1f} ms, subsample(indices) {dm[1] * 1e3:.1f} ms")
        print(f"    host / device {np.median(ht) / np.median(dt):6.2f}", flush=True)
    parent.connectivity()
    rows = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        nc, cells, _ = parent.connectivity()
        dt = time.perf_counter() - t0
        rounds, (bits_s, rounds_s) = parent.graph_stats()
        rows.append((dt, bits_s, rounds_s))
    w = [r[0] for r in rows]
    mm = med(rows)
    print(f"whole matrix, n = {n}: components {nc}, cells {cells} (completeness {cells / (n * (n - 1)):.3f}), "
          f"rounds {rounds} (the last one changed nothing)")
    print(f"    connectivity() {mm[0] * 1e3:9.1f} ms ({(max(w) - min(w)) * 1e3:7.1f})   bit pass over {8 * n * n / 1e6:.0f} MB "
          f"{mm[1] * 1e3:.1f} ms, rounds on {n * ((n + 63) // 64) * 8 / 1e6:.1f} MB of bits {mm[2] * 1e3:.1f} ms", flush=True)
