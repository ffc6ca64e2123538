"""GPU study: euclidean_embedding() end to end, resident (prepare, relax and score from one upload) against the
present route (the arrays of the 16-argument call fetched and uploaded again).

Wall clock around each call, one process, one GPU.  Per size `synthetic.make_problem(n, 5, 0.7)`, ndim 5,
`--iters` iterations, set_seed(7) before every call:
  * TOPOLOW_RESIDENT=0 and =1 (TOPOLOW_DEVICE_PREP=1 for both), one warm-up each, then `repeats` timed calls each,
    interleaved: median and spread (max - min); positions, est_distances, mae and iter asserted equal
  * with --parent DIR (a built checkout of the parent commit): the same call on that tree, in a child process of its
    own, same warm-up and repeats -- the baseline the gate core._RESIDENT_MIN_N is set against
  * the phases of one resident call, wall clock inside the library: create (upload + first pass, order, second pass),
    the session load from the handle, the whole optimize call, the relaxation loop inside it, post_metrics

usage: python tests/study/resident_embedding_timing.py [--sizes 1000,3000,10000] [--repeats 3] [--iters 20]
                                                        [--parent DIR]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

try:   # torch's HIP runtime has to be the first one a process loads (tests/conftest.py)
    import torch  # noqa: F401
except Exception:  # pragma: no cover
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHILD = r"""
import json, os, sys, time
try:
    import torch  # noqa: F401
except Exception:
    pass
import numpy as np
sys.path.insert(0, sys.argv[1])
import topolow_amd
from topolow_amd import synthetic
assert os.path.dirname(os.path.dirname(os.path.abspath(topolow_amd.__file__))) == os.path.abspath(sys.argv[1])
sizes, repeats, iters = [int(s) for s in sys.argv[2].split(",")], int(sys.argv[3]), int(sys.argv[4])
out = {}
for n in sizes:
    D = synthetic.make_problem(n, latent_dim=5, missing=0.7, seed=n).dissimilarity
    secs = []
    for rep in range(repeats + 1):
        topolow_amd.set_seed(7)
        t0 = time.perf_counter()
        r = topolow_amd.euclidean_embedding(D, ndim=5, mapping_max_iter=iters, k0=5.0, cooling_rate=0.01, c_repulsion=0.01)
        if rep:
            secs.append(time.perf_counter() - t0)
        mae = r.mae
        del r
    out[str(n)] = dict(secs=secs, mae=mae)
print("RESULT " + json.dumps(out))
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,3000,10000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20, help="mapping_max_iter")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: timed in a child process")
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]

    sys.path.insert(0, ROOT)
    import topolow_amd
    from topolow_amd import _native, synthetic

    def embed(D, resident):
        os.environ["TOPOLOW_DEVICE_PREP"] = "1"
        os.environ["TOPOLOW_RESIDENT"] = "1" if resident else "0"
        topolow_amd.set_seed(7)
        t0 = time.perf_counter()
        r = topolow_amd.euclidean_embedding(D, ndim=5, mapping_max_iter=args.iters, k0=5.0, cooling_rate=0.01,
                                            c_repulsion=0.01)
        return time.perf_counter() - t0, r

    parent = {}
    if args.parent:
        env = dict(os.environ, TOPOLOW_DEVICE_PREP="1")
        env.pop("TOPOLOW_RESIDENT", None)
        res = subprocess.run([sys.executable, "-c", CHILD, os.path.abspath(args.parent), args.sizes, str(args.repeats),
                              str(args.iters)], capture_output=True, text=True, env=env)
        if res.returncode != 0:
            raise SystemExit("the parent's run failed:\n" + res.stdout[-2000:] + res.stderr[-2000:])
        parent = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])

    print(f"# euclidean_embedding end to end; make_problem(n, 5, 0.7), ndim 5, {args.iters} iterations, set_seed(7); "
          f"{args.repeats} repeats after one warm-up, median (spread)")
    for n in sizes:
        D = synthetic.make_problem(n, latent_dim=5, missing=0.7, seed=n).dissimilarity
        secs = {False: [], True: []}
        kept = {}
        for rep in range(args.repeats + 1):
            for resident in (False, True):
                dt, r = embed(D, resident)
                if rep:
                    secs[resident].append(dt)
                if resident in kept:
                    assert np.array_equal(kept[resident].positions, r.positions)
                kept[resident] = r
                del r
        a, b = kept[False], kept[True]
        same = (np.array_equal(a.positions, b.positions) and np.array_equal(a.est_distances, b.est_distances) and
                a.iter == b.iter and a.convergence == b.convergence)
        assert same, "the resident route returned other positions"
        assert a.mae == b.mae, (a.mae, b.mae)      # a C-contiguous input: the same bits
        del kept, a, b
        row = f"n = {n:6d}  "
        med = {}
        for resident, label in ((False, "present"), (True, "resident")):
            med[label] = (float(np.median(secs[resident])), max(secs[resident]) - min(secs[resident]))
            row += f"{label} {med[label][0] * 1e3:9.1f} ms ({med[label][1] * 1e3:7.1f})   "
        if str(n) in parent:
            ps = parent[str(n)]["secs"]
            med["parent"] = (float(np.median(ps)), max(ps) - min(ps))
            row += f"parent commit {med['parent'][0] * 1e3:9.1f} ms ({med['parent'][1] * 1e3:7.1f})   "
            gain = med["parent"][0] - med["resident"][0]
            row += (f"resident lower than parent by {gain * 1e3:8.1f} ms, larger spread "
                    f"{max(med['parent'][1], med['resident'][1]) * 1e3:7.1f} ms   ")
        row += f"present / resident {med['present'][0] / med['resident'][0]:5.2f}   equal: {same}"
        print(row, flush=True)

        # the phases of one resident call
        t0 = time.perf_counter()
        with _native.PreparedHandle(D, None) as h:
            t_create = time.perf_counter() - t0
            ph = h.phase_seconds()
            init = np.zeros((n, 5))
            init[:, 0] = np.arange(n) * (h.info["numeric_max"] / n)
            res = h.optimize(init, 5, args.iters, 5.0, 0.01, 0.01, seed=7)
            rs = h.resident_seconds()
            t1 = time.perf_counter()
            h.post_metrics(res.positions)
            t_post = time.perf_counter() - t1
        print(f"            phases: create {t_create * 1e3:.1f} ms (upload + first pass {ph[0] * 1e3:.1f}, order "
              f"{ph[1] * 1e3:.1f}, second pass {ph[2] * 1e3:.1f}); optimize {rs[1] * 1e3:.1f} ms (session load from the "
              f"handle {rs[0] * 1e3:.1f}, setup in all {res.info['setup_seconds'] * 1e3:.1f}, relaxation loop "
              f"{res.info['device_seconds'] * 1e3:.1f}, schedule {res.info['schedule']}); post_metrics "
              f"{t_post * 1e3:.1f} ms", flush=True)


if __name__ == "__main__":
    main()
