"""What a convergence check costs a one-stage iteration of the job (not a test): config 3 as bench.py builds it, the
production schedule from the initial positions.  Each run: a fresh session, 60 untimed iterations (k is then below 3 and
every later iteration is one symmetric sweep + apply), then 150 iterations timed between two Session.wait() / device
synchronisations.  Settings, alternated A B C D A B C D ..., five rounds, median and (max - min) per setting:
  A  a check every 3 iterations (the job's own setting)
  B  a check every 10^6 iterations (none inside the timed window)
  C  A with TOPOLOW_SERIAL_CHECKS=1 (every check on the main stream)
  D  A with TOPOLOW_CHECK_IN_APPLY=0 (the separate controller for checks that rode on a sweep; a build without the
     knob runs A again)
A - B is what the checks cost; D - A what running them in the apply's launch recovers.

    python tests/study/check_cost.py [--settings ABCD] [--rounds 5] [--out FILE]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from topolow_amd import _native
from bench import workload_single

SETTINGS = {
    "A": (3, {}),
    "B": (10 ** 6, {}),
    "C": (3, {"TOPOLOW_SERIAL_CHECKS": "1"}),
    "D": (3, {"TOPOLOW_CHECK_IN_APPLY": "0"}),
}
WARM, TIMED = 60, 150


def one_run(call, n, check_freq, env):
    old = {k: os.environ.get(k) for k in ("TOPOLOW_SERIAL_CHECKS", "TOPOLOW_CHECK_IN_APPLY")}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        s = _native.Session(n, 5, precision="f32")
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    s.set_relabel(2024)
    s.load_coo(call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh, call.degrees)
    s.set_edges(call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
    s.set_positions(call.initial_positions)
    s.begin(WARM + TIMED, 5.0, 0.01, 0.01, 1e-4, 10 ** 9, check_freq, 2024, 0)

    def advance(m):
        done = 0
        while done < m:
            got = s.enqueue(m - done)
            assert got > 0
            done += got

    advance(WARM)
    s.wait()
    torch.cuda.synchronize()
    t = time.perf_counter()
    advance(TIMED)
    s.wait()
    torch.cuda.synchronize()
    us = (time.perf_counter() - t) / TIMED * 1e6
    s.sync()
    checks = len(s.check_trace())
    s.close()
    return us, checks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settings", default="ABCD")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    call, _ = workload_single(args.points)
    one_run(call, args.points, 3, {})            # untimed: loads the code objects
    got = {k: [] for k in args.settings}
    checks = {}
    for _ in range(args.rounds):
        for k in args.settings:
            us, checks[k] = one_run(call, args.points, *SETTINGS[k])
            got[k].append(us)
    lines = ["# python " + " ".join([os.path.relpath(__file__)] + sys.argv[1:]),
             "# us per one-stage iteration, %d timed iterations behind %d untimed, N = %d" % (TIMED, WARM, args.points)]
    for k in args.settings:
        v = np.array(got[k])
        lines.append("%s  median %.2f  max-min %.2f  runs %s  checks in the run %d" %
                     (k, np.median(v), v.max() - v.min(), " ".join("%.2f" % x for x in v), checks[k]))
    if "A" in got and "B" in got:
        lines.append("A - B  %.2f us per iteration" % (np.median(got["A"]) - np.median(got["B"])))
    if "A" in got and "D" in got:
        lines.append("D - A  %.2f us per iteration" % (np.median(got["D"]) - np.median(got["A"])))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
