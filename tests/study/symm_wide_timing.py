"""GPU study: one-stage iterations of an fp32 session at ndim 7..10 on a config-3-shaped problem (N = 10 000, 70 %
missing) -- the symmetric sweep for these dims (csrc/relax_symm_wide.h: sweep + apply) against the row-owner stage
kernel, with and without thresholds.  HIP-event time per iteration (topolow_session_profile_symmetric / _profile), the
iterations that also reduce a check's MAE apart.

Three forms are alternated on the same problem in one process, `rounds` times each: this build's sweep
(TOPOLOW_SYMMETRIC=1), this build's row-owner kernel (TOPOLOW_SYMMETRIC=0), and -- with --parent-lib -- a build of
the parent commit, which runs these dims on the row-owner kernel whatever the variable says.  Per figure: the median
of the rounds and their spread (max - min).  A dimension is worth enabling by default where the sweep is faster than
the parent by more than that spread.

The parent build is not made here: check the parent commit out beside this tree (git worktree add DIR HEAD~1), run
make -C DIR/topolow_amd/csrc there and pass DIR/topolow_amd/csrc/libtopolow_relax.so.  Both libraries then live in one
process, each behind its own copy of the ctypes binding.

usage: python tests/study/symm_wide_timing.py [--parent-lib PATH] [--lib PATH] [--n 10000] [--rounds 5] [--dims 7,8,9,10]"""
import argparse
import dataclasses
import importlib.util
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from topolow_amd import _native, core, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--lib", default=None, help="this build's library, if not the one in the tree")
ap.add_argument("--n", type=int, default=10000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=60)
ap.add_argument("--dims", default="7,8,9,10")
ap.add_argument("--min-n", default=None, help="TOPOLOW_SYMMETRIC_MIN_N for sizes below the default gate")
args = ap.parse_args()
if args.min_n is not None:
    os.environ["TOPOLOW_SYMMETRIC_MIN_N"] = args.min_n

if args.lib:
    _native.LIB_PATH = os.path.abspath(args.lib)
parent = None
if args.parent_lib:   # a second copy of the binding, bound to the other library
    spec = importlib.util.spec_from_file_location("topolow_amd._native_parent", _native.__file__)
    parent = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = parent
    spec.loader.exec_module(parent)
    parent.LIB_PATH = os.path.abspath(args.parent_lib)


def session(mod, call, n, dim, sym):
    if sym is None:
        os.environ.pop("TOPOLOW_SYMMETRIC", None)
    else:
        os.environ["TOPOLOW_SYMMETRIC"] = sym
    s = mod.Session(n, dim, precision="f32")
    s.set_relabel(3)
    s.load_coo(call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh, call.degrees)
    s.set_edges(call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
    return s


def measure(s, call, iters):
    """(us per plain iteration, us per iteration that also reduces a check, form) of `iters` one-stage iterations from
    the reference's start at k = 2, a check every 3."""
    s.set_positions(call.initial_positions)
    s.set_profiling(True)
    s.begin(iters, 2.0, 0.01, 0.01, 1e-12, 10 ** 9, 3, 5, 1)
    s.run()
    s.sync()
    sym_ms, sym_it, symf_ms, symf_it = s.profile_symmetric()
    fused_ms, fused_n = s.profile_fused()
    st_ms, st_n, _ck_ms, _ck_n = s.profile()
    s.set_profiling(False)
    if sym_it + symf_it > 0:
        assert st_n == 0 and sym_it + symf_it == iters
        return 1e3 * sym_ms / max(sym_it, 1), 1e3 * symf_ms / max(symf_it, 1), "sweep"
    assert st_n == iters
    return 1e3 * (st_ms - fused_ms) / max(st_n - fused_n, 1), 1e3 * fused_ms / max(fused_n, 1), "row-owner"


def stat(v):
    return f"{np.median(v):7.1f} +- {max(v) - min(v):4.1f}"


n = args.n
print(f"# N = {n}, 70 % missing, fp32, {args.iters} one-stage iterations at k = 2 (check every 3), {args.rounds} rounds alternated;")
print("# us per iteration (HIP events): median +- spread (max - min) of the rounds; 'check': the iterations that also reduce a check's MAE")
for dim in [int(d) for d in args.dims.split(",")]:
    prob = synthetic.make_problem(n, latent_dim=dim, missing=0.7, seed=12345)
    init = synthetic.initial_positions(prob.dissimilarity, dim, 12345)
    base = core.prepare_layout_call(prob.dissimilarity, dim, 1, 2.0, 0.01, 0.01, 1e-4, 5, init, False, 3, True)
    del prob
    for thr in (0.0, 0.15):
        call = base
        if thr > 0:   # a share of the measured pairs become ">" / "<" targets (the threshold instances)
            rng = np.random.default_rng(3)
            code = rng.choice([0, 1, -1], size=base.edge_thresh.shape[0], p=[1 - thr, thr / 2, thr / 2])
            call = dataclasses.replace(base, edge_thresh=code.astype(base.edge_thresh.dtype))
        forms = [("sweep + apply (this build)", _native, "1"), ("row-owner (this build, TOPOLOW_SYMMETRIC=0)", _native, "0")]
        if parent is not None:
            forms.append(("row-owner (parent build)", parent, None))
        ss = [session(mod, call, n, dim, sym) for _, mod, sym in forms]
        got = [[] for _ in forms]
        for s in ss:                                   # warm-up: builds the sweep's buffers, loads the kernels
            measure(s, call, 6)
        for _ in range(args.rounds):
            for q, s in enumerate(ss):
                got[q].append(measure(s, call, args.iters))
        for s in ss:
            s.close()
        print(f"ndim {dim:2d} thresholds {thr:4.2f}")
        for (name, _, _), g in zip(forms, got):
            assert len({x[2] for x in g}) == 1
            print(f"    {name:46s} [{g[0][2]:9s}] plain {stat([x[0] for x in g])}   check {stat([x[1] for x in g])}")
        sweep = np.median([x[0] for x in got[0]])
        for (name, _, _), g in zip(forms[1:], got[1:]):
            ro = [x[0] for x in g]
            spread = max(max(ro) - min(ro), max(x[0] for x in got[0]) - min(x[0] for x in got[0]))
            print(f"    ratio {name:40s} / sweep: x{np.median(ro) / sweep:.3f}   (difference {np.median(ro) - sweep:6.1f} us, spread {spread:.1f} us)",
                  flush=True)
