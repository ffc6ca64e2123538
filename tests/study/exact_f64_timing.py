"""GPU study: what precision "f64_exact" costs in time at config 3's shape (N = 10 000, 70 % missing, ndim 5).

Two kinds of iteration, HIP-event time each (topolow_session_profile_symmetric / _profile):
  * one-stage iterations as the symmetric sweep + apply (csrc/relax_symm64.h: symm64x_sweep_kernel against
    symm64_sweep_kernel), the iterations that also reduce a check's MAE apart;
  * 16-stage iterations on the row-owner stage kernel (csrc/relax_exact.h: slab_stage_exact_kernel against
    slab_stage_pipe_kernel<.., double, ..>), TOPOLOW_SYMMETRIC=0: the sum of an iteration's 16 launches.
Three forms are alternated on the same problem in one process, `rounds` times each: this build's "f64_exact", this
build's "f64" and -- with --parent-lib -- "f64" on a build of the parent commit.  Per figure: the median of the rounds
and their spread (max - min).  The exact form costs something where its median exceeds f64's by more than that spread.

With --asm PATH (the listing `make -C topolow_amd/csrc asm` writes; needs no GPU) the registers and waves per SIMD of
the 44 instances of the two exact kernels are printed as well.

The parent build is not made here: check the parent commit out beside this tree (git worktree add DIR HEAD~1), run
make -C DIR/topolow_amd/csrc there and pass DIR/topolow_amd/csrc/libtopolow_relax.so.

usage: python tests/study/exact_f64_timing.py [--parent-lib PATH] [--asm PATH] [--n 10000] [--dim 5] [--rounds 5]"""
import argparse
import dataclasses
import importlib.util
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from topolow_amd import _native, core, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--asm", default=None)
ap.add_argument("--n", type=int, default=10000)
ap.add_argument("--dim", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=60, help="one-stage iterations per round")
ap.add_argument("--stage-iters", type=int, default=12, help="16-stage iterations per round")
ap.add_argument("--min-n", default=None, help="TOPOLOW_SYMMETRIC_MIN_N for sizes below the default gate")
ap.add_argument("--no-gpu", action="store_true", help="the register table only")
args = ap.parse_args()
if args.min_n is not None:
    os.environ["TOPOLOW_SYMMETRIC_MIN_N"] = args.min_n


def register_table(path):
    text = open(path).read()
    print("# registers of the exact kernels (from the ISA listing): VGPRs, AGPRs, scratch bytes, waves per SIMD")
    for pat, label in ((r"_ZN7topolow20symm64x_sweep_kernelILi(\d+)ELb([01])ELb([01])E\w+", "symm64x_sweep_kernel<ndim, thresholds, ERR>"),
                       (r"_ZN7topolow23slab_stage_exact_kernelILi(\d+)E\w+?ELb([01])EEEv\w+", "slab_stage_exact_kernel<ndim, cfg, thresholds>")):
        rows = []
        for m in re.finditer(r"^(" + pat + "):", text, re.M):
            end = text.index(".Lfunc_end", m.start())
            tail = text[end:end + 3000]
            g = lambda key: int(re.search(r"; %s: (\d+)" % key, tail).group(1))  # noqa: E731
            rows.append((int(m.group(2)),) + tuple(int(x) for x in m.groups()[2:]) +
                        (g("NumVgprs"), g("NumAgprs"), g("ScratchSize"), g("Occupancy")))
        print(f"# {label}: {len(rows)} instances")
        for r in sorted(rows):
            print("    " + " ".join(f"{x:4d}" for x in r))


if args.asm:
    register_table(args.asm)
if args.no_gpu:
    sys.exit(0)

parent = None
if args.parent_lib:   # a second copy of the binding, bound to the other library
    spec = importlib.util.spec_from_file_location("topolow_amd._native_parent", _native.__file__)
    parent = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = parent
    spec.loader.exec_module(parent)
    parent.LIB_PATH = os.path.abspath(args.parent_lib)
    parent._PRECISIONS.pop("f64_exact", None)


def session(mod, call, n, dim, precision, sym):
    os.environ["TOPOLOW_SYMMETRIC"] = sym
    s = mod.Session(n, dim, precision=precision)
    s.set_relabel(3)
    s.load_coo(call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh, call.degrees)
    s.set_edges(call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh)
    return s


def measure_sweep(s, call, iters):
    """(us per plain sweep + apply, us per one that also reduces a check) of `iters` one-stage iterations at k = 2."""
    s.set_positions(call.initial_positions)
    s.set_profiling(True)
    s.begin(iters, 2.0, 0.01, 0.01, 1e-12, 10 ** 9, 3, 5, 1)
    s.run()
    s.sync()
    sym_ms, sym_it, symf_ms, symf_it = s.profile_symmetric()
    s.set_profiling(False)
    assert sym_it + symf_it == iters, (sym_it, symf_it)
    return 1e3 * sym_ms / max(sym_it, 1), 1e3 * symf_ms / max(symf_it, 1)


def measure_stages(s, call, iters):
    """(us per 16-stage row-owner iteration, us per stage launch) of `iters` iterations at k = 20."""
    s.set_positions(call.initial_positions)
    s.set_profiling(True)
    s.begin(iters, 20.0, 0.01, 0.01, 1e-12, 10 ** 9, 3, 5, 16)
    s.run()
    s.sync()
    st_ms, st_n, _ck_ms, _ck_n = s.profile()
    s.set_profiling(False)
    assert st_n == 16 * iters, st_n
    return 1e3 * st_ms / iters, 1e3 * st_ms / st_n


def stat(v):
    return f"{np.median(v):8.1f} +- {max(v) - min(v):5.1f}"


n, dim = args.n, args.dim
prob = synthetic.make_problem(n, latent_dim=dim, missing=0.7, seed=12345)
init = synthetic.initial_positions(prob.dissimilarity, dim, 12345)
base = core.prepare_layout_call(prob.dissimilarity, dim, 1, 2.0, 0.01, 0.01, 1e-4, 5, init, False, 3, True)
del prob
print(f"# N = {n}, 70 % missing, ndim {dim}; {args.rounds} rounds alternated; us (HIP events): median +- spread (max - min) of the rounds")
forms = [("f64_exact (this build)", _native, "f64_exact"), ("f64 (this build)", _native, "f64")]
if parent is not None:
    forms.append(("f64 (parent build)", parent, "f64"))
for thr in (0.0, 0.15):
    call = base
    if thr > 0:   # a share of the measured pairs become ">" / "<" targets (the threshold instances)
        rng = np.random.default_rng(3)
        code = rng.choice([0, 1, -1], size=base.edge_thresh.shape[0], p=[1 - thr, thr / 2, thr / 2])
        call = dataclasses.replace(base, edge_thresh=code.astype(base.edge_thresh.dtype))
    for kind, sym, measure, count in (("one-stage iteration: sweep + apply", "1", measure_sweep, args.iters),
                                      ("16-stage iteration: row-owner stage kernel", "0", measure_stages, args.stage_iters)):
        ss = [session(mod, call, n, dim, precision, sym) for _, mod, precision in forms]
        got = [[] for _ in forms]
        for s in ss:                                   # warm-up: builds the sweep's buffers, loads the kernels
            measure(s, call, 3)
        for _ in range(args.rounds):
            for q, s in enumerate(ss):
                got[q].append(measure(s, call, count))
        for s in ss:
            s.close()
        print(f"thresholds {thr:4.2f}: {kind}")
        second = "with a fused check" if sym == "1" else "per stage launch"
        for (name, _, _), g in zip(forms, got):
            print(f"    {name:24s} {stat([x[0] for x in g])}   {second} {stat([x[1] for x in g])}")
        exact = [x[0] for x in got[0]]
        for (name, _, _), g in zip(forms[1:], got[1:]):
            ref = [x[0] for x in g]
            spread = max(max(ref) - min(ref), max(exact) - min(exact))
            print(f"    ratio f64_exact / {name:20s}: x{np.median(exact) / np.median(ref):.3f}   "
                  f"(difference {np.median(exact) - np.median(ref):6.1f} us, spread {spread:.1f} us)", flush=True)
