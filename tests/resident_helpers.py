"""Shared by the resident-embedding tests: seeded problems with thresholds, and the harness that drives
`_topolow_euclidean_embedding_resident` of the R shim on the test double of R's C API
(tests/fake_r/resident_harness.c)."""
import json
import os
import subprocess

import numpy as np

from topolow_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_problems = {}


def problem(n, missing, thresholds, seed=None):
    """(values f64 with NaN = NA, codes int8 or None), C-contiguous, symmetric like a parsed titer table: `missing`
    of the cells NA, `thresholds` of the pairs coded (two thirds ">", one third "<").  Cached: callers do not write."""
    key = (n, missing, thresholds, seed)
    if key not in _problems:
        s = 1000 * n + int(100 * missing) + int(1000 * thresholds) if seed is None else seed
        D = np.ascontiguousarray(synthetic.make_problem(n, latent_dim=5, missing=missing, seed=s).dissimilarity)
        codes = None
        if thresholds > 0:
            rng = np.random.default_rng(s + 1)
            u = np.triu(rng.random((n, n)), 1)
            u = u + u.T
            codes = np.zeros((n, n), dtype=np.int8)
            codes[(u > 0) & (u < thresholds * 2 / 3)] = 1
            codes[(u >= thresholds * 2 / 3) & (u < thresholds)] = -1
        D.setflags(write=False)
        _problems[key] = (D, codes)
    return _problems[key]


def start_positions(n, ndim, seed):
    """A random-walk start like the reference's (R/core.R:407-415), row q for point q of the ordered matrix."""
    rng = np.random.default_rng(seed)
    steps = rng.uniform(0.0, 0.2, size=(ndim, n - 1)).T
    return np.ascontiguousarray(np.vstack([np.zeros((1, ndim)), np.cumsum(steps, axis=0)]))


def same_bits(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and \
        np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()


def build_harness(out_dir):
    out = os.path.join(str(out_dir), "resident_harness")
    csrc = os.path.join(ROOT, "topolow_amd", "csrc")
    cmd = ["gcc", "-O1", "-I", os.path.join(ROOT, "tests", "fake_r"), "-I", os.path.join(ROOT, "include"),
           "-o", out, os.path.join(ROOT, "tests", "fake_r", "resident_harness.c"),
           os.path.join(ROOT, "topolow_amd", "r", "topolow_shim.c"), "-L", csrc, "-ltopolow_relax",
           "-Wl,-rpath," + csrc, "-lm"]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def _fmt(a):
    return " ".join(repr(float(x)) for x in np.asarray(a, dtype=np.float64).ravel(order="F"))


def run_harness(harness, tmp_path, values, codes, order, init, ndim, n_iter=20, k0=5.0, cooling_rate=0.01,
                c_repulsion=0.01, relative_epsilon=1e-4, window=5, check_freq=3, preserve_order=False, verbose=False,
                want_est=True, seed=7, interrupt_after=0, bad=0, n=None):
    """`order`: 1-based or None.  `n`: what the header line claims (default: the values' size)."""
    values = np.asarray(values, dtype=np.float64)
    vn = values.shape[0]
    n = vn if n is None else n
    head = [n, ndim, vn, 0 if codes is None else codes.shape[0], 0 if order is None else len(order), init.shape[0],
            init.shape[1], int(bool(want_est)), int(bool(preserve_order)), int(bool(verbose)), n_iter, window,
            check_freq, seed, interrupt_after, bad]
    lines = [" ".join(str(x) for x in head), f"{k0!r} {cooling_rate!r} {c_repulsion!r} {relative_epsilon!r}",
             _fmt(values)]
    if codes is not None:
        lines.append(_fmt(codes))
    if order is not None:
        lines.append(" ".join(str(int(x)) for x in order))
    lines.append(_fmt(init))
    path = os.path.join(str(tmp_path), "resident.txt")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    res = subprocess.run([harness, path], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-2000:])
    return json.loads(res.stdout)
