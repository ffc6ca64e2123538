"""Shared by the post-metrics tests: the counting rule in NumPy, seeded inputs, and the harness that drives
`_topolow_post_metrics` of the R shim on the test double of R's C API (tests/fake_r/post_harness.c)."""
import json
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def counting_cells(values, codes=None):
    """The rule of topolow_post_metrics: the value is finite and the code, if there are codes, is 0."""
    ok = np.isfinite(values)
    return ok if codes is None else ok & (np.asarray(codes) == 0)


def reference_sum(values, est, mask):
    """sum |values - est| over the counting cells, exactly rounded."""
    return math.fsum(np.abs(values[mask] - est[mask]).tolist())


def make_inputs(n, ndim, seed):
    """positions, values (about 60 % NaN, a cell and its mirror drawn independently, a few +-Inf, a diagonal that
    mixes 0, non-zero values and NaN) and codes in {0, 1, -1}."""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, ndim)) * 3.0
    values = rng.uniform(0.0, 12.0, size=(n, n))
    values[rng.random((n, n)) < 0.6] = np.nan
    flat = values.reshape(-1)
    k = max(1, n * n // 50)
    flat[rng.integers(0, n * n, size=k)] = np.inf
    flat[rng.integers(0, n * n, size=k)] = -np.inf
    diag = rng.choice(3, size=n) if n > 2 else np.arange(n)     # the smallest sizes still see two kinds
    values[np.arange(n), np.arange(n)] = np.where(diag == 0, 0.0, np.where(diag == 1, rng.uniform(0.5, 2.0, n), np.nan))
    codes = rng.choice(np.array([0, 0, 0, 1, -1], dtype=np.int32), size=(n, n))
    return p, values, codes


def build_harness(out_dir):
    out = os.path.join(str(out_dir), "post_harness")
    csrc = os.path.join(ROOT, "topolow_amd", "csrc")
    cmd = ["gcc", "-O1", "-I", os.path.join(ROOT, "tests", "fake_r"), "-I", os.path.join(ROOT, "include"),
           "-o", out, os.path.join(ROOT, "tests", "fake_r", "post_harness.c"),
           os.path.join(ROOT, "topolow_amd", "r", "topolow_shim.c"), "-L", csrc, "-ltopolow_relax",
           "-Wl,-rpath," + csrc, "-lm"]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def _fmt(a):
    return " ".join(repr(float(x)) for x in np.asarray(a, dtype=np.float64).ravel(order="F"))


def run_harness(harness, tmp_path, positions, values, codes, want_est):
    n, ndim = positions.shape
    lines = [f"{n} {ndim} {values.shape[0]} {0 if codes is None else codes.shape[0]} {int(bool(want_est))}", _fmt(positions), _fmt(values)]
    if codes is not None:
        lines.append(_fmt(codes))
    path = os.path.join(str(tmp_path), "post.txt")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    res = subprocess.run([harness, path], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.stdout, res.stderr)
    return json.loads(res.stdout)
