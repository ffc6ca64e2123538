"""GPU study: the post-processing step (R/core.R:474-481) at config 3's size (N = 10 000, ndim 5, 70 % NaN).

Wall clock around each call (every call ends with its results on the host), one process, one GPU; per case a
warm-up call, then `rounds` timed calls: median and spread (max - min).
  * today's path: _native.est_distances + core.post_mae (the host half as NumPy)
  * _native.post_metrics with est and without, once per way of reaching the caller's pageable matrices
    (pinned staging buffers filled by host threads / hipHostRegister for the length of the call / asynchronous copies
    on the pageable memory as it is); the default is marked
  * per staging, one more call with the phases timed from device events: the sums over all tiles of the uploads, the
    kernels and the downloads (they overlap, so they do not add up to the wall clock)
  * the box's host link: one pinned 256 MB buffer up and down through torch, the best of five
Every result is checked against the first: est bit for bit, sum and count bit for bit across stagings.

usage: python tests/study/post_metrics_timing.py [--n 10000] [--dim 5] [--missing 0.7] [--rounds 5] [--codes]"""
import argparse
import os
import sys
import time

import numpy as np

try:   # torch's HIP runtime has to be the first one a process loads (tests/conftest.py)
    import torch
except Exception:  # pragma: no cover
    torch = None

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from topolow_amd import _native, core  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10000)
ap.add_argument("--dim", type=int, default=5)
ap.add_argument("--missing", type=float, default=0.7)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--codes", action="store_true", help="also pass an int32 code matrix (1.5 times the upload)")
args = ap.parse_args()


def timed(fn, rounds):
    fn()   # warm-up
    secs, out = [], None
    for _ in range(rounds):
        t0 = time.perf_counter()
        out = fn()
        secs.append(time.perf_counter() - t0)
    return float(np.median(secs)), max(secs) - min(secs), out


def line(label, med, spread, extra=""):
    print(f"  {label:<46s} median {med * 1e3:9.1f} ms   spread {spread * 1e3:8.1f} ms   {extra}", flush=True)


rng = np.random.default_rng(0)
n, dim = args.n, args.dim
p = rng.normal(size=(n, dim)) * 3.0
values = np.asfortranarray(rng.uniform(0.0, 12.0, size=(n, n)))
values[rng.random((n, n)) < args.missing] = np.nan
codes = np.asfortranarray(rng.choice(np.array([0, 0, 0, 1, -1], np.int32), size=(n, n))) if args.codes else None
print(f"# post-metrics at n = {n}, ndim = {dim}, {args.missing:.0%} NaN, codes: {codes is not None}; "
      f"{args.rounds} rounds after a warm-up; values {values.nbytes / 1e6:.0f} MB, est {n * n * 8 / 1e6:.0f} MB")

if torch is not None and torch.cuda.is_available():
    host = torch.empty(256 << 20, dtype=torch.uint8).pin_memory()
    dev = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    best = {"up": 0.0, "down": 0.0}
    for _ in range(5):
        for key, (dst, src) in (("up", (dev, host)), ("down", (host, dev))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dst.copy_(src, non_blocking=True)
            torch.cuda.synchronize()
            best[key] = max(best[key], host.numel() / (time.perf_counter() - t0) / 1e9)
    print(f"# host link, pinned 256 MB copies: {best['up']:.1f} GB/s up, {best['down']:.1f} GB/s down "
          f"(so {values.nbytes / best['up'] / 1e6:.0f} ms for values up, {n * n * 8 / best['down'] / 1e6:.0f} ms for est down)")
    del host, dev
    torch.cuda.empty_cache()
else:
    print("# host link: not measured (no torch device)")

print("today's path")
med_e, sp_e, est0 = timed(lambda: _native.est_distances(p), args.rounds)
line("_native.est_distances", med_e, sp_e)
matrix = core.coded_matrix(values if codes is None else np.where(codes == 0, values, np.nan))
med_m, sp_m, mae0 = timed(lambda: core.post_mae(matrix, est0), max(2, args.rounds // 2))
line("core.post_mae (host, NumPy)", med_m, sp_m)
line("both", med_e + med_m, sp_e + sp_m)

print("topolow_post_metrics")
first = None
for staging in ("pinned", "register", "pageable"):
    mark = " (default)" if _native.POST_STAGINGS[staging] == 1 else ""
    for want in (True, False):
        try:
            med, sp, (est, s, c) = timed(lambda: _native.post_metrics(p, values, codes, want_est=want, staging=staging),
                                         args.rounds)
        except _native.NativeError as e:   # an error code, e.g. a range the runtime will not register
            print(f"  staging {staging}: refused by the runtime: {e}", flush=True)
            break
        if first is None:
            first = (s, c)
            assert np.array_equal(est, est0), "est differs from topolow_est_distances"
            rel = abs(_native.mae_of(s, c) - mae0) / mae0
            assert rel <= 1e-12, rel
            print(f"  # mae {_native.mae_of(s, c)!r} against post_mae {mae0!r}: relative difference {rel:.2e}")
        assert (s, c) == first, (staging, want, s, c, first)
        if want:
            assert np.array_equal(est, est0)
        line(f"staging {staging}{mark}, {'with' if want else 'without'} est", med, sp,
             f"{(med_e + med_m) / med:6.1f} x today's path")
        del est
    else:
        ph = []
        _native.post_metrics(p, values, codes, want_est=True, staging=staging, phases=ph)
        print(f"  {'':<46s} phases (device events, summed over tiles): upload {ph[0] * 1e3:.1f} ms, "
              f"kernels {ph[1] * 1e3:.1f} ms, download {ph[2] * 1e3:.1f} ms", flush=True)
