"""What a fold costs on a resident session, against what it would cost without one (a measurement, not a test).

Config 3's generator (topolow_amd/synthetic.py) at N points (default 10 000), 5 folds, ndim 5, f32 slab schedule:
  device  hold_out + restore_held_out + score_pairs of a fold on a session that holds the full matrix
          against a fresh Session + load_coo + set_edges of the same fold's list (encode + upload)
  host    topolow_cv_fold_pairs (no edge list) against topolow_cv_fold (edge vector + sort) on the same picks
Wall time around calls that return with the device idle; the median over the folds (the first fold of each kind also
pays one-time allocations and is reported apart).  Usage: python tests/study/cv_session_cost.py [N] [out.json]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from topolow_amd import _native, core, cv, synthetic


def timed(fn, *a):
    t0 = time.perf_counter()
    out = fn(*a)
    return out, time.perf_counter() - t0


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    folds, ndim = 5, 5
    m = core.coded_matrix(synthetic.make_problem(n, latent_dim=5, missing=0.7, seed=12345).dissimilarity)
    fb = cv.FoldBuilder(m)
    cells = fb.cells()
    picks = fb.folds(folds, np.random.default_rng(1))
    up = fb.rows < fb.cols
    full = (fb.rows[up], fb.cols[up], fb.vals[up], fb.codes[up])
    deg = np.bincount(fb.rows, minlength=n).astype(np.int32)
    init = synthetic.initial_positions(m.values, ndim, 3)

    s = _native.Session(n, ndim, precision="f32")
    s.set_relabel(12345)
    _, t_full_load = timed(lambda: (s.load_coo(*full, deg), s.set_edges(*full)))
    rows = []
    for h in picks:
        fold, t_fold = timed(_native.cv_fold, cells, h, False, False)
        pairs, t_pairs = timed(_native.cv_fold_pairs, cells, h, False, False)
        order, fdeg, vmax, n_edges, (pi, pj), (si, sj, st) = pairs
        _, t_hold = timed(s.hold_out, pi, pj, fdeg)
        s.set_positions(init)
        s.begin(3, 5.0, 0.01, 0.01, 1e-4, 5, 3, 1)
        s.run()
        s.finish(download=False)
        _, t_score = timed(s.score_pairs, si, sj, st)
        _, t_restore = timed(s.restore_held_out, deg)
        # the same fold without a resident session: a new session, the fold's list encoded and uploaded
        fo, fd, ei, ej, ed, et = fold[:6]
        caller = np.arange(n) if fo is None else fo
        fdeg_caller = np.empty(n, np.int32)
        fdeg_caller[caller] = fd

        def fresh():
            f = _native.Session(n, ndim, precision="f32")
            f.set_relabel(12345)
            f.load_coo(caller[ei], caller[ej], ed, et, fdeg_caller)
            f.set_edges(caller[ei], caller[ej], ed, et)
            return f
        f, t_fresh = timed(fresh)
        f.close()
        rows.append(dict(picks=int(h.size), held_pairs=int(pi.size), scored=int(si.size), hold_out_s=t_hold,
                         score_s=t_score, restore_s=t_restore, session_fold_s=t_hold + t_score + t_restore,
                         fresh_load_s=t_fresh, cv_fold_s=t_fold, cv_fold_pairs_s=t_pairs))
        print(rows[-1], flush=True)
    s.close()
    med = {k: float(np.median([r[k] for r in rows])) for k in rows[0] if k.endswith("_s")}
    out = dict(n=n, folds=folds, ndim=ndim, cells=int(fb.rows.size), full_load_s=t_full_load, first_fold=rows[0],
               median=med)
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as fh:
            json.dump(dict(out, per_fold=rows), fh, indent=1)


if __name__ == "__main__":
    main()
