"""What a fold costs when it is prepared on the device from a prepared handle, against the host's preparation from the
cell list (a measurement, not a test).

Config 3's generator (topolow_amd/synthetic.py) at N points (default 10 000), 5 folds, ndim 5, f32 slab schedule, in
one process on one box:
  resident  per fold, from topolow_layout_prep_fold_seconds after a one-fold topolow_layout_prep_cv_sweep: the fold
            preparation (mark + masked sums + order + compaction), the hold-out from device pairs, the score, the restore
  host      per fold: topolow_cv_fold_pairs, topolow_session_hold_out, _score_pairs, _restore_held_out on a session
            that holds the full matrix
  sweep     the wall time of all folds in one call by either route (ITERS iterations per fold), and what each route
            pays once: the handle (upload + both passes) against the library's cell list
The median over the folds; the first fold of each kind also pays one-time allocations and is reported apart.
Usage: python tests/study/cv_resident_cost.py [N] [out.json] [ITERS]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from topolow_amd import _native, core, cv, synthetic


def timed(fn, *a, **kw):
    t0 = time.perf_counter()
    out = fn(*a, **kw)
    return out, time.perf_counter() - t0


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    iters = int(sys.argv[3]) if len(sys.argv) > 3 else 100
    folds, ndim = 5, 5
    m = core.coded_matrix(synthetic.make_problem(n, latent_dim=5, missing=0.7, seed=12345).dissimilarity)
    fb = cv.FoldBuilder(m)
    rng = np.random.default_rng(1)
    picks = fb.folds(folds, rng)
    draws = [rng.random((ndim, n - 1)) for _ in picks]
    seeds = [int(rng.integers(0, 2 ** 63 - 1)) for _ in picks]
    par = lambda k: ([ndim] * k, [5.0] * k, [0.01] * k, [0.01] * k)

    # -- the resident route: one upload, then per fold a one-fold sweep whose steps the handle times
    handle, t_handle = timed(_native.PreparedHandle, m.values, None, preserve_order=True)
    rows = []
    for f, h in enumerate(picks):
        out, t_call = timed(handle.cv_sweep, False, False, *par(1), [h], [draws[f]], [seeds[f]], 3, 1e-4, 5, 3,
                            precision="f32", schedule="slab")
        prep, hold, score, restore = handle.fold_seconds()
        rows.append(dict(picks=int(h.size), scored=int(out[1][0]), route=int(out[6][0]), resident_prepare_s=prep,
                         resident_hold_out_s=hold, resident_score_s=score, resident_restore_s=restore,
                         resident_fold_s=prep + hold + score + restore, resident_one_fold_call_s=t_call))
        print(rows[-1], flush=True)
    res_sweep, t_res_sweep = timed(handle.cv_sweep, False, False, *par(folds), picks, draws, seeds, iters, 1e-4, 5, 3,
                                   precision="f32", schedule="slab")
    handle.close()

    # -- the host route, same process: the cell list, the fold from it, the three session steps
    cells, t_cells = timed(fb.cells)
    up = fb.rows < fb.cols
    full = (fb.rows[up], fb.cols[up], fb.vals[up], fb.codes[up])
    deg = np.bincount(fb.rows, minlength=n).astype(np.int32)
    init = synthetic.initial_positions(m.values, ndim, 3)
    s = _native.Session(n, ndim, precision="f32")
    s.set_relabel(12345)
    s.load_coo(*full, deg)
    s.set_edges(*full)
    for f, h in enumerate(picks):
        pairs, t_pairs = timed(_native.cv_fold_pairs, cells, h, False, False)
        order, fdeg, vmax, n_edges, (pi, pj), (si, sj, st) = pairs
        _, t_hold = timed(s.hold_out, pi, pj, fdeg)
        s.set_positions(init)
        s.begin(3, 5.0, 0.01, 0.01, 1e-4, 5, 3, 1)
        s.run()
        s.finish(download=False)
        _, t_score = timed(s.score_pairs, si, sj, st)
        _, t_restore = timed(s.restore_held_out, deg)
        rows[f].update(held_pairs=int(pi.size), host_cv_fold_pairs_s=t_pairs, host_hold_out_s=t_hold,
                       host_score_s=t_score, host_restore_s=t_restore,
                       host_fold_s=t_pairs + t_hold + t_score + t_restore)
        print({k: v for k, v in rows[f].items() if k.startswith("host")}, flush=True)
    s.close()
    host_sweep, t_host_sweep = timed(_native.cv_sweep_session, cells, False, False, *par(folds), picks, draws, seeds,
                                     iters, 1e-4, 5, 3, precision="f32", schedule="slab")
    same = all(np.array_equal(a, b) for a, b in zip(res_sweep[:5], host_sweep[:5]))
    med = {k: float(np.median([r[k] for r in rows])) for k in rows[0] if k.endswith("_s")}
    out = dict(n=n, folds=folds, ndim=ndim, iterations_per_fold=iters, cells=int(fb.rows.size), median=med,
               first_fold=rows[0], handle_create_s=t_handle, cell_list_s=t_cells, resident_sweep_s=t_res_sweep,
               session_sweep_s=t_host_sweep, resident_sweep_device_s=res_sweep[5], session_sweep_device_s=host_sweep[5],
               sweeps_equal_bit_for_bit=bool(same), order_routes=[int(x) for x in res_sweep[6]])
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as fh:
            json.dump(dict(out, per_fold=rows), fh, indent=1)


if __name__ == "__main__":
    main()
