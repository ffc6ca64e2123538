"""The assertions of tests/test_gpu_row_owner_needles.py can see ONE pair (host only: the library's plan query and the CPU
model, no GPU).  For every launch of the table in tests/stage_needles.py, with and without thresholds, in both kinds:
the plan search finds the wanted slab within its bound; the builder's coverage conditions hold (stage_needle asserts them);
the model itself is inside the band with ratio 0 and its own fp32 arithmetic at 0.5 of the band or less; in the repel kind
a planted pair carries 0.9 of the move of its row or more; and EVERY mutation of EVERY planted cell -- the pair lost, counted
twice, its word read from the column before or after, the two rows of its wave exchanged, a row outside the block written
-- leaves the band or breaks the bit-equality of the idle and the outside rows."""
import numpy as np
import pytest

from tests import stage_needles as sn

GROUPS = sn.all_groups()


@pytest.mark.parametrize("thresholded", [False, True])
@pytest.mark.parametrize("kind", ["spring", "repel"])
@pytest.mark.parametrize("label,ndim,wide,launches", GROUPS, ids=[g[0].replace(" ", "-") for g in GROUPS])
def test_every_mutation_of_every_planted_cell_is_seen(label, ndim, wide, launches, kind, thresholded):
    exact = label.startswith("exact")
    bands = ("f64",) if exact else ("f32", "f64")
    for launch in launches:
        it, nd = sn.needle_of(launch, ndim, thresholded, kind, wide, exact)
        assert sn.shape_holds(nd.ranges, launch.shape) and it < sn.plan_search_bound(launch.n)
        assert tuple(sn._native.slab_plan(launch.n, launch.stages, sn.PLAN_SEED, it)[launch.slot]) == nd.ranges
        base = sn.model_output(nd, nd.want_exact)
        for band in bands:
            assert sn.hold(nd, base, band, exact=exact) == 0.0
        ratio = sn.model_f32_ratio(nd)
        share = sn.planted_share(nd) if kind == "repel" else (1.0, 0.0)
        print("%s n %d stages %d slot %d %s rows %s: it %d of at most %d, ranges %s, %d cells, fp32 model / band %.3f%s" %
              (label, launch.n, launch.stages, launch.slot, launch.shape, launch.rows, it, sn.plan_search_bound(launch.n),
               nd.ranges, len(nd.cells), ratio, "" if kind == "spring" else ", planted share %.3f" % share[0]))
        assert ratio <= 0.5
        assert share[0] >= 0.9 and share[1] <= 0.1, share
        # a planted cell's term is what the model takes for it: the row's move is the sum of its cells' terms
        start = nd.call.initial_positions
        if kind == "spring":
            for i in {i for i, _ in nd.cells}:
                cs = [c for c in np.flatnonzero(np.isfinite(nd.call.dissimilarity_matrix[i]) & sn.in_ranges(nd.n, nd.ranges))
                      if c != i]
                total = sum(sn.cell_term(nd, i, int(c), exact) for c in cs)
                assert np.abs(start[i] - nd.want_exact[i] - total).max() <= 1e-13 * np.abs(total).max() + \
                    2.0 ** -50 * np.abs(start[i]).max(), i
        # the f64 band is the tighter one at every point: what leaves the fp32 band leaves the f64 band too
        assert exact or sn.f64_band_is_the_tighter(nd)
        seen = 0
        for name, cell, out in sn.mutations(nd, exact):
            with pytest.raises(AssertionError):
                sn.hold(nd, out, bands[0], exact=exact)
                print("NOT SEEN:", label, launch, kind, thresholded, name, cell)
            seen += 1
        assert seen >= 5 * len(nd.cells)       # lost, doubled, a neighbouring column, one or two of the wave, stray


def test_the_table_reaches_every_instance_and_shape():
    """All 24 plain fp32 instances and the f64 instance at every instantiated ndim (with and without thresholds: the
    parametrisation above), the exact instance, the wide ones; each with a wrapped slab whose two parts both exceed its
    widest chunk, a 4-column part at either end, and a slab narrower than a group."""
    labels = {g[0] for g in GROUPS}
    for precision in ("f32", "f64"):
        for ndim in sn.PLAIN_DIMS:
            launches = sn.plain_launches(precision, ndim)
            assert any(tuple(launches) == tuple(g[3]) and g[1] == ndim for g in GROUPS)
            n = sn.main_n(precision, ndim)
            assert n == 2 * sn.WIDEST_CHUNK[n] + 256 + 7 and n % 4 == 3
            got = {l.shape[0] for l in launches if l.n == n}
            assert {"long", "tail4", "head4", "flat"} <= got
            it, rg = sn.find_iteration(n, 16, sn.PLAN_SEED, ("wrapped",), 0)
            assert rg[1] - rg[0] < 256 and rg[3] - rg[2] < 256
            it, rg = sn.find_iteration(n, 1, sn.PLAN_SEED, ("long", sn.WIDEST_CHUNK[n]), 0)
            assert min(rg[1] - rg[0], rg[3] - rg[2]) > sn.WIDEST_CHUNK[n]
    for ndim in sn.ERR_DIMS:            # the ERR instances: an even row count, the same three wrapped shapes, a narrow slab
        launches = sn.err_launches(ndim)
        assert any(tuple(launches) == tuple(g[3]) and g[1] == ndim and g[0].startswith("err") for g in GROUPS)
        n = sn.main_n("f32", ndim) + 1
        assert n % 2 == 0 and {"long", "tail4", "head4"} <= {l.shape[0] for l in launches if l.n == n}
        it, rg = sn.find_iteration(n, 1, sn.PLAN_SEED, ("long", sn.WIDEST_CHUNK[n]), 0)
        assert min(rg[1] - rg[0], rg[3] - rg[2]) > sn.WIDEST_CHUNK[n] == sn.WIDEST_CHUNK[n - 1]
        assert any(l.n == 70 for l in launches)
    for launches in [sn.wide_launches()] + [sn.exact_launches(ndim) for ndim in sn.EXACT_DIMS]:
        assert {"tail4", "head4"} <= {l.shape[0] for l in launches} and any(l.n == 70 for l in launches)
    assert any(l.n == 5 for ndim in sn.EXACT_DIMS for l in sn.exact_launches(ndim))
    assert any(l.startswith("exact") for l in labels) and any(l.startswith("wide") for l in labels)
    assert any(launch.n % 4 == 1 for g in GROUPS for launch in g[3])


@pytest.mark.parametrize("label,ndim,wide,launches", [g for g in GROUPS if g[0].startswith(("plain", "err", "exact"))],
                         ids=[g[0].replace(" ", "-") for g in GROUPS if g[0].startswith(("plain", "err", "exact"))])
def test_repel_problems_reach_every_special_column_from_a_special_row(label, ndim, wide, launches):
    """A repel row takes one cell, so one problem's special rows reach len(srows) special columns only.  The thresholded
    problem serves the columns from where the plain one's special rows stopped: of the launch with both parts long, the
    two together put every special column on a special row (and each alone on an ordinary row)."""
    launch = launches[0]
    assert launch.shape[0] == "long" and launch.rows is None
    on_special, on_ordinary = set(), []
    for thresholded in (False, True):
        _, nd = sn.needle_of(launch, ndim, thresholded, "repel", wide)
        assert 2 * len(nd.srows) >= len(nd.labels)
        on_special |= {c for i, c in nd.cells if i in nd.srows}
        on_ordinary.append({c for i, c in nd.cells if i not in nd.srows})
    assert on_special == set(nd.labels), sorted(set(nd.labels) - on_special)
    assert on_ordinary[0] == on_ordinary[1] == set(nd.labels)
