"""That the assertions of tests/test_gpu_check_pairs.py see one pair (CPU only; what tests/test_symm_needle_one_pair.py is
for the moves): on every problem those tests use, with the oracle alone, a list with one contributing pair removed, counted
twice or moved to the neighbouring cell, or with one tie's code flipped, falls outside them, and the list itself passes.
Also what makes the planted cells reviewable: every seam class of check_needles.seam_cells holds a contributing pair."""
import numpy as np
import pytest

from tests import check_needles as cn

PROBLEMS = sorted(set(cn.DENSE_CASES + cn.FUSED_CASES + (cn.BIG_DENSE, cn.PUSH_CASE)))


def _position_sets(nd):
    return (("start", nd.pos), ("x 2", 2.0 * nd.pos))


def _outside(got, want, band, trace=True):
    """The assertion on a pass's (sum, count) does not accept `got`, nor (trace) does the one on a trace's MAE.  The
    passes are held on every position set; a trace shows the ratio alone and is held on runs from the start, where the
    pair errors are bimodal (scaled by 2 they are not: a pair's error may be the mean, and the ratio cannot see it go)."""
    if cn.pass_holds(got, want, band)[0]:
        return False
    return not trace or got[1] == 0 or not cn.mae_holds(got[0] / got[1], want, band)[0]


@pytest.mark.parametrize("thresholded", [False, True])
@pytest.mark.parametrize("n,dim", PROBLEMS)
def test_one_pair_falls_outside_the_assertions(n, dim, thresholded):
    nd = cn.needle(n, dim, cn.SEED, thresholded)
    ei, ej, t, code = nd.edge_i, nd.edge_j, nd.edge_dist_dev, nd.edge_thresh
    assert len(set(zip(ei.tolist(), ej.tolist()))) == len(ei) and (ei < ej).all()
    for name, pos in _position_sets(nd):
        want = cn.oracle(pos, nd)
        band = cn.sum_band_f32(pos, ei, ej, t, code, cn.kernel_dim(dim))
        c, err, _ = cn.pair_terms(pos, ei, ej, t, code)
        assert int(c.sum()) == want[1] and float(err[c].sum()) == pytest.approx(want[0], rel=1e-12)
        # the list itself passes, as a pass's (sum, count) and as a trace's MAE
        assert cn.pass_holds(want, want, band)[0] and (want[1] == 0 or cn.mae_holds(want[0] / want[1], want, band)[0])
        if want[1] < 2:
            assert n < 16
            continue
        # one contributing pair removed / counted twice: every one of them (a pair that does not contribute changes nothing)
        for sign in (-1, 1):
            for e in err[c]:
                assert _outside((want[0] + sign * e, want[1] + sign), want, band, name == "start"), (name, sign, e)
        # one tie's code flipped between 0 and ">"
        for k in nd.ties[:2]:
            flipped = code.copy()
            flipped[k] = 1 - flipped[k]
            got = cn.orc.edge_error(pos, ei, ej, t, flipped)
            assert got[1] != want[1] and _outside(got, want, band, name == "start"), (name, k)


@pytest.mark.parametrize("thresholded", [False, True])
@pytest.mark.parametrize("n,dim", PROBLEMS)
def test_every_seam_class_holds_a_contributing_pair_whose_move_is_seen(n, dim, thresholded):
    """Per seam class: a planted pair that contributes at the start, and one whose move to the nearest free cell (of its row:
    (i, j + 1), (i, j - 1), (i, j + 2), ...; then of its column) falls outside the assertions.  (Not every single move can: the moved pair's error is
    another draw of a few units' spread, and the sum's band is a few hundredths -- a pair in a hundred lands inside it
    with the count unchanged.  Nine moves in ten are asserted to be seen.)"""
    nd = cn.needle(n, dim, cn.SEED, thresholded)
    ei, ej, t, code = nd.edge_i, nd.edge_j, nd.edge_dist_dev, nd.edge_thresh
    index = {(int(i), int(j)): k for k, (i, j) in enumerate(zip(ei, ej))}
    want = cn.oracle(nd.pos, nd)
    band = cn.sum_band_f32(nd.pos, ei, ej, t, code, cn.kernel_dim(dim))
    c, _, _ = cn.pair_terms(nd.pos, ei, ej, t, code)
    assert set(nd.planted) == {cell for v in nd.classes.values() for cell in v} and all(p in index for p in nd.planted)
    seen = {}
    for i, j in nd.planted:
        k = index[(i, j)]
        if not c[k]:
            continue
        near = [(i, j + d * sg) for d in range(1, 9) for sg in (1, -1)] + [(i + d * sg, j) for d in range(1, 9) for sg in (1, -1)]
        free = [(a, b) for a, b in near if 0 <= a < b < n and (a, b) not in index]
        if not free:
            continue
        mi, mj = ei.copy(), ej.copy()
        mi[k], mj[k] = free[0]
        seen[(i, j)] = _outside(cn.orc.edge_error(nd.pos, mi, mj, t, code), want, band)
    for name, cells in nd.classes.items():
        contributing = [cell for cell in cells if c[index[cell]]]
        assert contributing or n < 16, (name, cells)
        assert any(seen.get(cell, False) for cell in cells) or n < 16, (name, cells)
    if n >= 16:
        assert sum(seen.values()) >= 0.9 * len(seen), (sum(seen.values()), len(seen))
    # a wave whose two rows differ in holding a threshold code, both with a contributing pair to their right
    if thresholded and n >= 66:
        has_code = np.zeros(n + 1, dtype=bool)
        has_code[ei[code != 0]] = True
        has_code[ej[code != 0]] = True
        counts = np.zeros(n + 1, dtype=bool)
        counts[ei[c]] = True
        even = np.arange(0, n - 1, 2)
        assert ((has_code[even] != has_code[even + 1]) & counts[even] & counts[even + 1]).any()


@pytest.mark.parametrize("n,dim", [(2050, 5), (2113, 16), (1025, 10), (66, 5)])
def test_a_restated_dense_pass_with_a_wrong_predicate_loses_pairs(n, dim):
    """The CPU restatement of dense_error_kernel's predicates (check_needles.dense_pass_visits) visits every listed pair;
    with the diagonal test c >= i + 2 in place of c > i, or without the last group of a chunk, it loses contributing pairs,
    and what it then reduces fails the assertions."""
    nd = cn.needle(n, dim, cn.SEED, True)
    assert cn.dense_pass_visits(n, nd.edge_i, nd.edge_j).all()
    want = cn.oracle(nd.pos, nd)
    band = cn.sum_band_f32(nd.pos, nd.edge_i, nd.edge_j, nd.edge_dist_dev, nd.edge_thresh, cn.kernel_dim(dim))
    for wrong in (dict(diag=lambda c, i: c >= i + 2), dict(drop_last_group=True)):
        visited = cn.dense_pass_visits(n, nd.edge_i, nd.edge_j, **wrong)
        got = cn.oracle(nd.pos, nd, mask=visited)
        assert got[1] < want[1] and _outside(got, want, band), (wrong, got, want)


def test_the_full_list_and_the_builders_rules():
    """The 4.5-million-edge list: every pair once, the targets' margins; and the rules of the needle's targets."""
    nd = cn.full_list(*cn.FULL_LIST, cn.SEED, True)
    n = nd.n
    assert len(nd.edge_i) == n * (n - 1) // 2 == 4498500
    key = nd.edge_i.astype(np.int64) * n + nd.edge_j
    assert (nd.edge_i < nd.edge_j).all() and len(np.unique(key)) == len(key)
    for p in (nd, cn.needle(2113, 5, cn.SEED, True)):
        _, err, _ = cn.pair_terms(p.pos, p.edge_i, p.edge_j, p.edge_dist_dev, p.edge_thresh)
        off = np.ones(len(err), dtype=bool)
        off[p.ties] = False
        e = err[off]
        assert ((np.abs(e - 1.0) < 0.11) | (np.abs(e - 4.0) < 0.41)).all()             # bimodal: none near the mean
        assert 0.3 < (e < 2).mean() < 0.7
        assert np.array_equal(cn.round4(p.edge_dist_dev), p.edge_dist_dev)
        assert np.abs(p.edge_dist_dev - p.edge_dist).max() <= 2.0 ** -22 * p.edge_dist.max()
        assert set(np.unique(p.edge_thresh).tolist()) == {-1, 0, 1}
    p = cn.needle(2113, 5, cn.SEED, True)
    assert np.array_equal(p.edge_thresh[p.ties], [0, 1, -1]) and np.array_equal(p.edge_dist[p.ties], [5.0] * 3)
    want = cn.oracle(p.pos, p)
    others = np.ones(len(p.edge_i), dtype=bool)
    others[p.ties] = False
    rest = cn.oracle(p.pos, p, mask=others)
    assert want[1] == rest[1] + 1 and want[0] == rest[0]          # the exact tie counts with error 0, the strict ones do not
