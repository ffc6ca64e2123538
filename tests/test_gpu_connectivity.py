"""Components of the measurement graph on the device (run with -m gpu): PreparedHandle.connectivity -- labels,
n_components, n_cells -- against the NumPy host form subsample.component_labels, on handles of either layout
(transposed = 1 and 0) and on a handle that declined its ordering (topolow_amd/csrc/relax_prep_graph.h).

The shapes are small where the kernels can go wrong: one word, the edges of the 64-bit words and of the 4-line blocks of
the hook kernel, ragged last words, long paths, cells that exist in one triangle only."""
import math

import numpy as np
import pytest

from topolow_amd import _native, subsample

pytestmark = pytest.mark.gpu

NA = np.nan


def check(D, codes=None, subset=None, layouts=("C", "F"), **handle_kw):
    """Device against host on the induced submatrix; returns the device's (n_components, n_cells, labels, rounds)."""
    D = np.asarray(D, dtype=np.float64)
    idx = np.arange(D.shape[0]) if subset is None else np.asarray(subset)
    want, want_cells = subsample.component_labels(D[np.ix_(idx, idx)])
    want_nc = int(np.sum(want == np.arange(idx.shape[0])))
    got = None
    for layout in layouts:
        with _native.PreparedHandle(D, codes, layout=layout, **handle_kw) as h:
            nc, cells, labels = h.connectivity(subset)
            rounds, _ = h.graph_stats()
        assert labels.dtype == np.int32 and np.array_equal(labels, want), layout
        assert (nc, cells) == (want_nc, want_cells), layout
        assert 1 <= rounds <= idx.shape[0] + 1
        got = (nc, cells, labels, rounds)
    return got


def chain(n, seed):
    """A path through all n points in a shuffled order (seed None: in index order), one cell per link, in one triangle
    or the other as it falls."""
    perm = np.arange(n) if seed is None else np.random.default_rng(seed).permutation(n)
    D = np.full((n, n), NA)
    D[perm[:-1], perm[1:]] = 1.0
    return D


def sparse(n, per_point, seed):
    return np.where(np.random.default_rng(seed).random((n, n)) < per_point / n, 1.0, NA)


def test_two_points():
    assert check(np.array([[0.0, 3.0], [3.0, 0.0]]))[:2] == (1, 2)
    assert check(np.array([[0.0, NA], [2.0, NA]]))[:2] == (1, 1)           # the lower cell alone
    assert check(np.array([[0.0, NA], [NA, 0.0]]))[:2] == (2, 0)
    big = np.full((5, 5), NA)
    big[3, 1] = 1.0
    assert check(big, subset=[3, 1])[:2] == (1, 1) and check(big, subset=[1, 3])[:2] == (1, 1)
    assert check(big, subset=[4, 3])[:2] == (2, 0)


def test_a_chain_of_300_with_shuffled_labels():
    nc, cells, labels, _ = check(chain(300, 5))
    assert nc == 1 and cells == 299 and not labels.any()


@pytest.mark.parametrize("seed", [11, None], ids=["shuffled", "in-order"])
def test_a_chain_of_4097_finishes_and_is_right(seed):
    """65 words a line (the last holds one bit), 1 025 hook blocks (the last holds one line), 17 jump blocks.  A path's
    roots form a path; a round hooks every root that has a smaller neighbouring root, so at most every second root
    survives it: 4 097 -> 1 in 13 rounds, and one more finds nothing to do -- not the 4 096 of the diameter."""
    nc, cells, labels, rounds = check(chain(4097, seed), layouts=("C",), preserve_order=True)
    assert nc == 1 and cells == 4096 and not labels.any()
    print("rounds", rounds)
    assert rounds <= math.ceil(math.log2(4097)) + 1


@pytest.mark.parametrize("n", [65, 257, 1025])
@pytest.mark.parametrize("per_point", [1.2, 6.0], ids=["many-components", "few-components"])
def test_sizes_past_the_word_and_block_boundaries(n, per_point):
    nc, _, _, _ = check(sparse(n, per_point, n))
    assert nc > 1 if per_point < 2 else nc >= 1


def test_two_cliques_joined_by_one_cell_of_the_lower_triangle():
    n, a = 130, 70
    D = np.full((n, n), NA)
    D[:a, :a] = 1.0
    D[a:, a:] = 2.0
    assert check(D)[0] == 2
    D[100, 3] = 5.0                                                  # row > column: the lower triangle only
    nc, cells, labels, _ = check(D)
    assert nc == 1 and cells % 2 == 1 and cells == a * (a - 1) + (n - a) * (n - a - 1) + 1
    assert not labels.any()


def test_a_point_with_nothing_but_its_diagonal():
    D = sparse(90, 8.0, 3)
    D[40, :] = NA
    D[:, 40] = NA
    D[40, 40] = 0.0
    nc, _, labels, _ = check(D)
    assert labels[40] == 40 and np.sum(labels == 40) == 1 and nc >= 2


def test_threshold_codes_and_infinite_cells_are_measured():
    n = 100
    rng = np.random.default_rng(8)
    D = np.full((n, n), NA)
    codes = np.zeros((n, n), dtype=np.int8)
    perm = rng.permutation(n)
    for q, (r, c) in enumerate(zip(perm[:-1], perm[1:])):            # a path whose every link is coded or infinite
        D[r, c] = np.inf if q % 3 == 0 else 4.0
        codes[r, c] = (0, 1, -1)[q % 3]
    nc, cells, _, _ = check(D, codes)
    assert nc == 1 and cells == n - 1


def test_a_subset_whose_components_meet_only_outside_it():
    """n = 700: two groups of points, each connected within itself, joined through hub points alone.  A subset of 333
    without a hub, unsorted, falls apart into the two groups; the whole matrix is connected."""
    n = 700
    rng = np.random.default_rng(21)
    group = np.arange(n) % 2
    hubs = np.array([10, 351, 699])
    D = np.full((n, n), NA)
    for g in (0, 1):
        members = rng.permutation(np.flatnonzero(group == g))
        D[members[:-1], members[1:]] = 1.0                           # a path through the group
        extra = rng.choice(members, size=(200, 2))
        D[extra[:, 0], extra[:, 1]] = 2.0
    D[hubs, :] = 3.0                                                 # a hub is measured against everybody
    assert check(D, layouts=("C",))[0] == 1
    pool = np.setdiff1d(np.arange(n), hubs)
    subset = rng.permutation(pool)[:333]
    assert not np.array_equal(subset, np.sort(subset))
    nc, _, labels, _ = check(D, subset=subset)
    assert nc >= 2
    assert len({int(labels[q]) for q in range(333) if group[subset[q]] == 0} &
               {int(labels[q]) for q in range(333) if group[subset[q]] == 1}) == 0
    with_hub = np.concatenate([subset[:332], hubs[:1]])
    assert check(D, subset=with_hub, layouts=("F",))[0] < nc


def test_a_handle_that_declined_its_ordering_still_answers():
    D = sparse(150, 3.0, 2)
    D[7, 9] = -1.0                                                   # a negative cell: the device does not order
    with _native.PreparedHandle(D) as h:
        assert h.declined
    check(D)
    check(D, subset=np.random.default_rng(1).permutation(150)[:77])


def test_the_whole_matrix_and_the_identity_subset_agree():
    D = sparse(200, 2.0, 6)
    with _native.PreparedHandle(D, preserve_order=True) as h:
        a = h.connectivity()
        b = h.connectivity(np.arange(200))
        assert a[:2] == b[:2] and np.array_equal(a[2], b[2])
        with pytest.raises(_native.NativeError, match="repeated"):
            h.connectivity([1, 2, 2])
        with pytest.raises(_native.NativeError, match="out of range"):
            h.connectivity([1, 200])
        c = h.connectivity()                                          # the refusals left the handle as it was
        assert a[:2] == c[:2] and np.array_equal(a[2], c[2])
