"""The host forms of topolow_amd.subsample -- check_matrix_connectivity and subsample_dissimilarity_matrix against the
reference's documented behaviour (R/utils.R:186-196, 199-253, 321-463).  No device."""
import warnings

import numpy as np
import pytest

import topolow_amd
from topolow_amd import core, subsample

NA = np.nan


def _two_cliques(a, b):
    """Points 0..a-1 all measured against each other, points a..a+b-1 too, nothing in between."""
    n = a + b
    D = np.full((n, n), NA)
    D[:a, :a] = 1.0
    D[a:, a:] = 2.0
    np.fill_diagonal(D, 0.0)
    return D


def _brute_labels(values):
    """Components by a depth-first walk, cell by cell: the definition, not the algorithm under test."""
    n = values.shape[0]
    adj = ~np.isnan(values)
    adj = adj | adj.T
    lab = np.full(n, -1)
    for s in range(n):
        if lab[s] >= 0:
            continue
        stack, lab[s] = [s], s
        while stack:
            x = stack.pop()
            for y in np.flatnonzero(adj[x]):
                if y != x and lab[y] < 0:
                    lab[y] = s
                    stack.append(y)
    off = ~np.eye(n, dtype=bool)
    return lab, int(np.sum(~np.isnan(values) & off))


def test_the_functions_are_exported():
    assert topolow_amd.check_matrix_connectivity is subsample.check_matrix_connectivity
    assert topolow_amd.subsample_dissimilarity_matrix is subsample.subsample_dissimilarity_matrix
    assert {"check_matrix_connectivity", "subsample_dissimilarity_matrix"} <= set(topolow_amd.__all__)


def test_the_reference_examples():
    connected = np.array([0, 1, 2, 1, 0, 1.5, 2, 1.5, 0]).reshape(3, 3)
    res = subsample.check_matrix_connectivity(connected)
    assert res == dict(is_connected=True, n_components=1, completeness=1.0, n_points=3, n_measurements=3.0)
    islands = np.full((4, 4), NA)
    np.fill_diagonal(islands, 0.0)
    islands[0, 1] = islands[1, 0] = 1.0
    islands[2, 3] = islands[3, 2] = 1.0
    res = subsample.check_matrix_connectivity(islands)
    assert res["is_connected"] is False and res["n_components"] == 2
    assert res["n_points"] == 4 and res["n_measurements"] == 2.0 and res["completeness"] == 4 / 12


def test_either_cell_makes_an_edge_and_counts_one_half():
    D = _two_cliques(3, 3)
    D[4, 1] = 7.0                                   # the lower triangle only
    res = subsample.check_matrix_connectivity(D)
    assert res["is_connected"] and res["n_components"] == 1
    assert res["n_measurements"] == (6 + 6 + 1) / 2 and res["completeness"] == 13 / 30
    labels, cells = subsample.component_labels(D)
    assert labels.tolist() == [0] * 6 and cells == 13


def test_an_isolated_point_is_a_component_whatever_its_diagonal():
    D = _two_cliques(4, 1)
    res = subsample.check_matrix_connectivity(D)
    assert res["n_components"] == 2 and not res["is_connected"]
    labels, _ = subsample.component_labels(D)
    assert labels.tolist() == [0, 0, 0, 0, 4]
    D[4, 4] = NA
    assert subsample.component_labels(D)[0].tolist() == [0, 0, 0, 0, 4]


def test_thresholds_and_infinite_cells_are_measured():
    D = np.array([["0", ">5", "NA"], [">5", "0", "<2"], ["NA", "<2", "0"]], dtype=object)
    assert subsample.check_matrix_connectivity(D)["is_connected"]
    E = np.full((3, 3), NA)
    E[0, 1] = np.inf
    E[2, 1] = np.inf
    assert subsample.check_matrix_connectivity(E) == dict(is_connected=True, n_components=1, completeness=2 / 6,
                                                         n_points=3, n_measurements=1.0)


@pytest.mark.parametrize("n,seed", [(2, 0), (17, 1), (64, 2), (65, 3), (300, 4)])
def test_labels_are_the_smallest_member_on_sparse_random_graphs(n, seed):
    rng = np.random.default_rng(seed)
    D = np.where(rng.random((n, n)) < 1.2 / n, 1.0, NA)     # about one cell per point: many components, long paths
    labels, cells = subsample.component_labels(D)
    want, want_cells = _brute_labels(D)
    assert np.array_equal(labels, want) and cells == want_cells


def test_a_long_chain_with_shuffled_labels():
    n = 500
    perm = np.random.default_rng(9).permutation(n)
    D = np.full((n, n), NA)
    D[perm[:-1], perm[1:]] = 1.0
    labels, cells = subsample.component_labels(D)
    assert labels.tolist() == [0] * n and cells == n - 1


def test_the_stop_texts():
    with pytest.raises(ValueError, match="^dissimilarity_matrix must be a matrix$"):
        subsample.check_matrix_connectivity([1.0, 2.0])
    with pytest.raises(ValueError, match="^dissimilarity_matrix must be square$"):
        subsample.check_matrix_connectivity(np.zeros((2, 3)))
    with pytest.raises(ValueError, match="^dissimilarity_matrix must have at least 2 points$"):
        subsample.check_matrix_connectivity(np.zeros((1, 1)))
    with pytest.raises(ValueError, match="^dissimilarity_matrix must be a matrix$"):
        subsample.subsample_dissimilarity_matrix(np.zeros(4), 2)
    with pytest.raises(ValueError, match="^dissimilarity_matrix must be square$"):
        subsample.subsample_dissimilarity_matrix(np.zeros((2, 3)), 2)
    for bad in (1, 1.9, "3", None, NA):
        with pytest.raises(ValueError, match="^sample_size must be a numeric value >= 2$"):
            subsample.subsample_dissimilarity_matrix(np.zeros((5, 5)), bad)


def test_the_sparse_but_connected_warning_is_the_reference_text():
    n = 30
    D = np.full((n, n), NA)
    D[np.arange(n - 1), np.arange(1, n)] = 1.0      # a chain: connected, 29 cells of 870
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = subsample.check_matrix_connectivity(D)
    assert res["is_connected"]
    assert [str(x.message) for x in w] == [
        "Network is connected but sparse (3.3% complete). This may lead to poor optimization. "
        "Consider using more data points."]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        subsample.check_matrix_connectivity(D, min_completeness=0.01)
        subsample.check_matrix_connectivity(_two_cliques(15, 15), min_completeness=0.9)   # sparse, NOT connected
    assert w == []


def test_a_sample_size_of_n_or_more_returns_the_matrix_itself(capsys):
    D = core.RMatrix(_two_cliques(3, 2), list("abcde"))
    res = subsample.subsample_dissimilarity_matrix(D, 5.7, verbose=True, rng=np.random.default_rng(0))
    assert res["subsampled_matrix"] is D and res["selected_indices"].tolist() == [0, 1, 2, 3, 4]
    assert res["selected_names"] == list("abcde") and res["attempt_number"] == 1
    assert res["is_connected"] is False and res["n_components"] == 2 and res["completeness"] == 8 / 20
    assert capsys.readouterr().out == "Requested sample_size (5) >= matrix size (5). Using full matrix.\n"
    assert set(res) == {"subsampled_matrix", "selected_indices", "selected_names", "is_connected", "n_components",
                        "completeness", "attempt_number"}
    rng = np.random.default_rng(3)
    subsample.subsample_dissimilarity_matrix(D, 9, rng=rng)
    assert rng.bit_generator.state == np.random.default_rng(3).bit_generator.state      # nothing is drawn


def test_the_retry_loop_ends_with_the_reference_error_when_no_draw_can_be_connected(capsys):
    """Two cliques of 4: any 5 points hold members of both, so every draw has exactly 2 components."""
    D = _two_cliques(4, 4)
    rng = np.random.default_rng(1)
    with pytest.raises(ValueError) as e:
        subsample.subsample_dissimilarity_matrix(D, 5, max_attempts=3, rng=rng, verbose=True)
    text = str(e.value)
    assert text.startswith("Failed to obtain a connected subsample after 3 attempts.\n"
                           "  Final sample size tried: 5 (started at 5)\n"
                           "  Original matrix size: 8\n"
                           "  Last attempt had 2 components with ")
    assert text.endswith("% completeness\n\nPossible solutions:\n"
                         "  1. Increase opt_subsample (current: 5)\n"
                         "  2. Reduce number of CV folds\n"
                         "  3. Use full dataset (opt_subsample = NULL)\n"
                         "  4. Check if your data has inherent disconnected groups")
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 5 and lines[1] == "  Attempt 2/3..." and lines[3] == "  Attempt 3/3..."
    for q in (0, 2, 4):                              # 4 + 1 points: 12 cells of 20; 3 + 2: 8 of 20
        assert lines[q] in ("  X Not connected (2 components, 60.0% complete)",
                            "  X Not connected (2 components, 40.0% complete)")
    ref = np.random.default_rng(1)                   # three draws were made, each as make_folds draws
    for _ in range(3):
        ref.choice(8, size=5, replace=False)
    assert rng.bit_generator.state == ref.bit_generator.state


def test_a_connected_draw_and_preserve_order(capsys):
    pts = np.random.default_rng(2).normal(size=(40, 2))
    full = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1))
    names = ["p%d" % q for q in range(40)]
    D = core.RMatrix(full, names)
    want = np.random.default_rng(7).choice(40, size=12, replace=False)
    res = subsample.subsample_dissimilarity_matrix(D, 12.9, rng=np.random.default_rng(7), verbose=True)
    assert np.array_equal(res["selected_indices"], want) and sorted(want.tolist()) != want.tolist()
    assert res["selected_names"] == [names[q] for q in want] and res["subsampled_matrix"].names == res["selected_names"]
    assert np.array_equal(res["subsampled_matrix"].values, full[np.ix_(want, want)])
    assert res["is_connected"] is True and res["n_components"] == 1 and res["completeness"] == 1.0
    assert res["attempt_number"] == 1 and "handle" not in res
    assert capsys.readouterr().out == "  [OK] Connected subsample obtained (attempt 1, size 12, 100.0% complete)\n"
    res = subsample.subsample_dissimilarity_matrix(full, 12, rng=np.random.default_rng(7), preserve_order=True)
    assert np.array_equal(res["selected_indices"], np.sort(want)) and res["selected_names"] is None
    assert np.array_equal(res["subsampled_matrix"], full[np.ix_(np.sort(want), np.sort(want))])


def test_a_later_attempt_succeeds():
    """A clique of 9 and one stranger: a draw of 6 is connected iff it misses the stranger; the attempt is counted."""
    D = _two_cliques(9, 1)
    for seed in range(40):
        draws = np.random.default_rng(seed)
        first = draws.choice(10, size=6, replace=False)
        second = draws.choice(10, size=6, replace=False)
        if 9 in first and 9 not in second:
            break
    else:
        pytest.fail("no seed among 40 whose first draw holds the stranger and whose second does not")
    res = subsample.subsample_dissimilarity_matrix(D, 6, rng=np.random.default_rng(seed))
    assert res["attempt_number"] == 2 and np.array_equal(res["selected_indices"], second)
