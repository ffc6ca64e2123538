"""Pruning and degrees on a prepared handle (run with -m gpu): the device forms against the host forms of prune.py,
which are the specification -- kept_indices, removed_indices, every entry of stats, the warnings and the errors, on
handles of both layouts, at the shapes where the kernels of relax_prep_prune.h can go wrong (word edges, a ragged last
word, more lines than one block of waves, counts that cross many words, cells in one triangle only).  Everything is
exact: integers, masks and bit-equal arrays."""
import functools
import math
import warnings

import numpy as np
import pytest

from tests import prune_problems as pp
from tests import resident_helpers as rh
from tests.test_gpu_subsample_handle import FETCHED, assert_same_handle
from topolow_amd import _native, core, prune, subsample

pytestmark = pytest.mark.gpu

LAYOUTS = ["C", "F"]


def run(D, **kw):
    """(result or None, [warning texts], error text or None) of prune_sparse_matrix, verbose off."""
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        try:
            out, err = prune.prune_sparse_matrix(D, verbose=False, **kw), None
        except ValueError as e:
            out, err = None, str(e)
    return out, [str(w.message) for w in caught], err


def same_value(a, b):
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return type(a) is type(b) and a == b


def assert_same_result(dev, host, what):
    (d, d_warned, d_err), (h, h_warned, h_err) = dev, host
    assert d_err == h_err, (what, d_err, h_err)
    assert d_warned == h_warned, (what, d_warned, h_warned)
    if h is None:
        assert d is None, what
        return
    for key in ("kept_indices", "removed_indices"):
        assert np.array_equal(d[key], h[key]), (what, key)
    assert d["kept_names"] == h["kept_names"], what
    assert set(d["stats"]) == set(h["stats"]), (what, sorted(d["stats"]), sorted(h["stats"]))
    for key, want in h["stats"].items():
        assert same_value(d["stats"][key], want), (what, key, d["stats"][key], want)
    a, b = core._as_rmatrix(d["pruned_matrix"]).values, core._as_rmatrix(h["pruned_matrix"]).values
    assert a.shape == b.shape and (rh.same_bits(a, b) if a.dtype.kind == "f" else np.array_equal(a, b)), what


def on_handle(D, layout, cds=None, **kw):
    """prune_sparse_matrix(D, handle=a fresh handle of D in `layout`): run()'s triple, the child closed."""
    values = core.coded_matrix(D).values if cds is not None else D
    with _native.PreparedHandle(values, cds, layout=layout) as h:
        dev = run(D, handle=h, **kw)
    if dev[0] is not None:
        assert dev[0]["handle"].n == dev[0]["stats"]["final_size"]
        dev[0]["handle"].close()
    return dev


@functools.lru_cache(maxsize=None)
def random_case(n):
    D = pp.random_sparse(n, 6 if n > 10 else 4, 40 + n, symmetric=(n % 2 == 1))
    return D, run(D, min_connections=4, min_points=3)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", [10, 63, 64, 65, 129, 257])
def test_random_sparse_at_the_word_edges(n, layout):
    D, host = random_case(n)
    assert host[0] is not None and 0 < host[0]["stats"]["points_removed"] < n, "the case prunes something"
    assert_same_result(on_handle(D, layout, min_connections=4, min_points=3), host, (n, layout))


@functools.lru_cache(maxsize=None)
def cascade_case(max_iterations):
    D, _ = pp.shuffled(pp.clique_path(6, 200), 11)
    return D, run(D, min_connections=2, min_points=1, max_iterations=max_iterations)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_cascade_takes_a_round_per_path_point(layout):
    D, host = cascade_case(1000)
    assert host[0]["stats"]["iterations"] == 201 and host[0]["stats"]["final_size"] == 6 and host[1] == []
    assert_same_result(on_handle(D, layout, min_connections=2, min_points=1, max_iterations=1000), host, layout)
    D, host = cascade_case(100)                                    # the default max_iterations
    assert host[0]["stats"]["points_removed"] == 100 and host[0]["stats"]["iterations"] == 100
    assert host[1] == ["Reached max_iterations (100) before convergence"]
    assert_same_result(on_handle(D, layout, min_connections=2, min_points=1), host, layout)
    D, host = cascade_case(201)                                    # converges in the very round max_iterations names
    assert host[0]["stats"]["final_size"] == 6 and host[1] == ["Reached max_iterations (201) before convergence"]
    assert_same_result(on_handle(D, layout, min_connections=2, min_points=1, max_iterations=201), host, layout)
    D, host = cascade_case(0)
    assert_same_result(on_handle(D, layout, min_connections=2, min_points=1, max_iterations=0), host, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_min_points_stop_and_everything_removed(layout):
    D, _ = pp.shuffled(pp.clique_path(6, 5), 12)
    host = run(D, min_connections=2, min_points=9)
    assert host[0]["stats"]["final_size"] == 9 and host[1][0].startswith("Stopping at iteration 3: removing 1 points")
    assert_same_result(on_handle(D, layout, min_connections=2, min_points=9), host, layout)
    path = pp.empty(70)
    for a in range(69):
        pp.link(path, a, a + 1)
    host = run(path, min_connections=2, min_points=0)
    assert host[2] == "All points removed during pruning. Try lower min_connections."
    assert_same_result(on_handle(path, layout, min_connections=2, min_points=0), host, layout)
    host = run(path, min_connections=2, min_points=1)              # the last two would leave none: they stay
    assert host[0]["stats"]["final_size"] == 2 and host[1][0].startswith("Stopping at iteration 35: removing 2 points")
    assert_same_result(on_handle(path, layout, min_connections=2, min_points=1), host, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("lower", [False, True], ids=["upper", "lower"])
def test_cells_in_one_triangle_only_are_counted_along_rows(lower, layout):
    D = pp.upper_only(70)
    D = np.ascontiguousarray(D.T) if lower else D
    host = run(D, min_connections=2, min_points=2, ensure_connected=False)
    assert host[0]["stats"]["iterations"] == 35 and host[0]["stats"]["final_size"] == 2
    assert host[0]["kept_indices"].tolist() == ([68, 69] if lower else [0, 1])
    assert_same_result(on_handle(D, layout, min_connections=2, min_points=2, ensure_connected=False), host, (lower, layout))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_codes_and_infinities_count_as_measured(layout):
    rng = np.random.default_rng(13)
    D = pp.random_sparse(65, 6, 14)
    S = np.where(np.isnan(D), "NA", np.char.mod("%.6f", D)).astype(object)
    pick = ~np.isnan(D) & ~np.eye(65, dtype=bool)
    kind = rng.integers(0, 5, size=D.shape)
    S[pick & (kind == 1)] = "<40"
    S[pick & (kind == 2)] = ">1280"
    S[pick & (kind == 3)] = "Inf"
    m = core.coded_matrix(S)
    assert (m.codes != 0).sum() > 50 and np.isinf(m.values).sum() > 20
    host = run(S, min_connections=4, min_points=3)
    assert 0 < host[0]["stats"]["points_removed"] < 65
    assert_same_result(on_handle(S, layout, cds=m.codes, min_connections=4, min_points=3), host, layout)
    assert np.array_equal(host[0]["kept_indices"], run(D, min_connections=4, min_points=3)[0]["kept_indices"])


def test_a_handle_that_declined_its_ordering_serves():
    D = pp.random_sparse(129, 6, 15)
    a, b = np.argwhere(~np.isnan(D) & ~np.eye(129, dtype=bool))[0]
    D[a, b] = D[b, a] = -1.0
    host = run(D, min_connections=4, min_points=3)
    with _native.PreparedHandle(D) as h:
        assert h.declined
        dev = run(D, handle=h, min_connections=4, min_points=3)
        deg, cells = h.degrees()
    dev[0]["handle"].close()
    assert_same_result(dev, host, "declined")
    net = prune.analyze_network_structure(D)
    assert np.array_equal(deg, net["connectivity"]["degree"]) and cells == 2 * net["summary"]["n_measurements"]


@functools.lru_cache(maxsize=None)
def large_case():
    D = pp.random_sparse(3000, 14.5, 16)                            # just above where the 10-core of such a graph appears
    return D, run(D, min_connections=10, min_points=10)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_many_rounds_with_counts_that_cross_many_words(layout):
    D, host = large_case()
    s = host[0]["stats"]
    assert s["iterations"] >= 10 and 100 < s["final_size"] < 2900 and not any("Stopping" in w for w in host[1]), s
    assert_same_result(on_handle(D, layout, min_connections=10, min_points=10), host, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_target_completeness_search(layout):
    D, _ = pp.shuffled(pp.layered(), 17)
    host = run(D, target_completeness=0.5)
    assert host[0]["stats"]["min_connections_used"] == 8 and host[0]["stats"]["final_size"] == 12   # three attempts
    assert_same_result(on_handle(D, layout, target_completeness=0.5), host, (layout, "three attempts"))
    D, _ = pp.shuffled(pp.layered("circulant"), 18)
    host = run(D, target_completeness=0.9, min_points=12)
    assert host[1] == ["Reached min_points (12) before target completeness. Final completeness: 0.727, Target: 0.900"]
    assert_same_result(on_handle(D, layout, target_completeness=0.9, min_points=12), host, (layout, "min_points"))
    host = run(D, target_completeness=0.9, min_points=13)          # every attempt from the fourth on warns, then the error
    assert host[2] == "Could not reach target completeness after maximum attempts" and len(host[1]) == 8
    assert_same_result(on_handle(D, layout, target_completeness=0.9, min_points=13), host, (layout, "exhausted"))
    host = run(pp.regular(60, 20), target_completeness=0.9, min_points=0)
    assert host[2] == "All points removed during pruning. Try lower min_connections."
    assert_same_result(on_handle(pp.regular(60, 20), layout, target_completeness=0.9, min_points=0), host, (layout, "all"))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_degrees_equal_the_host_count(layout):
    for n in (65, 257):
        D = pp.random_sparse(n, 9, 19 + n, symmetric=False)
        D[1, 2] = np.inf
        adj = ~np.isnan(D) & ~np.eye(n, dtype=bool)
        with _native.PreparedHandle(D, layout=layout) as h:
            deg, cells = h.degrees()
            assert deg.dtype == np.int32 and np.array_equal(deg, adj.sum(axis=1)) and cells == adj.sum()
            assert not np.array_equal(deg, adj.sum(axis=0))
            net = prune.analyze_network_structure(D, handle=h)
            want = prune.analyze_network_structure(D)
            assert net["adjacency"] is None and net["summary"] == want["summary"]
            assert np.array_equal(net["connectivity"]["degree"], want["connectivity"]["degree"])
            assert rh.same_bits(net["connectivity"]["completeness"], want["connectivity"]["completeness"])
            if n == 257:
                sub = np.random.default_rng(20).permutation(257)[:100]
                sdeg, scells = h.degrees(sub)
                assert np.array_equal(sdeg, adj[np.ix_(sub, sub)].sum(axis=1)) and scells == sdeg.sum()
                with pytest.raises(_native.NativeError, match="repeated"):
                    h.degrees([5, 6, 5])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_child_equals_a_fresh_handle_and_the_parent_is_unchanged(layout):
    D = pp.random_sparse(257, 6, 21)
    names = ["s%03d" % q for q in range(257)]
    host = run(core.RMatrix(D, names), min_connections=4, min_points=3)
    with _native.PreparedHandle(D, layout=layout) as parent:
        before, graph_before = parent.fetch(), parent.connectivity()
        dev = run(core.RMatrix(D, names), handle=parent, min_connections=4, min_points=3)
        assert_same_result(dev, host, layout)
        assert dev[0]["kept_names"] == [names[q] for q in host[0]["kept_indices"]]
        skipped = run(D, handle=parent, min_connections=4, min_points=3, want_matrix=False)
        assert skipped[0]["pruned_matrix"] is None and np.array_equal(skipped[0]["kept_indices"], host[0]["kept_indices"])
        skipped[0]["handle"].close()
        after, graph_after = parent.fetch(), parent.connectivity()
        for name in FETCHED:
            x, y = getattr(before, name), getattr(after, name)
            assert (x is None and y is None) or rh.same_bits(x, y), name
        assert graph_before[:2] == graph_after[:2] and np.array_equal(graph_before[2], graph_after[2])
    pruned = host[0]["pruned_matrix"].values
    with dev[0]["handle"] as child, _native.PreparedHandle(np.ascontiguousarray(pruned), layout=layout,
                                                           preserve_order=True) as fresh:
        assert_same_handle(child, fresh, layout)                   # the child outlives its parent
        con = subsample.check_matrix_connectivity(pruned, 0.01, handle=child)
        assert con["is_connected"] == host[0]["stats"]["is_connected"]
        assert con["n_components"] == host[0]["stats"]["n_components"]
        assert con["n_measurements"] == host[0]["stats"]["final_measurements"]
