"""Sub-handles gathered on the device (run with -m gpu): PreparedHandle.subsample(indices) against a fresh
PreparedHandle of the host-gathered submatrix -- info, the route, and every fetch() output, bit for bit -- and the
resident entries on a child against the same entries on the fresh handle (topolow_layout_prep_subsample)."""
import numpy as np
import pytest

from tests import resident_helpers as rh
from topolow_amd import _native, subsample

pytestmark = pytest.mark.gpu

FETCHED = ("order", "degrees", "edge_i", "edge_j", "edge_dist", "edge_thresh", "dense", "tdense", "values_reordered",
           "codes_reordered")


def matrix(n, form, codes, seed=0):
    """Symmetric distances of random points, 40 % NA, the diagonal 0.  form "exact": every value k * 2^-10 (route 1);
    "generic": doubles as they come (route 2); "duplicates": generic with points 3 and 4 made copies of point 2."""
    rng = np.random.default_rng(100 * n + seed)
    pts = rng.normal(size=(n, 3)) * 3.0
    if form == "duplicates":
        pts[3] = pts[4] = pts[2]
    D = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1))
    if form == "exact":
        D = np.round(D * 1024.0) / 1024.0
    na = np.triu(rng.random((n, n)) < 0.4, 1)
    if form == "duplicates":
        na[:5, :] = False
        na[:, :5] = False
    D[na | na.T] = np.nan
    cds = None
    if codes:
        u = np.triu(rng.random((n, n)), 1)
        u = u + u.T
        cds = np.zeros((n, n), dtype=np.int8)
        cds[(u > 0) & (u < 0.10)] = 1
        cds[(u >= 0.10) & (u < 0.15)] = -1
    return D, cds


def gathered(D, cds, idx):
    ix = np.ix_(idx, idx)
    return np.ascontiguousarray(D[ix]), (np.ascontiguousarray(cds[ix]) if cds is not None else None)


def same_info(a, b):
    return all(rh.same_bits(np.asarray(a[k]), np.asarray(b[k])) for k in set(a) | set(b))


def assert_same_handle(child, fresh, what):
    assert same_info(child.info, fresh.info), (what, child.info, fresh.info)
    assert child.declined == fresh.declined and (child.n, child.layout, child.has_codes) == \
        (fresh.n, fresh.layout, fresh.has_codes), what
    assert (child.order is None) == (fresh.order is None), what
    assert child.order is None or np.array_equal(child.order, fresh.order), what
    a, b = child.fetch(), fresh.fetch()
    for name in FETCHED:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), (what, name)
        assert x is None or rh.same_bits(x, y), (what, name)
        if x is not None and x.ndim == 2:
            assert x.flags.c_contiguous == y.flags.c_contiguous, (what, name)
    return a


def both(D, cds, idx, layout, what, **kw):
    """Child of a parent of D against a fresh handle of D[idx, idx]; returns the route."""
    sub, subc = gathered(D, cds, np.arange(D.shape[0]) if idx is None else idx)
    with _native.PreparedHandle(D, cds, layout=layout) as parent:
        fetched = None if parent.declined else parent.fetch()
        child_kw = dict(preserve_order=kw.get("preserve_order", False), order_in=kw.get("order"))
        with parent.subsample(idx, **child_kw) as child, _native.PreparedHandle(sub, subc, layout=layout, **kw) as fresh:
            assert_same_handle(child, fresh, what)
            route = child.info["order_route"]
        if fetched is not None:                      # the parent is as it was
            again = parent.fetch()
            for name in FETCHED:
                x, y = getattr(fetched, name), getattr(again, name)
                assert (x is None and y is None) or rh.same_bits(x, y), (what, name)
    return route


@pytest.mark.parametrize("layout", ["C", "F"])
@pytest.mark.parametrize("codes", [False, True], ids=["plain", "codes"])
@pytest.mark.parametrize("form,route", [("exact", _native.ORDER_DEVICE_EXACT), ("generic", _native.ORDER_DEVICE_GAP)])
def test_child_equals_fresh_handle_of_the_gathered_submatrix(form, route, codes, layout):
    D, cds = matrix(300, form, codes)
    rng = np.random.default_rng(3)
    idx = rng.permutation(300)[:100]
    assert not np.array_equal(idx, np.sort(idx))
    assert both(D, cds, idx, layout, (form, codes, layout, 100)) == route
    both(D, cds, idx[:2], layout, (form, codes, layout, 2))                       # m = 2: whatever the route
    assert both(D, cds, np.arange(300), layout, (form, codes, layout, "identity")) == route
    assert both(D, cds, None, layout, (form, codes, layout, "NULL")) == route


@pytest.mark.parametrize("layout", ["C", "F"])
def test_more_than_one_tile_row_and_a_ragged_last_tile(layout):
    D, cds = matrix(1300, "generic", True)
    idx = np.random.default_rng(4).permutation(1300)[:1100]
    assert both(D, cds, idx, layout, (layout, 1100)) == _native.ORDER_DEVICE_GAP


@pytest.mark.parametrize("layout", ["C", "F"])
def test_duplicated_points_report_the_same_route_whichever_it_is(layout):
    D, cds = matrix(300, "duplicates", False)
    idx = np.concatenate([[4, 2, 3], np.random.default_rng(5).permutation(np.arange(5, 300))[:97]])
    both(D, cds, idx, layout, ("duplicates", layout))


@pytest.mark.parametrize("layout", ["C", "F"])
def test_preserve_order_and_order_in(layout):
    D, cds = matrix(300, "generic", True)
    rng = np.random.default_rng(6)
    idx = rng.permutation(300)[:100]
    assert both(D, cds, idx, layout, "preserve", preserve_order=True) == _native.ORDER_PRESERVED
    assert both(D, cds, idx, layout, "order_in", order=rng.permutation(100).astype(np.int32)) == _native.ORDER_DECLINED
    assert both(D, cds, idx, layout, "keep", order=np.array([-1], dtype=np.int32)) == _native.ORDER_DECLINED
    with _native.PreparedHandle(D, cds, layout=layout) as parent:
        with pytest.raises(_native.NativeError, match="permutation"):
            parent.subsample(idx, order_in=np.zeros(100, dtype=np.int32))
        with pytest.raises(_native.NativeError, match="repeated"):
            parent.subsample([5, 6, 5])


def test_a_declined_parent_still_has_children():
    D, cds = matrix(300, "generic", False)
    D[7, 9] = D[9, 7] = -1.0
    idx = np.random.default_rng(7).permutation(300)[:100]
    idx = idx[(idx != 7) & (idx != 9)]                # the child holds no negative cell: it orders itself
    with _native.PreparedHandle(D) as parent:
        assert parent.declined
    assert both(D, cds, idx, "C", "declined parent") == _native.ORDER_DEVICE_GAP
    with_negative = np.concatenate([idx[:50], [9, 7]])
    assert both(D, cds, with_negative, "C", "declined child") == _native.ORDER_DECLINED


def test_a_child_of_a_child_and_its_graph():
    D, cds = matrix(300, "generic", True)
    rng = np.random.default_rng(8)
    first, second = rng.permutation(300)[:150], rng.permutation(150)[:60]
    sub, subc = gathered(D, cds, first[second])
    with _native.PreparedHandle(D, cds) as parent:
        with parent.subsample(first) as child:
            grandchild = child.subsample(second)
    with grandchild, _native.PreparedHandle(sub, subc) as fresh:       # parent and child are closed by now
        assert_same_handle(grandchild, fresh, "grandchild")
        pick = rng.permutation(60)[:25]
        nc, cells, labels = grandchild.connectivity(pick)
        want, want_cells = subsample.component_labels(sub[np.ix_(pick, pick)])
        assert np.array_equal(labels, want) and cells == want_cells and nc == np.sum(want == np.arange(25))


RUN_KW = dict(n_iter=20, k0=5.0, cooling_rate=0.01, c_repulsion=0.01, relative_epsilon=1e-4, convergence_window=5,
              convergence_check_freq=3)


@pytest.mark.parametrize("n,m,schedule", [(300, 200, "gs"), (1300, 1100, "slab")], ids=["one-workgroup", "slab"])
def test_optimize_and_post_metrics_on_a_child_equal_those_on_the_fresh_handle(n, m, schedule):
    D, cds = matrix(n, "generic", True)
    idx = np.random.default_rng(9).permutation(n)[:m]
    sub, subc = gathered(D, cds, idx)
    init = rh.start_positions(m, 5, m)
    with _native.PreparedHandle(D, cds) as parent:
        child = parent.subsample(idx)
    with child, _native.PreparedHandle(sub, subc) as fresh:             # the child works after its parent is closed
        got, want = child.optimize(init, 5, seed=9, **RUN_KW), fresh.optimize(init, 5, seed=9, **RUN_KW)
        assert got.info["schedule"] == want.info["schedule"] == schedule
        assert rh.same_bits(got.positions, want.positions)
        assert (got.converged, got.iterations) == (want.converged, want.iterations)
        assert rh.same_bits(np.float64(got.final_mae), np.float64(want.final_mae))
        assert rh.same_bits(np.float64(got.final_k), np.float64(want.final_k))
        (ea, sa, ca), (eb, sb, cb) = child.post_metrics(got.positions), fresh.post_metrics(want.positions)
        assert rh.same_bits(ea, eb) and rh.same_bits(np.float64(sa), np.float64(sb)) and ca == cb and ca > 0
        assert_same_handle(child, fresh, "after the runs")
