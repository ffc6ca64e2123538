"""The subsampled route end to end on the device (run with -m gpu): subsample_dissimilarity_matrix(..., handle=parent)
against its host form under the same generator state, and cv.likelihood_sweep(path="resident", handle=child) against
the same sweep opening its own handle."""
import numpy as np
import pytest

from topolow_amd import _native, core, cv, subsample

pytestmark = pytest.mark.gpu

SEED = 5          # the first two draws of 150 hold a point of the small component, the third does not (asserted below)
FIELDS = ("selected_names", "is_connected", "n_components", "completeness", "attempt_number")


def planted():
    """400 points, symmetric, about half of the pairs measured: 396 points in one component, 4 measured among
    themselves only.  A draw of 150 is connected iff it misses all four (about one draw in seven)."""
    rng = np.random.default_rng(77)
    pts = rng.normal(size=(400, 3)) * 3.0
    D = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1))
    na = np.triu(rng.random((400, 400)) < 0.5, 1)
    D[na | na.T] = np.nan
    small = np.array([17, 130, 131, 388])
    D[small, :] = np.nan
    D[:, small] = np.nan
    D[np.ix_(small, small)] = 1.5
    np.fill_diagonal(D, 0.0)
    return core.RMatrix(D, ["s%03d" % q for q in range(400)])


def test_a_connected_draw_from_the_parent_equals_the_host_form():
    D = planted()
    whole = subsample.check_matrix_connectivity(D)
    assert whole["n_components"] == 2
    ra, rb = np.random.default_rng(SEED), np.random.default_rng(SEED)
    host = subsample.subsample_dissimilarity_matrix(D, 150, rng=ra)
    assert host["attempt_number"] == 3 and "handle" not in host
    with _native.PreparedHandle(D.values, preserve_order=True) as parent:
        assert subsample.check_matrix_connectivity(D, handle=parent) == whole
        dev = subsample.subsample_dissimilarity_matrix(D, 150, rng=rb, handle=parent)
    child = dev["handle"]
    try:
        assert ra.bit_generator.state == rb.bit_generator.state
        assert set(dev) == set(host) | {"handle"}
        for name in FIELDS:
            assert dev[name] == host[name], name
        assert dev["is_connected"] is True and dev["n_components"] == 1
        assert np.array_equal(dev["selected_indices"], host["selected_indices"])
        assert np.array_equal(dev["subsampled_matrix"].values, host["subsampled_matrix"].values, equal_nan=True)
        assert dev["subsampled_matrix"].names == host["subsampled_matrix"].names == dev["selected_names"]
        # the child is the handle of that very matrix, in the caller's labels, and outlives the parent
        assert child.n == 150 and child.info["order_route"] == _native.ORDER_PRESERVED and child.order is None
        assert child.connectivity()[0] == 1
        with _native.PreparedHandle(dev["subsampled_matrix"].values, preserve_order=True) as fresh:
            a, b = child.fetch(), fresh.fetch()
            for name in ("degrees", "edge_i", "edge_j", "edge_dist", "edge_thresh", "dense", "tdense"):
                assert np.array_equal(getattr(a, name), getattr(b, name)), name

        sets = [dict(N=2, k0=5.0, cooling_rate=0.02, c_repulsion=0.01), dict(N=3, k0=3.0, cooling_rate=0.02, c_repulsion=0.005)]
        r1, r2 = np.random.default_rng(4), np.random.default_rng(4)
        given = cv.likelihood_sweep(dev["subsampled_matrix"], sets, 30, 1e-4, folds=3, rng=r1, path="resident", handle=child)
        own = cv.likelihood_sweep(dev["subsampled_matrix"], sets, 30, 1e-4, folds=3, rng=r2, path="resident")
        assert given[0] == own[0] and given[2] == own[2] == 6 and given[3] == own[3]
        assert all(np.isfinite(x["Holdout_MAE"]) for x in given[0])
        assert r1.bit_generator.state == r2.bit_generator.state
        assert child.connectivity()[0] == 1                              # the sweep left the given handle open
    finally:
        child.close()


def test_the_whole_matrix_comes_back_with_a_copy_of_the_parent():
    D = planted()
    with _native.PreparedHandle(D.values, preserve_order=True) as parent:
        res = subsample.subsample_dissimilarity_matrix(D, 400, handle=parent)
        with res["handle"] as child:
            assert res["subsampled_matrix"] is D and res["n_components"] == 2 and not res["is_connected"]
            assert child.n == 400 and child.info == parent.info
            a, b = child.fetch(want_dense=False), parent.fetch(want_dense=False)
            assert np.array_equal(a.edge_dist, b.edge_dist) and np.array_equal(a.degrees, b.degrees)
