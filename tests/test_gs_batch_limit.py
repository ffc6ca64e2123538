"""Host-only: topolow_batch_problem_fits, the size test that routes a CV sweep between the one-workgroup exact-GS kernel
and the resident sessions (cv.likelihood_sweep) -- no GPU needed, the function is arithmetic on the kernel's LDS carve-up.

Limits found by bisection (largest n that fits, n_edges = 0), f64 / f32 per ndim:
  ndim   1     2     3     4     5     6     7     8     9     10    11-12  13-16
  f64    6814  5111  4088  3407  2920  2555  2271  2044  1858  1703  1460   1135
  f32    8176  6814  5840  5111  4543  4088  3716  3407  3144  2920  2555   2044
"""
import pytest

from tests import gs_forms as g
from topolow_amd import _native


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("ndim", g.GS_NDIMS)
def test_fits_is_monotone_and_ends_where_the_lds_does(ndim, precision):
    """True for every n from 2 to the limit, false for every n beyond it (gs_forms.batch_limit scans them all); the limit
    is where the kernel's carve-up, restated in gs_forms.lds_bytes, crosses 160 KB; a padded ndim shares the limit of the
    coordinate count it runs as."""
    limit = g.batch_limit(ndim, precision)
    print(f"batch_problem_fits limit: ndim {ndim} {precision} -> {limit}")
    rs = 4 if precision == "f32" else 8
    assert g.lds_bytes(limit, g.kernel_dim(ndim), rs) <= g.LDS_LIMIT < g.lds_bytes(limit + 1, g.kernel_dim(ndim), rs)
    assert limit == g.batch_limit(g.kernel_dim(ndim), precision)
    # an edge count never makes a problem that fits without one fail: the table form is taken only inside its own,
    # smaller budget, the dense form otherwise
    for n in sorted({2, 65, min(2048, limit), limit}):
        for n_edges in (1, 200, 65534, 65535, n * (n - 1) // 2):
            assert _native.batch_problem_fits(n, ndim, precision, n_edges), (n, n_edges)
    assert not _native.batch_problem_fits(limit + 1, ndim, precision, 200)


def test_f64_limit_at_ndim_5_is_the_documented_one():
    """include/topolow_relax.h, README.md, DESIGN.md, INTEGRATION.md and cv.likelihood_sweep say "about 2 900 points in
    f64 at ndim 5": the limit rounds to that at two significant digits.  The other figures worked out by hand from the
    carve-up -- about 4 540 in fp32 at ndim 5, about 1 135 in f64 at ndim 16 -- hold to 1 %."""
    assert 2850 <= g.batch_limit(5, "f64") < 2950
    assert abs(g.batch_limit(5, "f64") - 2920) <= 29
    assert abs(g.batch_limit(5, "f32") - 4540) <= 45
    assert abs(g.batch_limit(16, "f64") - 1135) <= 11


def test_fits_refuses_what_the_kernel_has_no_instance_for():
    assert not _native.batch_problem_fits(1, 5, "f64", 0)
    assert not _native.batch_problem_fits(100, 0, "f64", 0)
    assert not _native.batch_problem_fits(100, 17, "f64", 0)
    assert _native.batch_problem_fits(100, 16, "f64", 0)
