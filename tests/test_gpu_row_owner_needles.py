"""The row-owner stage kernels one launch at a time on needle problems (run with -m gpu): slab_stage_pipe_kernel in its 24
plain fp32 instances (ndim 1..10, 12, 16; with and without threshold targets), its f64 instance at every one of those
ndim, its ERR instances; slab_stage_exact_kernel; slab_stage_wide_kernel at 32 and 64 coordinates (and 17, zero-padded).
The problems, the band and the table of launches are tests/stage_needles.py; that the assertions made here see one lost,
doubled or misplaced pair, one swapped wave and one stray store is tests/test_stage_needles_host.py.

Every launch is the FIRST one from the start positions: Session.stage on caller buffers laid out as
sharded.HipBackend.new_positions lays them out, pos_out pre-filled with a bit pattern, against the f64 CPU model's stage of
the same column ranges (tests/models/slab_model.py) through stage_needles.hold: rows outside the block, padding and guard
rows keep the pattern bit for bit, idle rows equal the start bit for bit, every other row is within 1e-5 |move| +
2^-22 |p| (fp32) or 1e-12 of the largest move (f64) of the model.

Sizes: n = 2 W + 256 + 7 with W the widest chunk of the instance (PipeGeom in csrc/relax_kernels.h: fp32 1024 columns at
ndim 1-2, 768 at 3, 512 at 4-5, 256 from 6; f64 1024 at ndim 1, 512 at 2, 256 from 3) -- 2 311, 1 799, 1 287 or 775 points,
so that a one-stage slab can wrap with both parts longer than a chunk; 70 points (one ragged group); 5 points; 773 points
(n % 4 = 1).  Shapes per size: stage_needles.shapes."""
import numpy as np
import pytest

from tests import stage_needles as sn
from tests.test_gpu_symmetric import _Env
from topolow_amd import _native

pytestmark = pytest.mark.gpu

KINDS = ("spring", "repel")


def _session(nd, it, stages, precision, rows=None):
    """A session of the needle's block (or of `rows`) with the problem loaded and a run begun, so that Session.stage
    draws the slabs of PLAN_SEED."""
    c = nd.call
    rb, re = rows or (nd.row_begin, nd.row_end)
    with _Env(TOPOLOW_SYMMETRIC="0"):
        s = _native.Session(nd.n, nd.ndim, rb, re, precision=precision)
    s.load_dense(c.dissimilarity_matrix, c.threshold_matrix, c.degrees)
    if (rb, re) == (0, nd.n):
        s.set_edges(c.edge_i, c.edge_j, c.edge_dist, c.edge_thresh)
    else:       # the block's share of the list, by the parity rule of the sharded MAE (include/topolow_relax.h)
        own = np.where((c.edge_i + c.edge_j) % 2 == 0, np.minimum(c.edge_i, c.edge_j), np.maximum(c.edge_i, c.edge_j))
        m = (own >= rb) & (own < re)
        s.set_edges(c.edge_i[m], c.edge_j[m], c.edge_dist[m], c.edge_thresh[m])
    s.set_positions(c.initial_positions)
    s.begin(it + 1, nd.k, 0.01, nd.c_rep, 1e-12, 10 ** 9, 10 ** 6, sn.PLAN_SEED, stages)
    assert s.has_thresholds == bool(nd.flagged[rb:re].any())
    assert s.position_rows == (nd.n + 3) // 4 * 4
    assert int(s.lib.topolow_session_position_dim(s._h)) == sn.kernel_dim(nd.ndim)
    return s


def _one_stage(s, nd, it, slot, stages, precision, fused=False):
    """One launch on fresh caller buffers; returns pos_out (numpy) and with `fused` the (sum, count) it reduced."""
    import torch
    dtype = np.float32 if precision == "f32" else np.float64
    pos_in, pos_out = sn.launch_buffers(nd, dtype)
    d_in, d_out = torch.from_numpy(pos_in).cuda(), torch.from_numpy(pos_out).cuda()
    d_two = torch.zeros(2, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    if fused:
        s.stage_fused(d_in.data_ptr(), d_out.data_ptr(), it, nd.k, d_two.data_ptr())
    else:
        s.stage(d_in.data_ptr(), d_out.data_ptr(), it, slot, stages, nd.k)
    _, stopped, _ = s.sync()
    torch.cuda.synchronize()
    assert not stopped and s.first_nonfinite() == 0
    assert np.array_equal(d_in.cpu().numpy().view(np.uint8), pos_in.view(np.uint8))          # pos_in is read only
    return d_out.cpu().numpy(), d_two.cpu().numpy()


def _launch(launch, ndim, thresholded, kind, precision, wide=False):
    """A launch of the table; returns error / band."""
    exact = precision == "f64_exact"
    it, nd = sn.needle_of(launch, ndim, thresholded, kind, wide, exact)
    if launch.rows == sn.ONE_ROW:
        # a block of one row: every row of ONE_ROW by a session of its own, the rows put together for the band
        _, whole = sn.launch_buffers(nd, np.float32 if precision == "f32" else np.float64)
        pattern = sn.PATTERN[whole.dtype]
        for r in range(*launch.rows):
            s = _session(nd, it, launch.stages, precision, rows=(r, r + 1))
            out, _ = _one_stage(s, nd, it, launch.slot, launch.stages, precision)
            s.close()
            bits = out.view(pattern.dtype)
            assert (bits[:r] == pattern).all() and (bits[r + 1:] == pattern).all(), r
            whole[r] = out[r]
        return sn.hold(nd, whole, precision)
    s = _session(nd, it, launch.stages, precision)
    out, _ = _one_stage(s, nd, it, launch.slot, launch.stages, precision)
    s.close()
    return sn.hold(nd, out, precision, exact=exact)


def _launches(launches, ndim, thresholded, kind, precision, wide=False):
    worst = 0.0
    for launch in launches:
        ratio = _launch(launch, ndim, thresholded, kind, precision, wide)
        print("%s ndim %d thr %d %s n %d stages %d slot %d %s rows %s: error / band %.3f" %
              (precision, ndim, thresholded, kind, launch.n, launch.stages, launch.slot, launch.shape, launch.rows, ratio))
        worst = max(worst, ratio)
    print("%s ndim %d thr %d %s: largest error / band %.3f" % (precision, ndim, thresholded, kind, worst))
    return worst


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("thresholded", [False, True])
@pytest.mark.parametrize("ndim", sn.PLAIN_DIMS)
def test_fp32_instances_one_launch_against_the_model(ndim, thresholded, kind):
    """The 24 plain fp32 instances (CfgDim / CfgThr of launch_stage_pipe), two rows per wave in packed operations.  Per
    instance and kind: one stage of one wrapped with both parts longer than the widest chunk, with a 4-column second part,
    with a 4-column first part, not wrapped; every slot of a 3-stage iteration; a wrapped slot of a 16-stage iteration (a
    slab narrower than a group); 70 points; at ndim 3 five points; at ndim 7 the first three shapes at 773 points.
    Measured on an MI355X, the largest error / band per launch: spring 0.01 to 0.39 -- 0.393 at ndim 1, plain, not
    wrapped, on the row of a special column, whose four terms of 0.99 in all leave a move of 0.008; 0.15 or less from
    ndim 2 on -- and repel 0.07 to 0.25 (0.250: the rounding of the stored coordinate, a quarter of the band's
    2^-22 |p|); the model's own fp32 arithmetic gives 0.02 to 0.20 and 0.07 to 0.39 on the same problems."""
    _launches(sn.plain_launches("f32", ndim), ndim, thresholded, kind, "f32")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("thresholded", [False, True])
@pytest.mark.parametrize("ndim", sn.PLAIN_DIMS)
def test_f64_instance_one_launch_against_the_model(ndim, thresholded, kind):
    """The f64 instance at every instantiated ndim (4, 6, 7, 8 and 9 have no other stage-level comparison), the shapes of
    the fp32 test at its own chunk widths; band 1e-12 of the largest move.
    Measured on an MI355X, the largest error / band: spring 0.001, repel 0.178 (ndim 1, coordinates up to 2 300: the
    stored coordinate's rounding)."""
    _launches(sn.plain_launches("f64", ndim), ndim, thresholded, kind, "f64")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("thresholded", [False, True])
@pytest.mark.parametrize("ndim", sn.EXACT_DIMS)
def test_exact_instance_one_launch_against_the_model_on_unrounded_targets(ndim, thresholded, kind):
    """slab_stage_exact_kernel (precision f64_exact; it takes no row blocks): the model reads the targets as given, not as
    the words round them.  The shapes of the plain instances at the main size, 70 points, and at ndim 5 five points.
    Measured on an MI355X, the largest error / band: spring 0.020, repel 0.018."""
    _launches(sn.exact_launches(ndim), ndim, thresholded, kind, "f64_exact")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("thresholded", [False, True])
@pytest.mark.parametrize("ndim", sn.BLOCK_DIMS)
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_row_blocks_write_their_rows_and_nothing_else(precision, ndim, thresholded, kind):
    """Sessions of a row block: 259 rows from 259 (an odd count that starts and ends off a multiple of 8: the last wave
    works on a clamped copy of the last row), the last 261 rows, the first block again on a slot of a 3-stage iteration,
    and blocks of ONE row (twelve sessions, their rows held together).  Rows outside the block keep the pattern.
    Measured on an MI355X, the largest error / band: fp32 spring 0.158, repel 0.246 (one-row blocks 0.040 and 0.152);
    f64 spring 0.001, repel 0.012."""
    _launches(sn.block_launches(precision, ndim), ndim, thresholded, kind, precision)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("thresholded", [False, True])
@pytest.mark.parametrize("ndim", sn.WIDE_DIMS)
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_wide_instances_one_launch_against_the_model(precision, ndim, thresholded, kind):
    """slab_stage_wide_kernel at 32 and 64 coordinates, and 17 zero-padded to 32: 331 and 70 points, wrapped and not, 331
    with a 4-column part at either end, and a slot of a 3-stage iteration; a lane walks every 64th column, the planted columns are b, b + 63, b + 64, e - 1.
    Measured on an MI355X, the largest error / band: fp32 spring 0.083, repel 0.248; f64 spring 0.001, repel 0.004."""
    _launches(sn.wide_launches(), ndim, thresholded, kind, precision, wide=True)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("thresholded", [False, True])
@pytest.mark.parametrize("ndim", sn.ERR_DIMS)
def test_err_instances_write_the_plain_instances_positions(ndim, thresholded, kind):
    """The ERR instances (built for other wave budgets: kThrWavesE steps from 5 to 4 waves at ndim 5, kThrWaves at 7) on
    blocks of an even row count -- the main size and one point, wrapped with both parts longer than the widest chunk, with
    a 4-column second part, with a 4-column first part; 70 points --: Session.stage_fused writes positions bit-equal to Session.stage's, inside the band, and
    the count it reduces is exactly twice the number of spring pairs of the start positions.
    Measured on an MI355X, the largest error / band: spring 0.247 (ndim 2, 2 312 points), repel 0.248."""
    worst = 0.0
    for launch in sn.err_launches(ndim):
        it, nd = sn.needle_of(launch, ndim, thresholded, kind)
        s = _session(nd, it, 1, "f32")
        assert s.uses_dense_mae and s.can_fuse_checks
        plain, _ = _one_stage(s, nd, it, 0, 1, "f32")
        fused, two = _one_stage(s, nd, it, 0, 1, "f32", fused=True)
        s.close()
        assert np.array_equal(plain.view(np.uint32), fused.view(np.uint32)), \
            np.flatnonzero((plain.view(np.uint32) != fused.view(np.uint32)).any(axis=1))[:8]
        assert two[1] == 2 * sn.spring_pairs_at_start(nd), (two, sn.spring_pairs_at_start(nd))
        worst = max(worst, sn.hold(nd, fused, "f32"))
    print("ERR ndim %d thr %d %s: largest error / band %.3f" % (ndim, thresholded, kind, worst))
