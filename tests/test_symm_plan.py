"""The host plans of the symmetric sweep (csrc/relax_symm_plan.h: relax_symm_plan, relax_symm_plan_rows, sym_rr_row,
sym_rr_above) through the host-only queries topolow_symm_plan and topolow_symm_stage_rows, which call the functions the
session calls: every plan against a brute-force enumeration of the tiles it must cover, and the plan shapes the GPU tests
of tests/test_gpu_symmetric_long_runs.py rely on.  No GPU."""
import functools

import numpy as np
import pytest

from topolow_amd import _native

SIZES = [33, 66, 200, 203, 520, 1000, 2050, 2973, 7205, 10000]
WAVES = [1, 4, 8, 12, 20, 68, 1024, 2048]


def _geometry(n):
    npad = (n + 63) // 64 * 64
    return npad // 64, npad // 32              # tile-rows of 64 points, column blocks of 32


@functools.lru_cache(maxsize=None)
def _triangle(n):
    """The upper triangle's tiles in tile-row-major order -- tile-row R holds the column blocks 2R .. TC - 1, its 64 x 64
    diagonal square included: (R of every tile, J of every tile); a tile's index in the tile-major copy is its place."""
    TR, TC = _geometry(n)
    R = np.concatenate([np.full(TC - 2 * r, r) for r in range(TR)])
    J = np.concatenate([np.arange(2 * r, TC) for r in range(TR)])
    return R, J


def _index_of(n, R, J):
    """Place of tile (R, J) in _triangle(n), by search (not by the library's closed form)."""
    TR, TC = _geometry(n)
    tR, tJ = _triangle(n)
    key = tR.astype(np.int64) * TC + tJ
    at = np.searchsorted(key, np.asarray(R, np.int64) * TC + np.asarray(J))
    assert np.array_equal(key[at], np.asarray(R, np.int64) * TC + np.asarray(J))
    return at


def _check_plan(n, n_waves, units, wave_first, want_index, t0):
    """units / wave_first cover exactly the tiles want_index (ascending places in the triangle), in order; returns the
    tiles of every wave's run."""
    TR, TC = _geometry(n)
    tR, tJ = _triangle(n)
    R, j0, j1, tile0 = (units[:, q].astype(np.int64) for q in range(4))
    length = j1 - j0
    assert np.all((2 * R <= j0) & (j0 < j1) & (j1 <= TC)) and np.all((0 <= R) & (R < TR))    # one tile-row, a real interval
    # every tile of the set exactly once, no other, tile-row-major
    first = np.cumsum(length) - length
    uR = np.repeat(R, length)
    uJ = np.repeat(j0 - first, length) + np.arange(int(length.sum()))
    assert uR.shape == want_index.shape
    assert np.array_equal(uR, tR[want_index]) and np.array_equal(uJ, tJ[want_index])
    assert np.array_equal(tile0, _index_of(n, R, j0) - t0)
    assert np.all(np.diff(R) >= 0)
    # runs
    assert wave_first.shape == (n_waves + 1,) and wave_first[0] == 0 and wave_first[-1] == len(units)
    assert np.all(np.diff(wave_first) >= 0)
    done = np.concatenate([[0], np.cumsum(length)])
    per_wave = np.diff(done[wave_first])
    busy = per_wave[per_wave > 0]
    if len(busy):
        assert busy.max() - busy.min() <= 1, (n, n_waves, busy.min(), busy.max())
    if len(want_index) >= n_waves:
        assert len(busy) == n_waves, (n, n_waves)
    return per_wave


def _stage_tiles(n, S, st):
    """Places in the triangle of the tiles stage st of an S-stage iteration sweeps, from the per-row intervals."""
    rows = _native.symm_stage_rows(n, S, st)
    R = np.concatenate([np.full(max(0, int(r[1] - r[0])), q) for q, r in enumerate(rows)] + [np.zeros(0, int)])
    J = np.concatenate([np.arange(int(r[0]), max(int(r[0]), int(r[1]))) for r in rows] + [np.zeros(0, int)])
    assert np.all(J >= 2 * R)
    return _index_of(n, R, J)


@pytest.mark.parametrize("n", SIZES)
def test_whole_triangle_and_segment_plans_cover_their_tiles_once(n):
    TR, TC = _geometry(n)
    total = TR * (TR + 1)
    assert len(_triangle(n)[0]) == total
    for n_waves in WAVES:
        units, wave_first = _native.symm_plan(n, n_waves)
        _check_plan(n, n_waves, units, wave_first, np.arange(total), 0)
        for P in (2, 3, 4):
            covered = []
            for b in range(P):
                t0, t1 = total * b // P, total * (b + 1) // P
                units, wave_first = _native.symm_plan(n, n_waves, segment=b, n_segments=P)
                _check_plan(n, n_waves, units, wave_first, np.arange(t0, t1), t0)
                covered.append(np.arange(t0, t1))
            assert np.array_equal(np.concatenate(covered), np.arange(total))      # the segments tile the triangle in order


@pytest.mark.parametrize("S", [2, 4, 8])
@pytest.mark.parametrize("n", SIZES)
def test_stage_plans_split_the_triangle_and_the_apply_sums_the_right_tile_rows(n, S):
    TR, TC = _geometry(n)
    if TR < 2 * S:
        assert _native.symm_stage_rows(n, S, 0) is None and _native.symm_stage_bounds(n, S) is None
        with pytest.raises(ValueError):
            _native.symm_plan(n, 4, stages=S, stage=0)
        return
    total = TR * (TR + 1)
    sets = [_stage_tiles(n, S, st) for st in range(S)]
    assert np.array_equal(np.sort(np.concatenate(sets)), np.arange(total))        # disjoint, and together the triangle
    for st in range(S):
        assert np.all(np.diff(sets[st]) > 0)
        for n_waves in WAVES:
            units, wave_first = _native.symm_plan(n, n_waves, stages=S, stage=st)
            _check_plan(n, n_waves, units, wave_first, sets[st], 0)
        # sym_rr_above against sym_rr_row: the tile-rows whose column sums of this stage belong to the points of
        # tile-row R are those STRICTLY above R whose interval of the stage holds R's two column blocks
        rows = _native.symm_stage_rows(n, S, st)
        j0, j1, rp0, rp1 = (rows[:, q].astype(int) for q in range(4))
        for R in range(TR):
            holds = [(j0[Rp] <= 2 * R and 2 * R < j1[Rp], j0[Rp] <= 2 * R + 1 and 2 * R + 1 < j1[Rp]) for Rp in range(R)]
            assert all(a == b for a, b in holds)                                    # never half of a diagonal square
            named = list(range(rp0[R], rp1[R])) if rp1[R] > rp0[R] else []
            assert named == [Rp for Rp in range(R) if holds[Rp][0]], (n, S, st, R)


def _shape(n, n_waves, **kw):
    units, wave_first = _native.symm_plan(n, n_waves, **kw)
    length = (units[:, 2] - units[:, 1]).astype(int)
    done = np.concatenate([[0], np.cumsum(length)])
    return dict(units=len(units), run_tiles=np.diff(done[wave_first]), run_units=np.diff(wave_first),
                longest=int(length.max()) if len(length) else 0)


def test_the_plan_shapes_the_capped_grid_tests_are_built_on():
    """TOPOLOW_SYMMETRIC_GRID = g gives 4 g waves: 200 points on one workgroup and 1 000 on one or three give every wave
    a run of several units of several tiles -- the shape of a resident grid on a production-size problem -- while a
    resident grid (2 048 waves at two per SIMD) on anything up to 2 050 points gives one tile per unit."""
    a = _shape(200, 4)
    assert a["units"] == 7 and set(a["run_tiles"]) == {5} and a["longest"] == 5
    b = _shape(1000, 4)
    assert b["units"] == 19 and set(b["run_tiles"]) == {68} and b["run_units"].max() == 8 and b["longest"] == 32
    c = _shape(1000, 12)
    assert c["units"] == 26 and set(c["run_tiles"]) == {22, 23} and c["longest"] == 23
    for n in (33, 66, 200, 203, 520, 1000, 2050):
        d = _shape(n, 2048)
        assert d["longest"] == 1 and d["run_tiles"].max() == 1


def test_segment_row_windows_are_the_tile_rows_of_the_segments_tiles():
    """topolow_symm_segment_rows (the rows a caller brings together before topolow_session_symm_segment_build): rows
    [64 r_first, min(n, 64 (r_last + 1))) of the tile-rows that hold the segment's tiles -- from the segment's units, and
    from the brute-force tile list.  385 points are 7 tile-rows, 56 tiles: seven segments of eight tiles (the fewest a
    segment may have), none for eight segments."""
    for n in (385, 520, 1000):
        TR, _ = _geometry(n)
        total = TR * (TR + 1)
        tR, _ = _triangle(n)
        for P in (2, 3, 5, 7):
            for b in range(P):
                units, _ = _native.symm_plan(n, 4, segment=b, n_segments=P)
                r_first, r_last = int(units[:, 0].min()), int(units[:, 0].max())
                mine = tR[total * b // P:total * (b + 1) // P]
                assert (r_first, r_last) == (mine.min(), mine.max())
                assert _native.symm_segment_rows(n, b, P) == (64 * r_first, min(n, 64 * (r_last + 1))), (n, P, b)
    assert [_native.symm_segment_rows(385, r, 7) for r in range(7)] == [
        (0, 64), (0, 128), (64, 128), (64, 192), (128, 256), (192, 320), (256, 385)]
    assert _native.symm_segment_rows(385, 0, 8) is None
    assert _native.symm_segment_rows(385, 7, 7) is None and _native.symm_segment_rows(1, 0, 1) is None


def test_plan_queries_refuse_what_no_session_plans_with():
    lib = _native.load()
    assert lib.topolow_symm_plan(1, 4, 0, 0, 0, 1, None, 0, None) == -1          # no pair
    assert lib.topolow_symm_plan(1000, 0, 0, 0, 0, 1, None, 0, None) == -1       # no wave
    assert lib.topolow_symm_plan(1000, 4, 3, 0, 0, 1, None, 0, None) == -1       # stages: 2, 4, 8
    assert lib.topolow_symm_plan(1000, 4, 2, 2, 0, 1, None, 0, None) == -1       # stage < stages
    assert lib.topolow_symm_plan(1000, 4, 0, 0, 3, 3, None, 0, None) == -1       # segment < n_segments
    assert lib.topolow_symm_plan(1000, 4, 2, 0, 0, 2, None, 0, None) == -1       # a sharded run has no stage plans
    assert lib.topolow_symm_plan(1000, 4, 0, 0, 0, 1, None, 0, None) == 19       # null outputs: the count alone
    assert lib.topolow_symm_stage_rows(1000, 8, 8, None) == -1 and lib.topolow_symm_stage_rows(1000, 8, 7, None) == 16
