"""Sparse "needle" problems for the convergence check (host only: numpy and the CPU oracle, no GPU code).

The check's kernels (csrc/relax_kernels.h: dense_error_kernel in upper-triangle and PARITY form, edge_error_kernel, the ERR
instances of slab_stage_pipe_kernel) are held to oracle.edge_error pair by pair: about n measured pairs among n points, so
that one lost, doubled or misplaced pair changes the count by one and the sum by 0.9 at the least.  No n x n array is built
anywhere here: the large cases (8 200 points, 4.5 million listed pairs) depend on that.

Codes are the oracle's: 0 exact, 1 ">" (counts where r < t), -1 "<" (counts where r > t)."""
import collections
import functools

import numpy as np

from oracle import topolow_oracle as orc

CHUNK, GROUP, TILE_ROWS, WAVE_ROWS = 1024, 256, 64, 8          # ErrCfg = StageCfg<256, 2, 1024>, kErrTileRows

Needle = collections.namedtuple(
    "Needle", "n dim pos edge_i edge_j edge_dist edge_dist_dev edge_thresh degrees ties planted classes")


def round4(t):
    """The 4-ulp fp32 word a session stores for a target (tests/test_gpu_parity.py: _decode_rounded), as f64."""
    u = np.asarray(t, dtype=np.float64).astype(np.float32).view(np.uint32)
    mag = ((u & np.uint32(0x7FFFFFFF)) + np.uint32(2)) & np.uint32(0xFFFFFFFC)
    return ((u & np.uint32(0x80000000)) | mag).view(np.float32).astype(np.float64)


def _take(seq, k, start):
    seq = list(seq)
    return [seq[(start + q) % len(seq)] for q in range(min(k, len(seq)))]


def seam_cells(n, row_blocks=None):
    """{seam class: [(i, j), ...]} with i < j < n: the cells on the seams of dense_error_kernel.  row_blocks: the
    (row_begin, row_end) blocks the problem is also run as (their last rows are seams too)."""
    blocks = list(row_blocks) if row_blocks else [(0, n)]
    out = collections.OrderedDict()

    def add(name, cells):
        got = sorted({(int(i), int(j)) for i, j in cells if 0 <= i < j < n})
        if got:
            out[name] = got

    # columns: around every 256-column group base (1 024-multiples are chunk bases), and the last two real columns
    col_seams = collections.OrderedDict()
    for b in range(0, n + GROUP, GROUP):
        kind = "chunk" if b % CHUNK == 0 else "group"
        for off, tag in ((-1, "b-1"), (0, "b"), (3, "b+3"), (4, "b+4"), (255, "b+255")):
            if 0 < b + off < n:
                col_seams.setdefault("col %s %s" % (kind, tag), []).append(b + off)
    col_seams["col n-2"] = [n - 2] if n >= 3 else []
    col_seams["col n-1"] = [n - 1]
    all_cols = sorted({c for v in col_seams.values() for c in v})
    # rows: tile, wave and row-pair seams, the last rows of every block
    row_seams = collections.OrderedDict()
    row_seams["row 64q-1"] = [64 * q - 1 for q in range(1, n // TILE_ROWS + 2)]
    row_seams["row 64q"] = [64 * q for q in range(0, n // TILE_ROWS + 1)]
    waves = sorted({0, 1, 7, (CHUNK // 8) - 1, CHUNK // 8, (2 * CHUNK) // 8 - 1, (2 * CHUNK) // 8, max(0, (n - 9) // 8)})
    row_seams["row 8q+7"] = [8 * q + 7 for q in waves]
    row_seams["row 8q+8"] = [8 * q + 8 for q in waves]
    pairs = sorted({1, 16, 255, 511, 512, 600, max(0, (n - 5) // 2)})
    row_seams["row 2q"] = [2 * q for q in pairs]
    row_seams["row 2q+1"] = [2 * q + 1 for q in pairs]
    row_seams["row block last"] = [re_ - 1 for _, re_ in blocks]
    row_seams["row block last-1"] = [re_ - 2 for _, re_ in blocks]
    all_rows = sorted({r for v in row_seams.values() for r in v if 0 <= r < n - 1})

    for name, cols in col_seams.items():                     # every seam column under three seam rows above it
        cells = []
        for q, c in enumerate(cols):
            above = [r for r in all_rows if r < c]
            cells += [(r, c) for r in _take(above, 3, 7 * q + len(name))]
            if not above:
                cells += [(i, c) for i in range(max(0, c - 2), c)]
        add(name, cells)
    for name, rows in row_seams.items():                     # every seam row against the next two seam columns and a far one
        cells = []
        for q, r in enumerate(rows):
            right = [c for c in all_cols if c > r]
            cells += [(r, c) for c in right[:2]]
            cells += [(r, c) for c in _take(right, 1, 5 * q + len(name))]
            if not right and r + 1 < n:
                cells.append((r, r + 1))
        add(name, cells)
    # near the diagonal: i = 0, 1, 2, 3 mod 4, and around every chunk base
    add("diag i mod 4", [(i, i + d) for i in (4, 5, 6, 7, 0, 1, 2, 3) for d in (1, 2, 3, 4)])
    for cb in range(CHUNK, n, CHUNK):
        add("diag chunk %d" % cb, [(i, i + d) for i in range(cb - 3, cb + 4) for d in (1, 2, 3, 4)])
        # the last row pair on the packed fast path (row0 + 1 == cb - 1) and the first one inside the chunk (row0 == cb)
        add("fast-path edge %d" % cb, [(i, cb + d) for i in (cb - 2, cb - 1) for d in range(5)])
        add("first pair inside %d" % cb, [(i, cb + d) for i in (cb, cb + 1) for d in range(5)])
    return out


def _tie_points(n):
    """Three pairs of points (i < j), all six distinct, spread over the rows."""
    if n < 16:
        return []
    return [(n // 3, n // 3 + 7), (3, n // 2 + 1), (n // 2, n - 5)]


def _targets(rng, r, thresholded):
    """t = r +- e with e in [0.9, 1.1] or [3.6, 4.4]; r - e only where r > e + 0.5; codes 1/2, 1/4, 1/4."""
    m = r.shape[0]
    e = np.where(rng.random(m) < 0.5, rng.uniform(0.9, 1.1, m), rng.uniform(3.6, 4.4, m))
    minus = (rng.random(m) < 0.5) & (r > e + 0.5)
    t = np.where(minus, r - e, r + e)
    code = (rng.choice([0, 1, -1], size=m, p=[0.5, 0.25, 0.25]) if thresholded else np.zeros(m)).astype(np.int32)
    return t, code


def pair_terms(pos, ei, ej, t, code):
    """Per listed pair, in f64: (contributes, |t - r|, max(r, t))."""
    d = pos[ei] - pos[ej]
    r = np.sqrt((d * d).sum(-1))
    contributes = (code == 0) | ((code == 1) & (r < t)) | ((code == -1) & (r > t))
    return contributes, np.abs(t - r), np.maximum(r, t)


def sum_band_f32(pos, ei, ej, t, code, kernel_dim):
    """The fp32 passes' band on the sum: every contributing pair's |t - r| comes through kernel_dim + 6 roundings of
    2^-24 relative to max(r, t) at the most -- the subtractions dx (one per coordinate, relative to the coordinates, whose
    differences make up r), the fma chain (kernel_dim, folded with the dx), sqrt, t - r, the fp32 running sum and its fold
    into f64."""
    contributes, _, big = pair_terms(pos, ei, ej, t, code)
    return float((kernel_dim + 6) * 2.0 ** -24 * big[contributes].sum())


def oracle(pos, nd, which="dev", mask=None):
    """oracle.edge_error of `pos` on the needle's list: which = "dev" (targets as the device rounds them) or "raw"."""
    t = nd.edge_dist_dev if which == "dev" else nd.edge_dist
    m = slice(None) if mask is None else mask
    return orc.edge_error(pos, nd.edge_i[m], nd.edge_j[m], t[m], nd.edge_thresh[m])


def one_pair_margin(pos, ei, ej, t, code, kernel_dim):
    """The smallest move of sum / count when one contributing pair is dropped or counted twice, over the fp32 band of the
    ratio (sum_band_f32 / count)."""
    contributes, err, _ = pair_terms(pos, ei, ej, t, code)
    e = err[contributes]
    K, S = e.shape[0], e.sum()
    if K < 2:
        return np.inf
    drop = np.abs((S - e) / (K - 1) - S / K)
    twice = np.abs((S + e) / (K + 1) - S / K)
    band = sum_band_f32(pos, ei, ej, t, code, kernel_dim) / K
    return float(min(drop.min(), twice.min()) / band)


@functools.lru_cache(maxsize=None)
def check_needle(n, dim, seed, thresholded, cells=(), row_blocks=None, margin=100.0):
    """Positions 3 N(0, 1) rounded to fp32; every unordered pair measured with probability 2 / n plus the planted `cells`
    (default: all of seam_cells(n, row_blocks)); targets and codes by _targets; three tie pairs (distance and target exactly
    5.0, codes 0, ">" and "<"; all 0 in a problem without thresholds, which must hold no code at all) on six points with integer coordinates where n >= 16.  margin: one_pair_margin at the start
    is asserted to be at least this (None: not asserted -- cases that hold the count itself)."""
    rng = np.random.default_rng([n, dim, seed, int(thresholded)])
    pos = (3.0 * rng.standard_normal((n, dim))).astype(np.float32).astype(np.float64)
    ties = _tie_points(n)
    for k, (a, b) in enumerate(ties):
        pos[a] = 0.0
        pos[b] = 0.0
        pos[a, 0], pos[b, 0] = 10.0 * k, 10.0 * k + (3.0 if dim >= 2 else 5.0)
        if dim >= 2:
            pos[b, 1] = 4.0
    classes = seam_cells(n, row_blocks)
    planted = sorted({c for v in classes.values() for c in v}) if cells == () else sorted(set(cells))
    draws = int(rng.binomial(n * n, min(1.0, 2.0 / n)))
    a, b = rng.integers(0, n, size=(2, draws))
    keep = a < b
    key = np.concatenate([a[keep] * n + b[keep], np.array([i * n + j for i, j in planted], dtype=np.int64)])
    tie_keys = np.array([i * n + j for i, j in ties], dtype=np.int64)
    key = np.setdiff1d(np.unique(key), tie_keys)
    key = key[np.lexsort((key // n, key % n))]               # column-major, as core.prepare_layout_call lists the edges
    ei, ej = (key // n).astype(np.int32), (key % n).astype(np.int32)
    d = pos[ei] - pos[ej]
    t, code = _targets(rng, np.sqrt((d * d).sum(-1)), thresholded)
    if ties:
        ei = np.concatenate([ei, np.array([i for i, _ in ties], dtype=np.int32)])
        ej = np.concatenate([ej, np.array([j for _, j in ties], dtype=np.int32)])
        t = np.concatenate([t, np.full(len(ties), 5.0)])
        code = np.concatenate([code, np.array([0, 1, -1] if thresholded else [0, 0, 0], dtype=np.int32)])
    t_dev = round4(t)
    assert np.array_equal(t_dev[len(t) - len(ties):], np.full(len(ties), 5.0))
    degrees = (1 + np.bincount(ei, minlength=n) + np.bincount(ej, minlength=n)).astype(np.int32)
    tie_idx = np.arange(len(t) - len(ties), len(t))
    nd = Needle(n, dim, pos, ei, ej, t, t_dev, code, degrees, tie_idx, tuple(planted), classes)
    # margins of 0.9 at the least: fp32 and f64 never classify a pair differently
    c, err, _ = pair_terms(pos, ei, ej, t_dev, code)
    off = np.ones(len(t), dtype=bool)
    off[tie_idx] = False
    assert err[off].min() > 0.89 and np.array_equal(err[tie_idx], np.zeros(len(ties)))
    if margin is not None:
        got = one_pair_margin(pos, ei, ej, t_dev, code, kernel_dim(dim))
        assert got >= margin, (n, dim, seed, thresholded, got)
    for arr in (pos, ei, ej, t, t_dev, code, degrees):
        arr.setflags(write=False)
    return nd


def kernel_dim(ndim):
    """The coordinates a session computes with (zero-padded): csrc/topolow_session.h, kernel_dim."""
    return ndim if ndim <= 10 else (12 if ndim <= 12 else 16)


@functools.lru_cache(maxsize=2)
def full_list(n, dim, seed, thresholded):
    """Every unordered pair listed (n (n - 1) / 2 edges, column-major), targets by the needle's rule; no ties."""
    rng = np.random.default_rng([n, dim, seed, int(thresholded), 1])
    pos = (3.0 * rng.standard_normal((n, dim))).astype(np.float32).astype(np.float64)
    ej = np.repeat(np.arange(n, dtype=np.int32), np.arange(n))
    ei = (np.arange(ej.shape[0], dtype=np.int64) - (ej.astype(np.int64) * (ej - 1)) // 2).astype(np.int32)
    assert ei.min() == 0 and (ei < ej).all()
    d = pos[ei] - pos[ej]
    t, code = _targets(rng, np.sqrt((d * d).sum(-1)), thresholded)
    t_dev = round4(t)
    degrees = np.full(n, n, dtype=np.int32)
    nd = Needle(n, dim, pos, ei, ej, t, t_dev, code, degrees, np.zeros(0, dtype=np.int64), (), {})
    for arr in (pos, ei, ej, t, t_dev, code, degrees):
        arr.setflags(write=False)
    return nd


def parity_share(nd, row_begin, row_end):
    """Mask of the listed pairs a row block reduces: the parity rule of the sharded MAE (include/topolow_relax.h)."""
    lo, hi = np.minimum(nd.edge_i, nd.edge_j), np.maximum(nd.edge_i, nd.edge_j)
    own = np.where((lo + hi) % 2 == 0, lo, hi)
    return (own >= row_begin) & (own < row_end)


# ---- a CPU restatement of dense_error_kernel's predicates (upper-triangle form) ------------------------------------------
def dense_pass_visits(n, ei, ej, diag=lambda c, i: c > i, drop_last_group=False):
    """Which listed pairs (i < j) the upper-triangle dense pass reduces, from its own predicates: the tile skip
    (cb + cw - 1 <= tile_row0), the row-batch skip (cb + cw - 1 <= row0), the group load predicate `need`
    (c4 < cw and cb + c4 + 3 > row), the packed fast path (cb > row0 + 1: every pair of the batch) and the diagonal test of
    the slow path.  diag / drop_last_group: the deliberate mistakes the tests must catch."""
    i, j = np.minimum(ei, ej).astype(np.int64), np.maximum(ei, ej).astype(np.int64)
    n4 = (n + 3) & ~3
    cb = (j // CHUNK) * CHUNK
    cw = np.minimum(CHUNK, n4 - cb)
    tile_row0 = (i // TILE_ROWS) * TILE_ROWS
    row0 = i & ~1
    c4 = ((j - cb) // 4) * 4
    if drop_last_group:
        cw = np.where(cw > 4, cw - 4, cw)
    alive = ~(cb + cw - 1 <= tile_row0) & ~(cb + cw - 1 <= row0)
    need = (c4 < cw) & (cb + c4 + 3 > i)
    fast = (row0 + 1 < n) & (cb > row0 + 1)
    return alive & need & (fast | diag(j, i))


# ---- what the GPU tests assert, as functions the host tests feed modified lists into ---------------------------------------
def pass_holds(got, want, band):
    """§ the separate passes: (sum, count) against the oracle's -- the counts equal as integers, the sums inside `band`.
    Returns (holds, |difference of the sums| / band)."""
    ratio = abs(got[0] - want[0]) / band if band > 0 else (0.0 if got[0] == want[0] else np.inf)
    return int(got[1]) == int(want[1]) and ratio <= 1.0, ratio


def mae_holds(mae, want, band):
    """A check's MAE (all a trace shows) against the oracle's sum / count, inside band / count."""
    s, c = want
    ratio = abs(mae - s / c) * c / band
    return ratio <= 1.0, ratio


def row_blocks(n, blocks):
    """topolow_shard_rows: blocks of whole 8-row workgroups, empty trailing blocks dropped."""
    per = (((n + blocks - 1) // blocks) + 7) & ~7
    return tuple((b * per, min(n, (b + 1) * per)) for b in range((n + per - 1) // per))


def hand_made_blocks(n):
    """Odd row counts, starts that are no multiple of 64 or 2 (n above 1 090 only)."""
    return ((0, 1023), (1023, 1090), (1090, n)) if n > 1090 else ()


def all_blocks(n):
    return tuple(sorted(set(row_blocks(n, 2) + row_blocks(n, 3) + hand_made_blocks(n))))


def margin_for(n, dim, thresholded):
    """The one-pair margin check_needle asserts.  The margin is min |e - S/K| / (K (DIM + 6) 2^-24 mean max(r, t)) with
    |e - S/K| >= 1.1, K about n (3/4 of that with thresholds) and max(r, t) about 3 sqrt(2 dim) + 1: 100 where that can be
    reached, and 15 at the sizes the check's seams need at larger ndim (without thresholds 2 050 points reach 64 at ndim 5,
    35 at 9, 26 at 12 and 21 at 13, 2 113 points 18 at ndim 16, 8 200 points 25 at ndim 3), where one pair is still 15 bands
    and more."""
    load = n * (0.75 if thresholded else 1.0) * (kernel_dim(dim) + 6) * dim ** 0.5
    return 100.0 if load <= 28000 else 15.0


def needle(n, dim, seed, thresholded):
    """The problem of (n, dim, seed, thresholded) every test of the check uses: seams of the whole block and of all_blocks(n)."""
    return check_needle(n, dim, seed, thresholded, (), all_blocks(n) or None, margin_for(n, dim, thresholded))


# (n, dim): the sizes of the dense pass with the dims spread over them
DENSE_CASES = ((2, 1), (2, 16), (3, 2), (3, 13), (5, 3), (5, 10), (66, 5), (66, 8), (1023, 8), (1023, 2), (1025, 10),
               (1025, 3), (2050, 13), (2050, 5), (2113, 16), (2113, 1))
LIST_LENGTHS = (1, 255, 256, 257, 2049, 3 * 2048 + 1)
FUSED_CASES = tuple((n, dim) for n in (2050, 2113) for dim in (2, 5, 9, 12))
BIG_DENSE = (8200, 3)
FULL_LIST = (3000, 3)
PUSH_CASE = (2113, 5)
SEED = 0
