"""Needle problems for ONE launch of a row-owner stage kernel (slab_stage_pipe_kernel, slab_stage_wide_kernel in
csrc/relax_kernels.h, slab_stage_exact_kernel in csrc/relax_exact.h): the problems, the band, the case table and the
mutations (no GPU; used by tests/test_stage_needles_host.py and tests/test_gpu_row_owner_needles.py).

A stage kernel is held elsewhere to bands that one pair of a 180-partner row cannot leave.  Here a row has three spring
partners or fewer (kind "spring", c_repulsion 0: an unmeasured or satisfied pair contributes exactly nothing), or one close
unmeasured / satisfied pair whose repulsion carries 0.9 of its move or more (kind "repel"), and the cells that count are
planted on the columns and rows where the kernel changes what it does -- the ends of a slab part, both sides of every
256-column group seam counted from the part's first column (every chunk width is a multiple of 256), the four columns of
a group's first and last lane, the columns on either side of the wrap, the ragged end of n, the two packed rows of a
wave, the last row and the last, partly filled workgroup of a block -- so that one lost, doubled or misplaced pair is an
error of the order of the move, against _idle_and_moved's per-point band of 1e-5 of the move.

`python -m tests.stage_needles` prints, for every case of the table, the iteration the plan search found and the ratio
error / band of the model's own fp32 arithmetic against its f64 (the symmetric sweep's needle problems give 0.05 to 0.19,
these 0.02 to 0.39; a case above 0.5 is a badly built problem, never a reason for another band)."""
import collections
import dataclasses
import functools
import math

import numpy as np

from tests.models import slab_model
from topolow_amd import _native, core

K_SPRING, K_REPEL, C_REPEL = 1.5, 2.0e-5, 0.01
PLAN_SEED = 5                       # the sessions' schedule seed (Session.begin), the plan search's too
FAR = {"f32": 1.0e18, "f64": 1.0e150, "f64_exact": 1.0e150}           # phantom coordinate (csrc/relax_common.h)
# what pos_out holds before a launch: finite, negative, like no coordinate of any problem here
PATTERN = {np.dtype(np.float32): np.uint32(0xC2F0E1D2), np.dtype(np.float64): np.uint64(0xC05E1C3A5B4D2F17)}


def kernel_dim(ndim):
    """The coordinates a session computes with, the rest zero-padded (csrc/topolow_session.h: kernel_dim)."""
    return ndim if ndim <= 10 else next(d for d in (12, 16, 32, 64) if ndim <= d)


# ----------------------------------------------------------------------------------------
# the plan search
# ----------------------------------------------------------------------------------------
def plan_search_bound(n):
    """A one-stage slab starts at a random multiple of 4 among G = roundup4(n) / 4; the rarest shape asked for (a part of
    exactly 4 columns, or no wrap) is one of them: 1 / G per iteration, missed by 16 G iterations with probability e^-16."""
    return 16 * ((n + 3) // 4)


def shape_holds(ranges, want):
    b0, e0, b1, e1 = (int(v) for v in ranges)
    wrapped = e1 > b1
    if want[0] == "long":             # wrapped, both parts longer than want[1] columns
        return wrapped and e0 - b0 > want[1] and e1 - b1 > want[1]
    if want[0] == "tail4":            # wrapped, a second part of exactly 4 columns
        return wrapped and e1 - b1 == 4
    if want[0] == "head4":            # wrapped, a first part of exactly 4 columns
        return wrapped and e0 - b0 == 4
    if want[0] == "wrapped":
        return wrapped
    if want[0] == "flat":
        return not wrapped
    assert want[0] == "any", want
    return True


@functools.lru_cache(maxsize=None)
def find_iteration(n, stages, seed, want, slot=0):
    """The first it = 0, 1, ... whose slab at `slot` of an iteration of `stages` stages has the wanted shape (shape_holds),
    with that slab's (b0, e0, b1, e1): the host's plan query, no device."""
    for it in range(plan_search_bound(n)):
        plan = _native.slab_plan(n, stages, seed, it)
        if slot < len(plan) and shape_holds(plan[slot], want):
            return it, tuple(int(v) for v in plan[slot])
    raise AssertionError("no iteration below %d gives %r at slot %d of %d stages of %d points" %
                         (plan_search_bound(n), want, slot, stages, n))


# ----------------------------------------------------------------------------------------
# the planted columns and rows
# ----------------------------------------------------------------------------------------
def special_columns(n, ranges, wide=False):
    """{column: class}, the classes in the order they are served when rows run short.  Columns of points only: the
    columns n ... roundup4(n) - 1 are the phantom point and hold no pair."""
    b0, e0, b1, e1 = ranges
    n4 = (n + 3) // 4 * 4
    parts = [(b, e) for b, e in ((b0, e0), (b1, e1)) if e > b]
    found = {}

    def add(c, label, b, e):
        if b <= c < min(e, n):
            found.setdefault(c, label)

    for b, e in parts:
        add(b, "part begin", b, e)
        add(min(e - 1, n - 1), "part end", b, e)
    if len(parts) == 2:
        add(min(n4 - 1, n - 1), "before the wrap", b0, e0)
        add(0, "after the wrap", b1, e1)
    if n % 4:
        for b, e in parts:
            add(n - 1, "ragged end", b, e)
    for b, e in parts:
        if wide:                       # a lane walks every 64th column from b
            for c in (b + 63, b + 64):
                add(c, "lane stride", b, e)
            continue
        for q in range(1, (e - b + 255) // 256):
            add(b + 256 * q - 1, "group seam", b, e)
            add(b + 256 * q, "group seam", b, e)
        q = max((min(e, n) - b) // 256 - 1, 0)          # the last whole group of the part, else its only one
        for j in range(4):
            add(b + 256 * q + j, "first lane", b, e)
            add(b + 256 * q + 252 + j, "last lane", b, e)
    return found


def special_rows(row_begin, row_end):
    """Rows of the block in the order they are served: the two packed halves of the first wave, the last row, the last,
    partly filled workgroup (8 rows per workgroup), then the rest of the first workgroup and the last whole one -- three
    cells a row would not go round the special columns with the first four kinds alone."""
    nr = row_end - row_begin
    last0 = row_begin + 8 * ((nr - 1) // 8)
    order = [row_begin, row_begin + 1, row_end - 1] + list(range(last0, row_end)) + \
        list(range(row_begin, row_begin + 8)) + list(range(last0 - 8, last0))
    return [r for r in dict.fromkeys(order) if row_begin <= r < row_end]


def _plant_round(plant, pool, cols, cells, every_row):
    """Every column on a row of the pool, neighbouring columns on different rows (the first row that takes it, from the
    column's turn on); every_row (a list of columns): every row of the pool that holds no cell yet on one of them."""
    if not pool:
        return
    for t, c in enumerate(cols):
        any(plant(pool[(t + q) % len(pool)], c) for q in range(len(pool)))
    if every_row:
        for t, i in enumerate(pool):
            if not any(row == i for row, _ in cells):
                any(plant(i, every_row[(t + q) % len(every_row)]) for q in range(len(every_row)))


Needle = collections.namedtuple(
    "Needle", "n ndim ranges row_begin row_end thresholded kind k c_rep call call_r cells labels srows active want "
              "want_exact flagged")


def _round_to_word(t):
    """A target as the device keeps it: fp32 rounded to 4 ulp (the two low bits hold the code); tests/test_gpu_parity.py,
    _decode_rounded, on a list."""
    u = np.asarray(t, dtype=np.float64).astype(np.float32).view(np.uint32)
    mag = ((u & np.uint32(0x7FFFFFFF)) + np.uint32(2)) & np.uint32(0xFFFFFFFC)
    return ((u & np.uint32(0x80000000)) | mag).view(np.float32).astype(np.float64)


def _start_positions(rng, n, ndim, kind):
    if kind == "spring":
        return 3.0 * rng.standard_normal((n, ndim))
    # repel: everything far apart -- a jittered grid (a line at ndim 1) of spacing 1 that starts at 20, shuffled; the other
    # coordinates 3 N(0, 1).  (A point at the origin of a line has a move that is the small difference of the repulsions
    # from either side and no coordinate for the band's rounding term: the model's own fp32 leaves the band there.)
    pos = 3.0 * rng.standard_normal((n, ndim))
    where = rng.permutation(n)
    if ndim == 1:
        pos[:, 0] = 20.0 + where + rng.uniform(-0.2, 0.2, n)
    else:
        side = int(math.ceil(math.sqrt(n)))
        pos[:, 0] = 20.0 + where % side + rng.uniform(-0.2, 0.2, n)
        pos[:, 1] = where // side + rng.uniform(-0.2, 0.2, n)
    return pos


def in_ranges(n, ranges):
    m = np.zeros(n, dtype=bool)
    m[ranges[0]:min(ranges[1], n)] = True
    m[ranges[2]:min(ranges[3], n)] = True
    return m


class _Draft:
    """A needle problem while it is built: the rows and columns chosen for it, the start positions, the measured pairs
    {(lo, hi): (factor, code)} -- target = factor x the start distance -- and the planted cells."""

    def __init__(self, n, ndim, ranges, row_begin, row_end, thresholded, kind, seed, wide):
        self.rng = np.random.default_rng([n, ndim, seed, int(thresholded), kind == "repel", row_begin, row_end] + list(ranges))
        self.n, self.ndim, self.ranges, self.row_begin, self.row_end = n, ndim, ranges, row_begin, row_end
        self.thresholded, self.kind, self.spring_kind = thresholded, kind, kind == "spring"
        self.nr = row_end - row_begin
        self.block = list(range(row_begin, row_end))
        self.inr = in_ranges(n, ranges)
        self.labels = special_columns(n, ranges, wide)
        self.edges, self.cells, self.idle = {}, [], []
        self._choose_rows()
        # thresholded: wave w of the block may carry codes on both rows (w % 3 == 0), on its first row only (1), on none (2)
        self.may_code = np.ones(n, dtype=bool)
        if thresholded:
            rel = np.arange(self.nr)
            wave_class = (rel // 2) % 3
            self.may_code[row_begin:row_end] = (wave_class == 0) | ((wave_class == 1) & (rel % 2 == 0))
        self.pos = _start_positions(self.rng, n, ndim, kind)

    def _choose_rows(self):
        """idle (spring: 6 % of the block, not the first three waves, the last row or a special column), cols (the special
        columns in the order they are served), srows (special rows) and orows (ordinary rows spread over the block)."""
        rng, block, labels, nr = self.rng, self.block, self.labels, self.nr
        srows = special_rows(self.row_begin, self.row_end)
        if self.spring_kind and nr >= 2:
            keep = set(srows[:3]) | set(block[:6] if nr >= 24 else ())       # the first three waves: one of each kind of codes
            pool = [r for r in block if r not in keep and r not in labels] or [r for r in block if r not in keep]
            self.idle = sorted(rng.choice(pool, size=min(len(pool), max(1, math.ceil(0.06 * nr))), replace=False).tolist())
            for r in self.idle:
                labels.pop(r, None)
        if not self.spring_kind:
            # a repel row lies beside its column and cannot be the column of other rows: the rows of the first two waves
            # (the packed halves; with thresholds the wave with codes on both rows and the one with codes on one) are
            # rows, and where they are special columns too, those columns go unplanted in this kind
            for r in (block[:4] if nr >= 24 else srows[:2]):
                if len(labels) > 1:
                    labels.pop(r, None)
        self.cols = list(labels)
        assert self.cols, (self.n, self.ranges)
        usable = [r for r in block if r not in self.idle and (self.spring_kind or r not in labels)]
        self.srows = [r for r in srows if r in usable]
        rest = [r for r in usable if r not in self.srows]
        if sum(1 for r in rest if r not in labels) >= 16:
            rest = [r for r in rest if r not in labels]
        orows = [rest[int(q)] for q in np.linspace(0, len(rest) - 1, min(len(rest), max(len(self.cols), 16)))] if rest else []
        self.orows = list(dict.fromkeys(orows))
        if not self.spring_kind and self.thresholded:
            # a repel row takes one cell, so the special rows reach only the first len(srows) columns: with thresholds the
            # columns are served from where the plain problem's special rows stopped, and the two together reach them all
            turn = len(self.srows) % len(self.cols)
            self.cols = self.cols[turn:] + self.cols[:turn]

    def measure(self, i, c, planted, coded=True):
        """The pair {i, c} becomes measured; coded = False: with code 0 whatever the problem."""
        rng = self.rng
        factor = 2.0 if rng.random() < 0.5 else 0.5
        if self.spring_kind:
            # every spring of row i pulls its first coordinate the same way (up), so that a move is never the small
            # difference of two terms -- at ndim 1 the model's own fp32 leaves the band on such a row
            factor = 2.0 if self.pos[c, 0] > self.pos[i, 0] else 0.5
        code = 0
        if self.thresholded and coded and self.may_code[i] and self.may_code[c]:
            u, zero = rng.random(), 0.2 if planted else 0.5                 # code 0 / ">" / "<": 0.2, 0.4, 0.4 or 0.5, 0.25, 0.25
            code = 0 if u < zero else (1 if u < 0.5 + 0.5 * zero else -1)
        if planted and self.spring_kind and code != 0:
            code = 1 if factor > 1.0 else -1               # violated: a spring
        if planted and not self.spring_kind:
            factor = 0.5 if code == 1 else 2.0             # satisfied: the repulsion branch
        self.edges[(min(i, c), max(i, c))] = (factor, code)

    def plant_rounds(self, plant, ordinary):
        _plant_round(plant, self.srows, self.cols, self.cells, every_row=False)
        _plant_round(plant, ordinary(), self.cols, self.cells, every_row=False)
        _plant_round(plant, self.srows, [], self.cells, every_row=self.cols)


def _plant_spring(d):
    """spring: c_repulsion 0, k 1.5; positions 3 N(0, 1); targets r0 x {0.5, 2} -- 2 where the column lies above the row in
    the first coordinate; thresholded: a planted cell always on its violated side (a satisfied one would count for nothing
    and could not be missed).  A row takes three partners at the most.  Measured besides the planted cells: two cells per
    other row, inside the ranges, on every third free column, never in a planted or an idle row or column."""
    partners = collections.defaultdict(set)
    rowpool = set(d.srows) | set(d.orows)

    def plant(i, c):
        if i == c or c in partners[i]:
            return False
        if i in d.labels and any(row == i for row, _ in d.cells):
            return False           # a row that is a special column too keeps two of its three partners for its column
        if any(len(partners[p]) >= 3 for p in (i, c) if p in rowpool):
            return False
        partners[i].add(c)
        partners[c].add(i)
        d.measure(i, c, True)
        d.cells.append((i, c))
        return True

    d.plant_rounds(plant, lambda: d.orows)
    # the background -- the rows of its columns take no cells of their own (theirs all pull down)
    taken = rowpool | set(d.idle)
    allowed = np.array([c for c in np.flatnonzero(d.inr).tolist() if c not in taken], dtype=int)[::3]
    hubs = set(allowed.tolist())
    if len(allowed):
        for i in d.block:
            if i in taken or i in hubs:
                continue
            for c in allowed[d.rng.integers(len(allowed), size=2)].tolist():
                if c != i:
                    d.measure(i, c, False)


def _plant_repel(d):
    """repel: c_repulsion 0.01, k 2e-5 (springs a few 1e-2 of a planted term at the most), points a unit apart; a planted
    cell is unmeasured, or when thresholded and both its points may carry codes a threshold pair on its satisfied side;
    its row lies 0.02 to 0.03 from its column, one planted cell per row; the rows of one column are measured among each
    other (a weak spring, no second close repulsion) and a planted cell's neighbours c - 1, c + 1 in its row are measured
    with code 0, so that the word of the neighbouring column is another word."""
    rng, edges = d.rng, d.edges
    used, column_of = set(), {}
    members = collections.defaultdict(list)

    def plant(i, c):
        if i == c or i in used or i in members or c in column_of:
            return False
        used.add(i)
        column_of[i] = c
        members[c].append(i)
        d.cells.append((i, c))
        return True

    d.plant_rounds(plant, lambda: [r for r in d.orows if r not in used])
    for c, rows_of in members.items():
        for i in rows_of:                       # in a direction of its own -- up in the first coordinate, or the column's
            u = rng.standard_normal(d.ndim)     # own move is a small difference
            u[0] = abs(u[0])
            near = 0.020 if (i - d.row_begin) % 2 == 0 else 0.026       # the two rows of a wave never at one distance
            d.pos[i] = d.pos[c] + rng.uniform(near, near + 0.004) * u / np.sqrt((u * u).sum())
    d.pos = d.pos.astype(np.float32).astype(np.float64)
    for c, rows_of in members.items():
        for a in range(len(rows_of)):
            for b in range(a + 1, len(rows_of)):
                d.measure(rows_of[a], rows_of[b], False, coded=False)      # a spring whatever the distance
    for i, c in d.cells:
        if d.thresholded and d.may_code[i] and d.may_code[c] and rng.random() < 0.7:
            d.measure(i, c, True)
            if edges[(min(i, c), max(i, c))][1] == 0:
                del edges[(min(i, c), max(i, c))]        # code 0 would be a spring: this cell stays unmeasured
        for e in (c - 1, c + 1):
            if 0 <= e < d.n and e != i and column_of.get(i) != e and (min(i, e), max(i, e)) not in edges \
                    and e not in members.get(c, ()) and column_of.get(e) != i:
                d.measure(i, e, False, coded=False)
    taken = set(used) | set(members)
    allowed = np.array([c for c in np.flatnonzero(d.inr).tolist() if c not in taken], dtype=int)
    if len(allowed):
        for i in d.block:
            if i not in taken:
                c = int(allowed[rng.integers(len(allowed))])
                if c != i:
                    d.measure(i, c, False)


def _code_the_first_rows(d):
    """thresholded: the first three rows carry a code whatever their cells drew (the first wave on both rows, the second
    on its first): if need be through a satisfied threshold pair with a far point, which moves nothing (spring) or repels
    as the unmeasured pair did (repel)."""
    coded = {p for key, (_, code) in d.edges.items() if code != 0 for p in key}
    busy = {p for i, c in d.cells for p in (i, c)} | set(d.labels) | set(d.idle)
    spare = [c for c in np.flatnonzero(d.may_code).tolist() if c not in busy]
    for q, i in enumerate(d.block[:3]):
        far = [c for c in spare[q::3] if (min(i, c), max(i, c)) not in d.edges and c != i]
        if i not in coded and i not in d.idle and far:
            d.edges[(min(i, far[0]), max(i, far[0]))] = (0.5, 1)


@functools.lru_cache(maxsize=4)
def stage_needle(n, ndim, ranges, row_begin, row_end, thresholded, kind, seed, wide=False, exact=False):
    """The problem of one launch over the columns `ranges` = (b0, e0, b1, e1) and the rows [row_begin, row_end): the kinds
    are _plant_spring and _plant_repel, the choice of rows and columns _Draft.

    Returns a Needle: call (LayoutCall), call_r (targets as the device rounds them), cells [(row, column)], labels
    {column: class}, srows, active (points with a spring partner in `ranges`; repel: every point), want / want_exact (the
    f64 model's stage on the rounded / with `exact` on the unrounded targets), flagged (rows that hold a code)."""
    d = _Draft(n, ndim, ranges, row_begin, row_end, thresholded, kind, seed, wide)
    (_plant_spring if d.spring_kind else _plant_repel)(d)
    pos = d.pos.astype(np.float32).astype(np.float64)
    if thresholded and d.nr >= 24:
        _code_the_first_rows(d)
    edges, inr = d.edges, d.inr
    k, c_rep = (K_SPRING, 0.0) if d.spring_kind else (K_REPEL, C_REPEL)

    keys = sorted(edges, key=lambda e: (e[1], e[0]))           # column-major, as core.prepare_layout_call lists the edges
    ei = np.array([e[0] for e in keys], dtype=np.int32)
    ej = np.array([e[1] for e in keys], dtype=np.int32)
    factor = np.array([edges[e][0] for e in keys])
    code = np.array([edges[e][1] for e in keys], dtype=np.int32)
    r0 = np.sqrt(((pos[ei] - pos[ej]) ** 2).sum(-1))
    target = r0 * factor
    D = np.full((n, n), np.inf, order="F")
    T = np.zeros((n, n), dtype=np.int32, order="F")
    D[ei, ej] = D[ej, ei] = target
    T[ei, ej] = T[ej, ei] = code
    np.fill_diagonal(D, 0.0)
    D_r = D.copy(order="F")
    D_r[ei, ej] = D_r[ej, ei] = _round_to_word(target)
    degrees = (np.bincount(ei, minlength=n) + np.bincount(ej, minlength=n) + 1).astype(np.int32)   # the diagonal included
    call = core.LayoutCall(initial_positions=pos, dissimilarity_matrix=D, threshold_matrix=T, degrees=degrees, edge_i=ei,
                           edge_j=ej, edge_dist=target, edge_thresh=code, n_iter=1, k0=k, cooling_rate=0.01,
                           c_repulsion=c_rep, relative_epsilon=1e-12, convergence_window=10 ** 9,
                           convergence_check_freq=3, verbose=False)
    call_r = dataclasses.replace(call, dissimilarity_matrix=D_r)
    spring = (code == 0) | ((code == 1) & (factor > 1.0)) | ((code == -1) & (factor < 1.0))
    if d.spring_kind:
        active = np.zeros(n, dtype=bool)
        active[ei[spring & inr[ej]]] = True
        active[ej[spring & inr[ei]]] = True
    else:
        active = np.ones(n, dtype=bool)
    flagged = np.zeros(n, dtype=bool)
    flagged[ei[code != 0]] = True
    flagged[ej[code != 0]] = True
    rg = np.array(ranges, dtype=np.int32).reshape(2, 2)
    want = slab_model.stage(pos, D_r, T, degrees, rg, k, c_rep, "f64")
    want_exact = slab_model.stage(pos, D, T, degrees, rg, k, c_rep, "f64") if exact else want
    for a in (pos, D, T, D_r, degrees, ei, ej, target, code, active, want, want_exact, flagged):
        a.setflags(write=False)
    nd = Needle(n, ndim, tuple(ranges), row_begin, row_end, thresholded, kind, k, c_rep, call, call_r, tuple(d.cells),
                d.labels, tuple(d.srows), active, want, want_exact, flagged)
    _assert_coverage(nd, d.idle, d.orows, d.nr < 24)     # (under 24 rows they do not go round the columns)
    return nd


def spring_pairs_at_start(nd):
    """Pairs of the whole list whose spring is active on the start positions."""
    c = nd.call
    r0 = np.sqrt(((c.initial_positions[c.edge_i] - c.initial_positions[c.edge_j]) ** 2).sum(-1))
    return int(((c.edge_thresh == 0) | ((c.edge_thresh == 1) & (r0 < c.edge_dist)) |
                ((c.edge_thresh == -1) & (r0 > c.edge_dist))).sum())


def _assert_coverage(nd, idle, orows, tiny):
    """What the builder promises (the host test runs it for every case of the table)."""
    nr = nd.row_end - nd.row_begin
    cells, labels, srows = nd.cells, nd.labels, list(nd.srows)
    inr = in_ranges(nd.n, nd.ranges)
    assert cells and len(set(cells)) == len(cells)
    per_row = collections.Counter(i for i, _ in cells)
    for i, c in cells:
        assert nd.row_begin <= i < nd.row_end and inr[c] and c in labels and i != c, (i, c)
    T, D = nd.call.threshold_matrix, nd.call.dissimilarity_matrix
    if nd.kind == "spring":
        # three spring partners or fewer in every planted cell's row, each of them a planted cell of that row or (among a
        # handful of points, where rows are columns too) of the partner's row
        pos = nd.call.initial_positions
        for i in per_row:
            measured = np.flatnonzero(np.isfinite(D[i]) & inr)
            r = np.sqrt(((pos[measured] - pos[i]) ** 2).sum(-1))
            springs = (T[i, measured] == 0) | ((T[i, measured] == 1) & (r < D[i, measured])) | \
                ((T[i, measured] == -1) & (r > D[i, measured]))
            measured = measured[(measured != i) & springs]
            assert 1 <= len(measured) <= 3, (i, measured)
            assert all((i, c) in cells or (c, i) in cells for c in measured.tolist()), (i, measured)
            assert nd.active[i]
        assert all(not nd.active[r] for r in idle) and (nr < 2 or len(idle) >= 0.05 * nr), idle
    else:
        assert max(per_row.values()) == 1
        for i, c in cells:                 # unmeasured, or a threshold pair on its satisfied side
            assert not np.isfinite(D[i, c]) or T[i, c] != 0, (i, c)
    if nr >= 2 and srows[:2] == [nd.row_begin, nd.row_begin + 1]:
        # the two packed halves of the first wave: planted, with different partners
        a = {c for i, c in cells if i == nd.row_begin}
        b = {c for i, c in cells if i == nd.row_begin + 1}
        assert a and b and a != b, (a, b)
    if not tiny:
        assert nd.row_end - 1 in per_row or nd.row_end - 1 in labels or nd.row_end - 1 in idle
        last0 = nd.row_begin + 8 * ((nr - 1) // 8)
        assert any(last0 <= i < nd.row_end for i in per_row) or all(r in labels for r in range(last0, nd.row_end))
        assert any(i not in srows for i in per_row) or not orows          # ordinary rows in between
        # every special column on a special row and on an ordinary one -- where the rows go round: a spring row takes
        # three cells, a repel row one
        on_special = {c for i, c in cells if i in srows}
        on_ordinary = {c for i, c in cells if i not in srows}
        per = 3 if nd.kind == "spring" else 1
        if per * len(srows) >= len(labels):
            assert on_special == set(labels), sorted(set(labels) - on_special)
        else:
            assert len(on_special) >= min(len(labels), len(srows)), (len(on_special), len(srows))
        if len(orows) >= len(labels):
            assert on_ordinary == set(labels), sorted(set(labels) - on_ordinary)
    if nd.thresholded and nr >= 24 and not tiny:
        # a wave whose two rows both carry codes, one with codes on exactly one row, one with none -- each with a planted
        # row (with a row that moves, where a handful of special columns cannot reach three waves)
        seen = set()
        for i in (per_row if len(labels) >= 8 else np.flatnonzero(nd.active).tolist()):
            if not nd.row_begin <= i < nd.row_end:
                continue
            w0 = nd.row_begin + 2 * ((i - nd.row_begin) // 2)
            if w0 + 1 < nd.row_end:
                seen.add(int(nd.flagged[w0]) + int(nd.flagged[w0 + 1]))
        assert seen == {0, 1, 2}, seen


# ----------------------------------------------------------------------------------------
# one pair's term, and the repel kind's own condition
# ----------------------------------------------------------------------------------------
def pair_term(nd, i, c, t, code):
    """What the pair (row i, column c) takes from row i's coordinates in one stage when its word reads (t, code)."""
    pos, g = nd.call.initial_positions, float(nd.call.degrees[i]) + 1.0
    delta = pos[c] - pos[i]
    r = math.sqrt(float((delta * delta).sum()))
    rs = r + 0.01
    spring = math.isfinite(t) and (code == 0 or (code == 1 and r < t) or (code == -1 and r > t))
    coef = 2.0 * nd.k * (t - r) / rs / (4.0 * g + nd.k) if spring else nd.c_rep / (2.0 * rs * rs * rs) / g
    return delta * coef


def cell_term(nd, i, c, exact=False):
    D = (nd.call if exact else nd.call_r).dissimilarity_matrix
    return pair_term(nd, i, c, float(D[i, c]), int(nd.call.threshold_matrix[i, c]))


def planted_share(nd):
    """repel: the smallest share |term| / |move| over the planted cells, and the largest |move - term| / |move|."""
    start = nd.call.initial_positions
    least, off = np.inf, 0.0
    for i, c in nd.cells:
        move, term = start[i] - nd.want[i], cell_term(nd, i, c)
        size = np.sqrt((move * move).sum())
        least = min(least, np.sqrt((term * term).sum()) / size)
        off = max(off, np.sqrt(((move - term) ** 2).sum()) / size)
    return least, off


# ----------------------------------------------------------------------------------------
# the buffers of a launch and what is asserted of them
# ----------------------------------------------------------------------------------------
def guard_rows(nd):
    """Rows a caller's buffers hold beyond the padded points: the launch must leave them alone like every row outside its
    block, and in the repel kind, where every point moves, they stand where _idle_and_moved asks for idle points."""
    return (nd.row_end - nd.row_begin) // 16 + 1


def launch_buffers(nd, dtype):
    """(pos_in, pos_out) as sharded.HipBackend.new_positions lays them out: roundup4(n) rows (and the guard rows) of
    kernel_dim coordinates, the phantom coordinate in the rows from n on; pos_out filled with PATTERN."""
    dtype = np.dtype(dtype)
    rows, kd = (nd.n + 3) // 4 * 4 + guard_rows(nd), kernel_dim(nd.ndim)
    pos_in = np.zeros((rows, kd), dtype=dtype)
    pos_in[:nd.n, :nd.ndim] = nd.call.initial_positions
    pos_in[nd.n:, 0] = FAR["f32" if dtype == np.float32 else "f64"]
    pos_out = np.empty((rows, kd), dtype=dtype)
    pos_out.view(PATTERN[dtype].dtype)[...] = PATTERN[dtype]
    return pos_in, pos_out


def model_output(nd, want=None):
    """The pos_out the model's stage would leave, in f64."""
    _, out = launch_buffers(nd, np.float64)
    out[nd.row_begin:nd.row_end] = 0.0
    out[nd.row_begin:nd.row_end, :nd.ndim] = (nd.want if want is None else want)[nd.row_begin:nd.row_end]
    return out


def hold(nd, pos_out, precision, exact=False):
    """What every launch is held to.  pos_out: the buffer after the launch (any float type).
      * every other row of pos_out, the padding and the guard rows included, holds PATTERN bit for bit;
      * the zero-padded coordinates of the block's rows are exactly 0;
      * (i) and (ii) of tests/test_gpu_symmetric_long_runs.py, _idle_and_moved, over the block's rows, against the f64
        model's stage from the start positions: idle rows bit-equal to the start, fp32 |got - want| <= 1e-5 |move| +
        2^-22 |p| per point, f64 1e-12 of the largest move.  In the repel kind every point of the block moves: the guard
        rows, which the launch must leave as they were, are the idle points _idle_and_moved asks for.
    Returns the largest error / band."""
    from tests.test_gpu_symmetric_long_runs import _idle_and_moved
    pattern = PATTERN[pos_out.dtype]
    bits = pos_out.view(pattern.dtype)
    rows = slice(nd.row_begin, nd.row_end)
    clean = (bits[:nd.row_begin] == pattern).all() and (bits[nd.row_end:] == pattern).all()
    assert clean, ("written outside the block", np.flatnonzero((bits != pattern).any(axis=1))[:8])
    assert (pos_out[rows, nd.ndim:] == 0).all()
    got = pos_out[rows, :nd.ndim].astype(np.float64)
    want = (nd.want_exact if exact else nd.want)[rows]
    start, active = nd.call.initial_positions[rows], nd.active[rows]
    if nd.kind == "repel":
        guard = pos_out[-guard_rows(nd):, :nd.ndim].astype(np.float64)
        got, want, start = (np.concatenate([a, guard]) for a in (got, want, start))
        want[-len(guard):] = start[-len(guard):] = np.frombuffer(pattern.tobytes(), dtype=pos_out.dtype)[0]
        active = np.concatenate([active, np.zeros(len(guard), dtype=bool)])
    return _idle_and_moved(got, want, start, active, "f32" if precision == "f32" else "f64")


# ----------------------------------------------------------------------------------------
# the mutations: what one wrong pair, one swapped wave or one stray store would leave in pos_out
# ----------------------------------------------------------------------------------------
def mutations(nd, exact=False):
    """(name, cell, pos_out) for every planted cell (i, c), from the model's pos_out (out = start - sum of terms):
      lost       the cell's term dropped from row i (spring, c_repulsion 0: the stage with the cell unmeasured);
      doubled    the term added twice;
      column-1 / column+1   the cell's word taken from the neighbouring column of the row (skipped where that column is
                 the diagonal or no point);
      halves     the moves of the wave's two rows exchanged (the .x / .y of the packed accumulators), and
      outputs    the two rows' outputs exchanged (skipped where the wave has one row);
      stray      a row outside the block written (a guard row where the block is everything) with row i's output."""
    base = model_output(nd, nd.want_exact if exact else nd.want)
    start = nd.call.initial_positions
    D = (nd.call if exact else nd.call_r).dissimilarity_matrix
    T = nd.call.threshold_matrix
    d = nd.ndim
    rows_total = base.shape[0]
    for i, c in nd.cells:
        term = cell_term(nd, i, c, exact)
        out = base.copy()
        out[i, :d] += term
        yield "lost", (i, c), out
        out = base.copy()
        out[i, :d] -= term
        yield "doubled", (i, c), out
        for name, other in (("column-1", c - 1), ("column+1", c + 1)):
            if 0 <= other < nd.n and other != i:
                out = base.copy()
                out[i, :d] += term - pair_term(nd, i, c, float(D[i, other]), int(T[i, other]))
                yield name, (i, c), out
        j = nd.row_begin + ((i - nd.row_begin) ^ 1)
        if j < nd.row_end:
            out = base.copy()
            out[i, :d] = start[i] + (base[j, :d] - start[j])
            out[j, :d] = start[j] + (base[i, :d] - start[i])
            yield "halves", (i, c), out
            out = base.copy()
            out[[i, j]] = base[[j, i]]
            yield "outputs", (i, c), out
        outside = [r for r in (nd.row_begin - 1, nd.row_end) if 0 <= r < nd.n] or [rows_total - 1 - (i % guard_rows(nd))]
        out = base.copy()
        out[outside[(i + c) % len(outside)]] = base[i]
        yield "stray", (i, c), out


# ----------------------------------------------------------------------------------------
# the case table
# ----------------------------------------------------------------------------------------
# n = 2 W + 256 + 7, W the widest chunk of the ndim and precision (PipeGeom in csrc/relax_kernels.h: fp32 1024 columns at
# ndim 1-2, 768 at 3, 512 at 4-5, 256 from 6; f64 and f64_exact 1024 at ndim 1, 512 at 2, 256 from 3)
PLAIN_DIMS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16)
MAIN_N = {"f32": {1: 2311, 2: 2311, 3: 1799, 4: 1287, 5: 1287}, "f64": {1: 2311, 2: 1287}, "f64_exact": {1: 2311, 2: 1287}}
# The widest chunk of the instances that run at each size (773: n % 4 = 1; the even sizes: the ERR launches).  The "long"
# shape asks for both parts longer than it -- n = 2 W + 263 has no room for more.  This restates PipeGeom: a wider chunk
# there would leave these launches passing with parts shorter than a chunk, so the two change together.
WIDEST_CHUNK = {2311: 1024, 1799: 768, 1287: 512, 775: 256, 773: 256, 2312: 1024, 1288: 512, 776: 256}

Launch = collections.namedtuple("Launch", "n stages slot shape rows")          # rows: None (all), or (row_begin, row_end)


def main_n(precision, ndim):
    return MAIN_N[precision].get(ndim, 775)


def shapes(n):
    """One stage of one: wrapped with both parts longer than the widest chunk, with a 4-column second part, with a
    4-column first part, not wrapped; every slot of a 3-stage iteration; a wrapped slot of a 16-stage iteration (a slab
    narrower than a group)."""
    w = WIDEST_CHUNK[n]
    return [Launch(n, 1, 0, ("long", w), None), Launch(n, 1, 0, ("tail4",), None), Launch(n, 1, 0, ("head4",), None),
            Launch(n, 1, 0, ("flat",), None), Launch(n, 3, 0, ("any",), None), Launch(n, 3, 1, ("any",), None),
            Launch(n, 3, 2, ("any",), None), Launch(n, 16, 0, ("wrapped",), None)]


def plain_launches(precision, ndim):
    """The launches of one instance and kind: the shapes at the main size, one ragged group (70 points, wrapped), and at
    ndim 3 five points, at ndim 7 the main shapes' first three again with n % 4 = 1."""
    out = shapes(main_n(precision, ndim)) + [Launch(70, 1, 0, ("wrapped",), None)]
    if ndim == 3:
        out += [Launch(5, 1, 0, ("wrapped",), None), Launch(5, 1, 0, ("flat",), None)]
    if ndim == 7:
        out += shapes(773)[:3]
    return out


EXACT_DIMS = (2, 5, 10, 16)
BLOCK_DIMS = (2, 5, 9)
WIDE_DIMS = (17, 32, 64)
ERR_DIMS = (2, 4, 5, 7, 9, 12, 16)


def block_launches(precision, ndim):
    """Row blocks at the main size, one stage of one, wrapped with both parts long: an odd count of rows that starts and
    ends off a multiple of 8, the last block, and a block from which single rows are launched (ONE_ROW)."""
    n = main_n(precision, ndim)
    long_ = ("long", WIDEST_CHUNK[n])
    return [Launch(n, 1, 0, long_, (259, 518)), Launch(n, 1, 0, long_, (n - 261, n)), Launch(n, 3, 1, ("any",), (259, 518)),
            Launch(n, 1, 0, long_, ONE_ROW)]


ONE_ROW = (300, 312)                # the rows launched one at a time, each by a session of its own (a block of one row)


def wide_launches():
    """331 and 70 points wrapped and not, 331 with a 4-column part at either end, and a slot of a 3-stage iteration."""
    return [Launch(n, 1, 0, (w,), None) for n in (331, 70) for w in ("wrapped", "flat")] + \
        [Launch(331, 1, 0, ("tail4",), None), Launch(331, 1, 0, ("head4",), None), Launch(331, 3, 1, ("any",), None)]


def exact_launches(ndim):
    """The shapes at the main size, one ragged group, and at ndim 5 five points."""
    out = shapes(main_n("f64_exact", ndim)) + [Launch(70, 1, 0, ("wrapped",), None)]
    if ndim == 5:
        out += [Launch(5, 1, 0, ("wrapped",), None), Launch(5, 1, 0, ("flat",), None)]
    return out


def err_launches(ndim):
    """ERR launches are one-stage iterations of a block with an even row count: the main size and one point, wrapped with
    both parts longer than the widest chunk, with a 4-column second part, with a 4-column first part; 70 points (a slab
    narrower than a group)."""
    n = main_n("f32", ndim) + 1
    return shapes(n)[:3] + [Launch(70, 1, 0, ("wrapped",), None)]


def needle_of(launch, ndim, thresholded, kind, wide=False, exact=False):
    """(it, needle) of a launch of the table."""
    it, ranges = find_iteration(launch.n, launch.stages, PLAN_SEED, launch.shape, launch.slot)
    rb, re = launch.rows or (0, launch.n)
    return it, stage_needle(launch.n, ndim, ranges, rb, re, thresholded, kind, 0, wide, exact)


def all_groups():
    """(label, ndim, wide, launches) of every group of launches the GPU file runs; each with and without thresholds and
    in both kinds.  Precisions that share a size share the problems."""
    seen = {}
    for precision in ("f32", "f64"):
        for ndim in PLAIN_DIMS:
            seen.setdefault((ndim, False, tuple(plain_launches(precision, ndim))), "plain %s ndim %d" % (precision, ndim))
        for ndim in BLOCK_DIMS:
            seen.setdefault((ndim, False, tuple(block_launches(precision, ndim))), "blocks %s ndim %d" % (precision, ndim))
    for ndim in EXACT_DIMS:
        seen.setdefault((ndim, False, tuple(exact_launches(ndim))), "exact ndim %d" % ndim)
    for ndim in WIDE_DIMS:
        seen.setdefault((ndim, True, tuple(wide_launches())), "wide ndim %d" % ndim)
    for ndim in ERR_DIMS:
        seen.setdefault((ndim, False, tuple(err_launches(ndim))), "err ndim %d" % ndim)
    return [(label, ndim, wide, list(launches)) for (ndim, wide, launches), label in seen.items()]


def f64_band_is_the_tighter(nd, exact=False):
    """1e-12 of the largest move is below every point's fp32 band: what leaves the fp32 band leaves the f64 band."""
    rows = slice(nd.row_begin, nd.row_end)
    start, want = nd.call.initial_positions[rows], (nd.want_exact if exact else nd.want)[rows]
    move = np.abs(want - start).max(axis=1)[nd.active[rows]]
    return 1e-12 * move.max() <= (1e-5 * move + 2.0 ** -22 * np.abs(start[nd.active[rows]]).max(axis=1)).min()


def model_f32_ratio(nd):
    """error / band of the model's own fp32 arithmetic against its f64."""
    c = nd.call_r
    rg = np.array(nd.ranges, dtype=np.int32).reshape(2, 2)
    f32 = slab_model.stage(c.initial_positions, c.dissimilarity_matrix, c.threshold_matrix, c.degrees, rg, nd.k, nd.c_rep,
                           "f32")
    return hold(nd, model_output(nd, f32), "f32")


if __name__ == "__main__":
    worst = 0.0
    for label, ndim, wide, launches in all_groups():
        for launch in launches:
            for thresholded in (False, True):
                for kind in ("spring", "repel"):
                    it, nd = needle_of(launch, ndim, thresholded, kind, wide)
                    ratio = model_f32_ratio(nd)
                    worst = max(worst, ratio)
                    print("%-22s n %4d stages %2d slot %d %-14s rows %-10s thr %d %-6s it %5d (bound %5d) ranges %-24s "
                          "cells %3d  fp32 model / band %.3f" % (label, launch.n, launch.stages, launch.slot, launch.shape,
                                                                 launch.rows, thresholded, kind, it,
                                                                 plan_search_bound(launch.n), nd.ranges, len(nd.cells), ratio))
    print("largest fp32 model / band: %.3f" % worst)
    assert worst <= 0.5
