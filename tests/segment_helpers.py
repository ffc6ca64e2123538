"""P ranks of the caller-driven symmetric sweep (include/topolow_relax.h: topolow_session_symm_segment_build / _sweep /
_apply) on ONE device in ONE process, in lock-step, without torch.distributed: what sharded.HipBackend.symm_prepare and
sharded.ShardedRelaxation do over the wire, done by hand.  Every rank is a sharded.HipBackend on torch's current stream, so
stream order is the barrier between the ranks and nothing here waits for the device except where a test reads a tensor.

The driver owns the ping-pong position tensors of every rank; tests read positions from them (finish() returns the best
snapshot, not the last iteration)."""
import numpy as np

from tests.test_gpu_sharded_native import _load_block
from tests.test_gpu_symmetric import _Env
from topolow_amd import _native, sharded


class SegmentRanks:
    def __init__(self, call, n, dim, P, grid=None, env=None, load=_load_block, prepare=True):
        """One HipBackend per row block of sharded.row_block(n, P, r), loaded with its block of the matrix and (load) its
        parity-rule share of the edge list; grid: TOPOLOW_SYMMETRIC_GRID; prepare = False leaves the segments unbuilt."""
        import torch
        self.torch, self.call, self.n, self.dim, self.P = torch, call, n, dim, P
        env = dict(TOPOLOW_SYMMETRIC="1", TOPOLOW_SYMMETRIC_MIN_N="0", **(env or {}))
        if grid:
            env["TOPOLOW_SYMMETRIC_GRID"] = str(grid)
        self.blocks = [sharded.row_block(n, P, r)[:2] for r in range(P)]
        with _Env(**env):
            self.backs = [sharded.HipBackend(n, dim, b, e, 0) for b, e in self.blocks]
        for bk in self.backs:
            load(bk.session, call)
        self.ld = self.backs[0].session.encoded_ld
        self.any_thr = False
        if prepare:
            self.prepare()

    def close(self):
        for bk in self.backs:
            bk.session.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- preparation: HipBackend.symm_prepare without the collectives ----
    def rows(self, first, end):
        """Rows [first, end) of the matrix, gathered row range by row range from the owners' blocks."""
        torch = self.torch
        stage = torch.empty((end - first, self.ld), dtype=torch.int32, device=self.backs[0].device)
        for (b, e), bk in zip(self.blocks, self.backs):
            lo, hi = max(first, b), min(end, e)
            if hi > lo:
                enc = sharded._as_tensor(torch, bk.session.encoded_ptr, (e - b, self.ld), torch.int32, bk.device)
                stage[lo - first:hi - first] = enc[lo - b:hi - b]
        return stage

    def build(self, r, first=None, end=None, n_segments=None):
        """Rank r's segment from the rows [first, end) (default: its window, _native.symm_segment_rows)."""
        bk = self.backs[r]
        if first is None:
            first, end = _native.symm_segment_rows(self.n, r, self.P)
        stage = self.rows(first, end)
        bk.symm_ready = False
        bk.session.symm_segment_build(r, n_segments or self.P, stage.data_ptr(), first, end - first, self.any_thr)
        bk._moves = sharded._as_tensor(self.torch, bk.session.symm_moves_ptr, (self.n * self.dim,), self.torch.float32,
                                       bk.device)
        bk.symm_ready = True

    def prepare(self):
        torch = self.torch
        # degree terms: every rank contributes its own rows, zeros elsewhere; the sum goes to every rank
        terms = [sharded._as_tensor(torch, bk.session.degree_terms_ptr, (self.n,), torch.float32, bk.device)
                 for bk in self.backs]
        full = torch.zeros(self.n, dtype=torch.float32, device=self.backs[0].device)
        for (b, e), g in zip(self.blocks, terms):
            mine = torch.zeros_like(full)
            mine[b:e] = g[b:e]
            full += mine
        for g in terms:
            g.copy_(full)
        self.any_thr = any(bk.session.has_thresholds for bk in self.backs)
        for r in range(self.P):
            self.build(r)

    # ---- a run: ShardedRelaxation's one-stage iterations without the collectives ----
    def begin(self, n_iter, k0, cooling, c_rep, eps=1e-12, window=10 ** 9, freq=3, seed=5):
        init = self.call.initial_positions
        self.pos = [[bk.to_device(init, 0), bk.new_positions(0)] for bk in self.backs]
        for bk in self.backs:
            bk.begin(init, n_iter, k0, cooling, c_rep, eps, window, freq, seed)
        self.total = self.torch.zeros(2, dtype=self.torch.float64, device=self.backs[0].device)
        self.n_iter, self.k, self.cooling, self.freq = n_iter, k0, cooling, freq
        self.it = self.cur = 0
        self.pending = None            # (iter1, k_after, buffer): a check that rides on the next sweep
        self.checks = []               # (iter1, fused, [P][2] device tensor: every rank's (sum, count))

    def _check(self, iter1, k_after, buf, shares=None):
        """The check of pos[.][buf]: the ranks' shares (None: a separate pass each) summed, the total to every controller."""
        fused = shares is not None
        if not fused:
            shares = [bk.check_partial(self.pos[r][buf]).clone() for r, bk in enumerate(self.backs)]
        shares = self.torch.stack(shares)
        self.total.copy_(shares.sum(0))
        for r, bk in enumerate(self.backs):
            bk.controller_step(self.total, self.pos[r][buf], iter1, k_after)
        self.checks.append((iter1, fused, shares))

    def iteration(self, pending=None):
        """One iteration from pos[.][cur] into the other buffer; pending: a check to reduce in the sweeps."""
        it, k, cur = self.it, self.k, self.cur
        outs = [bk.symm_sweep(self.pos[r][cur], it, k, pending is not None) for r, bk in enumerate(self.backs)]
        moves = [m for m, _ in outs]
        total = moves[0].clone()
        for m in moves[1:]:
            total += m
        for m in moves:
            m.copy_(total)
        if pending is not None:
            self._check(*pending, shares=[t.clone() for _, t in outs])
        for r, bk in enumerate(self.backs):
            bk.symm_apply(self.pos[r][cur], self.pos[r][cur ^ 1], moves[r], it)
        self.cur ^= 1
        self.k = k * (1.0 - self.cooling)
        self.it = it + 1

    def advance(self, iters, fuse=True):
        """The next `iters` iterations with the run's checks: fused into the next sweep, the last one (or fuse = False)
        a separate pass."""
        for _ in range(iters):
            pending, self.pending = self.pending, None
            self.iteration(pending)
            if self.it % self.freq == 0 or self.it == self.n_iter:
                check = (self.it, self.k, self.cur)
                if fuse and self.it < self.n_iter:
                    self.pending = check
                else:
                    self._check(*check)

    def positions(self, r, buf=None):
        buf = self.cur if buf is None else buf
        return self.pos[r][buf][: self.n].cpu().numpy().astype(np.float64)

    def moves(self, r):
        return self.backs[r]._moves.cpu().numpy().copy()

    def check_totals(self):
        """[(iter1, fused, shares[P][2])] of the checks so far, on the host."""
        return [(i, f, sh.cpu().numpy()) for i, f, sh in self.checks]
