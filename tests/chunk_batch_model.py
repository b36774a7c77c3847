"""TEST INFRASTRUCTURE -- the frame-chunk model of tests/chunk_model.py (``ChunkedChain.speculate()`` + ``settle()``) for ALL
chains of a call at once, with the solver plugged in: the same sequence of solves (speculative pass, first verification
with the per-chain guard, ``rounds`` x {scan, repair}, sweep, serial walk of the guarded chains), every batch of solves
handed to a callable

    solve(pose[B, T, 5, 3], leg_index[B], init[B, 7] or None) -> angles[B, T, 7], fk[B, T, 9, 3]

(``init`` None = from the seeds of the leg).  Chunks of equal length go in one batch; the first chunk of a chain (no
run-in) and a ragged last chunk get batches of their own; the sweep runs left to right, one batch per step over the
chains whose chunk at that step is inconsistent.  With the C oracle as ``solve`` it must equal ``ChunkedChain`` chain by
chain (tests/test_chunk_batch_model.py); with the library's plain serial call it is the yardstick of the device-side
control path at sizes the oracle cannot follow (tests/test_chunk_control.py)."""
import numpy as np

from chunk_model import FAILED_FIRST, REPAIRED, SERIAL, SWEPT


def oracle_solver(oracle, legs):
    """``solve`` on the C oracle; legs: one (seg, bounds, seeds) per leg index."""
    def solve(pose, leg_index, init):
        ang, fk = np.empty(pose.shape[:2] + (7,)), np.empty(pose.shape[:2] + (9, 3))
        for b in range(pose.shape[0]):
            r = oracle.seq_leg(pose[b], *legs[int(leg_index[b])], init=None if init is None else np.array(init[b], dtype=np.float64))
            ang[b], fk[b] = r["angles"], r["fk"]
        return ang, fk
    return solve


class Replay:
    """pose (n, N, 5, 3): the n chains of a call in the library's chain order (sequence-major, legs inside); leg_index (n,);
    init (n, 7) or None.  Options as ``ChunkedChain``.  ``run()`` fills

        angles (n, N, 7), fk (n, N, 9, 3), chunk_states (n, K, 7), chunk_flags (n, K) uint8, stats (n, 16) int32 per chain,
        failed_first (n, K) bool, listed [round] -> (n, K) bool, pending_at_sweep (n, K) bool, swept (n, K) bool,
        serial (n,) bool, solved_frames (n,) -- frames solved for each chain, run-ins and the serial walk included."""

    def __init__(self, solve, pose, leg_index, chunk, halo, tol=1e-6, rounds=3, init=None, guard=False, lead=0):
        self.solve, self.pose, self.leg = solve, np.asarray(pose, dtype=np.float64), np.asarray(leg_index, dtype=np.int64)
        self.n, self.N = self.pose.shape[:2]
        self.C, self.h, self.lead = int(chunk), int(halo), int(lead)
        self.K = -(-(self.N - self.lead) // self.C)
        self.tol, self.rounds, self.guard = tol, int(rounds), bool(guard) and lead == 0
        self.init = None if init is None else np.asarray(init, dtype=np.float64)
        self.k_first = 0 if (self.lead > 0 and self.init is not None) else 1
        n, N, K = self.n, self.N, self.K
        self.angles, self.fk = np.zeros((n, N, 7)), np.zeros((n, N, 9, 3))
        self.chunk_states = np.zeros((n, K, 7))
        self.chunk_flags = np.zeros((n, K), np.uint8)
        self.stats = np.zeros((n, 16), np.int32)
        self.serial = np.zeros(n, bool)
        self.solved_frames = np.zeros(n, np.int64)
        self.listed = []
        self.failed_first = self.pending_at_sweep = self.swept = np.zeros((n, K), bool)

    def span(self, k):
        return self.lead + k * self.C, min(self.lead + (k + 1) * self.C, self.N)

    def _store(self, chains, k, ang, fk, off):
        a, b = self.span(k)
        self.angles[chains, a:b] = ang[:, off:]
        self.fk[chains, a:b] = fk[:, off:]
        self.solved_frames[chains] += ang.shape[1]

    def speculate(self):
        every = np.arange(self.n)
        groups = {}            # chunks whose solve has the same shape: (frames in front of the chunk, frames stored, first chunk?)
        for k in range(self.K):
            a, b = self.span(k)
            t0 = a - self.h if (k > 0 and a > self.h) else 0
            groups.setdefault((a - t0, b - a, k == 0), []).append((k, t0, b))
        for (off, _, first), members in groups.items():
            run_in = not first or self.lead > 0
            pose = np.concatenate([self.pose[:, t0:b] for _, t0, b in members])
            init = None if (run_in or self.init is None) else np.tile(self.init, (len(members), 1))
            ang, fk = self.solve(pose, np.tile(self.leg, len(members)), init)
            for j, (k, _, _) in enumerate(members):
                part = slice(j * self.n, (j + 1) * self.n)
                if run_in:
                    self.chunk_states[:, k] = ang[part, off - 1]
                self._store(every, k, ang[part], fk[part], off)
        return self

    def inconsistent(self):
        """(n, K) bool: the warm start a chunk was solved from is not within tol of the stored frame in front of it (chunk 0:
        of ``init``); never below k_first, NaN counts as a mismatch."""
        truth = np.zeros((self.n, self.K, 7))
        ks = np.arange(1, self.K)
        truth[:, 1:] = self.angles[:, self.lead + ks * self.C - 1]
        if self.init is not None:
            truth[:, 0] = self.init
        inc = ~np.all(np.abs(self.chunk_states - truth) <= self.tol, axis=-1)
        inc[:, :self.k_first] = False
        return inc

    def _repair(self, mask, flag):
        """Re-solves the chunks of ``mask`` (n, K) from the true state in front of them; no two of them are adjacent in a chain, or
        the caller goes column by column."""
        by_len = {}
        for k in np.flatnonzero(mask.any(0)):
            a, b = self.span(k)
            by_len.setdefault((b - a, k == 0), []).append(int(k))
        for ks in by_len.values():
            chains = np.concatenate([np.flatnonzero(mask[:, k]) for k in ks])
            which = np.concatenate([np.full(int(mask[:, k].sum()), k) for k in ks])
            a = self.lead + which * self.C
            length = self.span(ks[0])[1] - self.span(ks[0])[0]
            start = self.init[chains] if ks[0] == 0 else self.angles[chains, a - 1]
            self.chunk_states[chains, which] = start
            pose = self.pose[chains[:, None], a[:, None] + np.arange(length)[None]]
            ang, fk = self.solve(pose, self.leg[chains], start.copy())
            for k in ks:
                sel = which == k
                self._store(chains[sel], k, ang[sel], fk[sel], 0)
            self.chunk_flags[chains, which] |= flag

    def settle(self):
        K = self.K
        self.stats[:] = 0
        self.stats[:, :3] = (K, self.C, self.h)
        self.failed_first = self.inconsistent()
        self.chunk_flags[:] = np.where(self.failed_first, FAILED_FIRST, 0)
        fails = self.failed_first.sum(1)
        self.stats[:, 7] = fails
        if self.guard:
            self.serial = fails * 8 > K
            s = np.flatnonzero(self.serial)
            if s.size:
                self.chunk_flags[s] |= SERIAL
                self.stats[s, 8], self.stats[s, 9] = 1, K
        live = ~self.serial
        self.listed = []
        self.pending_at_sweep = self.swept = np.zeros((self.n, K), bool)
        for r in range(self.rounds + 1):
            inc = self.inconsistent() & live[:, None]
            if not inc.any():
                break
            if r < self.rounds:
                ready = inc.copy()
                ready[:, self.k_first + 1:] &= ~inc[:, self.k_first:-1]
                self.listed.append(ready)
                self.stats[:, 3 + min(r, 2)] += ready.sum(1)
                self._repair(ready, REPAIRED)
            else:
                self.pending_at_sweep = inc
                self.swept = np.zeros((self.n, K), bool)
                for k in range(self.k_first, K):
                    col = np.zeros((self.n, K), bool)
                    col[:, k] = self.inconsistent()[:, k] & live
                    if col.any():
                        self._repair(col, SWEPT)
                        self.swept |= col
                self.stats[:, 6] = self.swept.sum(1)
        s = np.flatnonzero(self.serial)
        if s.size:       # the guard's serial walk (the library runs it last; the scans leave these chains alone)
            ang, fk = self.solve(self.pose[s], self.leg[s], None if self.init is None else self.init[s].copy())
            self.angles[s], self.fk[s] = ang, fk
            self.solved_frames[s] += self.N
        return self

    def run(self):
        return self.speculate().settle()

    def total_stats(self):
        """The ten fields of ``SeqikOptions.chunk_stats`` for the whole call."""
        t = self.stats.sum(0)[:10].astype(np.int64)
        t[1:3] = (self.C, self.h)
        return t

    def counts(self):
        """What EXPERIMENTS.md records per case."""
        return dict(chunks=self.n * self.K, failed_first=int(self.failed_first.sum()), listed=[int(m.sum()) for m in self.listed],
                    pending_at_sweep=int(self.pending_at_sweep.sum()), swept=int(self.swept.sum()), serial=int(self.serial.sum()))
