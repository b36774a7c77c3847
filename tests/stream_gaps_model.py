"""The numpy statement of skip mode on streams (include/seqik_stream_gaps.h) that tests/test_stream_gaps.py compares the
library with -- the seed state, the state a chain carries out of a slab, named gap patterns -- and the ctypes front end
of tests/harness/stream_gaps_harness.hip."""
import ctypes
import os

import numpy as np

from conftest import ROOT, LegParamsC
from harness_build import build_harness, find_hipcc

SEQ_SEED_INDEX = [1, 2, 7, 8, 15, 16, 25]     # kSeedOffset[s] + kFirstActive[s] + j: every stage's active links
GENERIC_LINK_DOF = [2, 0, 1, 3, 4, 5, 6]      # kGenericLinkDof: link i of the generic chain carries this DOF


def np_seed_state(seeds, generic=False):
    """(7,) joint angles in DOF order: the init_angles that are bit-equivalent to none."""
    seeds = np.asarray(seeds, dtype=np.float64)
    if not generic:
        return seeds[SEQ_SEED_INDEX].copy()
    state = np.empty(7)
    for i, dof in enumerate(GENERIC_LINK_DOF):
        state[dof] = seeds[19 + i]
    return state


def np_next_state(angles, state):
    """One chain: expanded angles (N, 7) of a slab (NaN rows = missing) and the state it started from -> the state the
    next slab starts from: the last non-NaN row, or `state` unchanged."""
    ok = np.flatnonzero(~np.isnan(angles).any(axis=-1))
    return angles[ok[-1]].copy() if ok.size else np.array(state, dtype=np.float64, copy=True)


def np_next_state_batch(angles, state):
    """np_next_state over (..., N, 7) / (..., 7)."""
    out = np.array(state, dtype=np.float64, copy=True)
    for idx in np.ndindex(angles.shape[:-2]):
        out[idx] = np_next_state(angles[idx], state[idx])
    return out


def mark(pose, mask, rng, rows=(0, 1, 2, 3, 4), values=(np.nan,)):
    """A copy of pose (N, 5, 3) in which exactly the frames of `mask` (N,) bool hold one of `values` in a random
    coordinate of one of `rows`."""
    p = np.array(pose, dtype=np.float64, order="C", copy=True)
    rows = list(rows)
    for t in np.flatnonzero(mask):
        p[t, rows[rng.integers(0, len(rows))], rng.integers(0, 3)] = values[rng.integers(0, len(values))]
    return p


def frames(n, *spans):
    """(n,) bool, True on every frame of the given (first, end) spans / single frames."""
    m = np.zeros(n, bool)
    for s in spans:
        if isinstance(s, tuple):
            m[s[0]:s[1]] = True
        else:
            m[s] = True
    return m


class StreamGapsHarness:
    def __init__(self, so):
        self.lib = ctypes.CDLL(so)
        dp = ctypes.POINTER(ctypes.c_double)
        self.lib.harness_carry_slot.restype = ctypes.c_int64
        self.lib.harness_carry_slot.argtypes = [ctypes.c_int64]
        self.lib.harness_carry_chain.restype = None
        self.lib.harness_carry_chain.argtypes = [dp, ctypes.c_int64, dp]
        self.lib.harness_seed_state.restype = None
        self.lib.harness_seed_state.argtypes = [ctypes.POINTER(LegParamsC), ctypes.c_int32, dp]

    def carry_slot(self, n_valid):
        return int(self.lib.harness_carry_slot(int(n_valid)))

    def carry(self, cangles, n_valid, state):
        """The state after a slab whose solved compact angles are `cangles` (N, 7); `state` is not modified."""
        dp = ctypes.POINTER(ctypes.c_double)
        cangles = np.ascontiguousarray(cangles, dtype=np.float64)
        out = np.array(state, dtype=np.float64, order="C", copy=True)
        self.lib.harness_carry_chain(cangles.ctypes.data_as(dp), int(n_valid), out.ctypes.data_as(dp))
        return out

    def seed_state(self, seeds, generic=False):
        lp = LegParamsC()
        for i in range(27):
            lp.seeds[i] = float(seeds[i])
        out = np.full(7, np.nan)
        self.lib.harness_seed_state(ctypes.byref(lp), 1 if generic else 0, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        return out


def load_stream_gaps_harness():
    """Builds tests/harness/stream_gaps_harness.hip for the host if stale; None when there is no hipcc."""
    if find_hipcc() is None:
        return None
    return StreamGapsHarness(build_harness(os.path.join(ROOT, "tests", "harness", "stream_gaps_harness.hip")))
