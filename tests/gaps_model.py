"""The numpy statement of skip mode (include/seqik_gaps.h) that the tests compare the library with, the tile geometry of
its kernels, named gap patterns and poisoned inputs for the geometry tests, and the ctypes front end of
tests/harness/gaps_harness.hip.  Shared by tests/test_missing_key_points.py and tests/test_gaps_geometry.py."""
import ctypes
import os

import numpy as np

from conftest import ROOT, LegParamsC
from harness_build import build_harness, find_hipcc

MISSING = -100


def _lp(seg):
    lp = LegParamsC()
    for i in range(4):
        lp.seg[i] = float(seg[i])
    return lp


def rows_read(kind, affine):
    rows = [0, 1, 2, 3, 4] if kind == "seq" else [0, 4]
    return [r for r in rows if not (affine and r == 0)]


def np_missing(pose, kind="seq", affine=False):
    """(..., N) bool: a key point the solver reads holds a non-finite coordinate."""
    return ~np.isfinite(pose[..., rows_read(kind, affine), :]).all(axis=(-1, -2))


def np_compact(pose, seg, kind="seq", affine=False):
    """The compacted and padded recording of one chain (N, 5, 3), its map and n_valid, built with numpy."""
    miss = np_missing(pose, kind, affine)
    keep = np.flatnonzero(~miss)
    n = pose.shape[0]
    if keep.size:
        cpose = np.concatenate([pose[keep], np.repeat(pose[keep[-1]][None], n - keep.size, axis=0)])
    else:
        z = -np.concatenate([[0.0], np.cumsum(np.asarray(seg, dtype=np.float64))])
        filler = np.zeros((5, 3))
        filler[:, 2] = z
        cpose = np.repeat(filler[None], n, axis=0)
    mp = np.full(n, -1, np.int32)
    mp[keep] = np.arange(keep.size, dtype=np.int32)
    return cpose, mp, keep.size


def np_expand(mp, compact, fill):
    out = np.empty_like(compact)
    out[...] = fill
    out[mp >= 0] = compact[mp[mp >= 0]]
    return out


def inject_gaps(pose, rng, frac=0.05, blocks=((10, 60),), rows=(0, 1, 2, 3, 4), values=(np.nan,)):
    """A copy of pose (N, 5, 3) with about `frac` random leg-frames and the given frame blocks made non-finite."""
    p = np.array(pose, dtype=np.float64, copy=True)
    n = p.shape[0]
    hit = rng.random(n) < frac
    for a, b in blocks:
        hit[a:min(b, n)] = True
    for t in np.flatnonzero(hit):
        p[t, rng.choice(list(rows)), rng.integers(0, 3)] = values[rng.integers(0, len(values))]
    return p


def np_compact_batch(pose, seg, kind="seq", affine=False):
    """np_compact over every chain of a batch (..., N, 5, 3) whose legs share one `seg`, without a Python loop: a stable
    argsort of the mask is the stable partition.  Returns cpose, map (..., N) and n_valid (...)."""
    miss = np_missing(pose, kind, affine)
    n = pose.shape[-3]
    order = np.argsort(miss, axis=-1, kind="stable")          # the non-missing frames in order, then the missing ones
    nv = (~miss).sum(axis=-1)
    cpose = np.take_along_axis(pose, order[..., None, None], axis=-3)
    last = np.take_along_axis(cpose, np.maximum(nv - 1, 0)[..., None, None, None], axis=-3)
    filler = np.zeros((5, 3))
    filler[:, 2] = -np.concatenate([[0.0], np.cumsum(np.asarray(seg, dtype=np.float64))])
    last = np.where((nv > 0)[..., None, None, None], last, filler)
    pad = np.arange(n) >= nv[..., None]
    cpose = np.where(pad[..., None, None], last, cpose)
    mp = np.where(miss, -1, np.cumsum(~miss, axis=-1) - 1).astype(np.int32)
    return cpose, mp, nv.astype(np.int32)


def np_expand_batch(mp, compact, fill):
    """np_expand over a batch: mp (..., N), compact (..., N, W...)."""
    idx = np.maximum(mp, 0).reshape(mp.shape + (1,) * (compact.ndim - mp.ndim))
    got = np.take_along_axis(compact, idx, axis=mp.ndim - 1)
    return np.where((mp >= 0).reshape(idx.shape), got, np.asarray(fill, dtype=compact.dtype))


def bits(a):
    """The array as unsigned integers of its item size: equality of these counts NaN payloads and signed zeros."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------------
# tile geometry (the header comment of csrc/seqik_gaps.hip)
# ---------------------------------------------------------------------------------------------------------------------

MAX_TILES = 1024      # tiles per chain: the scan holds them in 16 rows of 64 lanes
PAD_BLOCK = 256       # slots per workgroup of the pad kernel


def tile_geometry(N):
    """One wavefront per tile of 64 k frames; k = 1 up to 65 536 frames, else the smallest k that keeps a chain at
    <= 1024 tiles.  Works on an int or an integer array."""
    N = np.asarray(N, dtype=np.int64)
    blocks64 = -(-N // 64)
    k = np.maximum(1, -(-blocks64 // MAX_TILES))
    tile = 64 * k
    tiles = -(-N // tile)
    last_frames = N - (tiles - 1) * tile                # frames of the last tile
    last_tile_blocks = -(-last_frames // 64)            # its 64-frame blocks, the last one maybe partial
    last_block_frames = last_frames - (last_tile_blocks - 1) * 64
    g = dict(k=k, tile=tile, tiles=tiles, last_tile_blocks=last_tile_blocks, last_block_frames=last_block_frames)
    return {name: (int(v) if v.ndim == 0 else v) for name, v in g.items()}


# ---------------------------------------------------------------------------------------------------------------------
# named gap patterns and poisoned input
# ---------------------------------------------------------------------------------------------------------------------

PATTERNS = ["none", "all", "only_first_valid", "only_last_valid", "first_missing", "alternating", "lane0_only",
            "lane63_only", "empty_tiles", "gap_across_tile_boundary", "tail_gap", "random_half", "random_sparse"]
TAIL_GAP = 2 * PAD_BLOCK + 37      # frames of the closing gap of `tail_gap` (one more where n_valid would hit a block edge)


def pattern(name, N, tile, rng):
    """(N,) bool, True = the frame is missing."""
    t = np.arange(N)
    if name == "none":
        return np.zeros(N, bool)
    if name == "all":
        return np.ones(N, bool)
    if name == "only_first_valid":
        return t != 0
    if name == "only_last_valid":
        return t != N - 1
    if name == "first_missing":
        return t == 0
    if name == "alternating":
        return t % 2 == 1
    if name == "lane0_only":
        return t % 64 != 0
    if name == "lane63_only":
        return t % 64 != 63
    if name == "empty_tiles":
        return (t // tile) % 3 == 1
    if name == "gap_across_tile_boundary":
        miss = np.zeros(N, bool)
        for b in range(tile, N, tile):
            miss[b - 3:b + 3] = True
        return miss
    if name == "tail_gap":
        if N < 4 * PAD_BLOCK:
            return t >= N // 2
        gap = TAIL_GAP + ((N - TAIL_GAP) % PAD_BLOCK == 0)
        return t >= N - gap
    if name == "random_half":
        return rng.random(N) < 0.5
    if name == "random_sparse":
        return rng.random(N) < 0.05
    raise ValueError(name)


def _u64(*words):
    return np.array(words, dtype=np.uint64)


DBL_MAX_BITS, DENORM_MIN_BITS, NEG_ZERO_BITS = 0x7FEFFFFFFFFFFFFF, 0x0000000000000001, 0x8000000000000000
#: finite values that must not mark a frame, wherever they stand: +-DBL_MAX, the smallest denormal, -0.0
HARMLESS = _u64(DBL_MAX_BITS, DBL_MAX_BITS | NEG_ZERO_BITS, DENORM_MIN_BITS, NEG_ZERO_BITS)
#: NaNs whose payload is not the default one (quiet, quiet and negative, signalling)
PAYLOAD_NANS = _u64(0x7FF80000DEADBEEF, 0xFFF8123456789ABC, 0x7FF0000000000001)
#: what marks a frame in a read row, and must travel untouched in an unread one
NON_FINITE = np.concatenate([bits(np.array([np.nan, np.inf, -np.inf])), PAYLOAD_NANS])


def poison(pose, mask, rows, rng, frac=0.1):
    """A copy of pose (N, 5, 3) in which exactly the frames of `mask` are missing for a solver that reads `rows`: each
    gets one of NON_FINITE in a random coordinate of a read row.  About `frac` of all frames also get a HARMLESS value in
    any row, and about `frac` one of NON_FINITE in a row the solver does not read (if there is one)."""
    p = np.array(pose, dtype=np.float64, order="C", copy=True)
    u = p.view(np.uint64)
    n = p.shape[0]
    rows = np.asarray(sorted(rows))
    unread = np.setdiff1d(np.arange(5), rows)

    def put(frames, in_rows, values):
        k = frames.size
        u[frames, in_rows[rng.integers(0, in_rows.size, k)], rng.integers(0, 3, k)] = values[rng.integers(0, values.size, k)]

    put(np.flatnonzero(rng.random(n) < frac), np.arange(5), HARMLESS)
    if unread.size:
        put(np.flatnonzero(rng.random(n) < frac), unread, NON_FINITE)
    put(np.flatnonzero(mask), rows, NON_FINITE)   # last: nothing above overwrites a mark
    return p


# ---------------------------------------------------------------------------------------------------------------------
# the host harness
# ---------------------------------------------------------------------------------------------------------------------

class GapsHarness:
    def __init__(self, so):
        self.lib = ctypes.CDLL(so)
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        lp = ctypes.POINTER(ctypes.c_int64)
        self.lib.harness_gaps_compact.restype = ctypes.c_int64
        self.lib.harness_gaps_compact.argtypes = [dp, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(LegParamsC), dp, ip]
        self.lib.harness_gaps_expand_f64.restype = None
        self.lib.harness_gaps_expand_f64.argtypes = [ip, ctypes.c_int64, dp, ctypes.c_int32, dp]
        self.lib.harness_gaps_expand_i32.restype = None
        self.lib.harness_gaps_expand_i32.argtypes = [ip, ctypes.c_int64, ip, ctypes.c_int32, ctypes.c_int32, ip]
        self.lib.harness_tile_geometry.restype = None
        self.lib.harness_tile_geometry.argtypes = [ctypes.c_int64, ctypes.c_int64, lp, lp]

    def compact(self, pose, seg, kind="seq", affine=False):
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        pose = np.ascontiguousarray(pose, dtype=np.float64)
        n = pose.shape[0]
        cpose = np.full_like(pose, 12345.0)
        mp = np.full(n, 777, np.int32)
        flags = (1 if kind == "generic" else 0) | (2 if affine else 0)
        nv = self.lib.harness_gaps_compact(pose.ctypes.data_as(dp), n, flags, ctypes.byref(_lp(seg)),
                                           cpose.ctypes.data_as(dp), mp.ctypes.data_as(ip))
        return cpose, mp, int(nv)

    def expand(self, mp, compact, fill=None):
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        mp = np.ascontiguousarray(mp, dtype=np.int32)
        n = mp.shape[0]
        compact = np.ascontiguousarray(compact)
        width = int(np.prod(compact.shape[1:])) if compact.ndim > 1 else 1
        out = np.empty_like(compact)
        if compact.dtype == np.float64:
            self.lib.harness_gaps_expand_f64(mp.ctypes.data_as(ip), n, compact.ctypes.data_as(dp), width,
                                             out.ctypes.data_as(dp))
        else:
            self.lib.harness_gaps_expand_i32(mp.ctypes.data_as(ip), n, compact.ctypes.data_as(ip), width, int(fill),
                                             out.ctypes.data_as(ip))
        return out

    def tile_geometry(self, n_first, n_last):
        """The library's seqik::tile_geometry for every n_frames in n_first..n_last -> (tile, tiles) int64 arrays."""
        lp = ctypes.POINTER(ctypes.c_int64)
        tile = np.zeros(n_last - n_first + 1, np.int64)
        tiles = np.zeros_like(tile)
        self.lib.harness_tile_geometry(n_first, n_last, tile.ctypes.data_as(lp), tiles.ctypes.data_as(lp))
        return tile, tiles


def load_gaps_harness():
    """Builds tests/harness/gaps_harness.hip for the host if stale; None when there is no hipcc."""
    if find_hipcc() is None:
        return None
    return GapsHarness(build_harness(os.path.join(ROOT, "tests", "harness", "gaps_harness.hip")))
