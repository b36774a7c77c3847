"""Skip mode at every edge of its tile geometry (csrc/seqik_gaps.hip): compaction and expansion against the
numpy construction of tests/gaps_model.py, bit for bit.

CPU tier: the recording lengths and gap patterns have the properties they are named for, the library's tile geometry
equals its Python statement for every length up to 140 000, the host restatement of the contract equals numpy on
poisoned input.  GPU tier (`-m gpu`): the kernels at one tile / many tiles, full and partial 64-frame blocks, full scan
rows and the first carry, k = 1, 2, 3, every gap pattern, every chain kind, per-leg fillers, every subset of the optional
outputs of the expansion.  Every device buffer is carved out of a larger one filled with a sentinel, with one record of
guard in front of and behind the call's extent; every chain of every sequence is compared and every guard checked."""
import itertools

import numpy as np
import pytest

from gaps_model import (MISSING, NON_FINITE, PAD_BLOCK, PATTERNS, bits, load_gaps_harness, np_compact,
                        np_compact_batch, np_expand, np_expand_batch, np_missing, pattern, poison, rows_read, same_bits,
                        tile_geometry)

# N -> (k, tiles per chain, 64-frame blocks of the last tile, frames of the last block): what each length is there for
SIZES = {
    1: (1, 1, 1, 1), 2: (1, 1, 1, 2), 63: (1, 1, 1, 63),        # one partial block
    64: (1, 1, 1, 64),                                           # exactly one block
    65: (1, 2, 1, 1),                                            # a one-frame second tile: the scan runs
    127: (1, 2, 1, 63), 128: (1, 2, 1, 64), 129: (1, 3, 1, 1),
    4096: (1, 64, 1, 64),                                        # scan row 0 exactly full
    4097: (1, 65, 1, 1),                                         # the first carry
    65535: (1, 1024, 1, 63), 65536: (1, 1024, 1, 64),            # every scan row full
    65537: (2, 513, 1, 1),                                       # k = 2, the last tile is one frame
    65600: (2, 513, 1, 64),                                      # ... one full block
    65601: (2, 513, 2, 1),                                       # ... a full block and a one-frame block
    131072: (2, 1024, 2, 64),
    131073: (3, 683, 3, 1),                                      # k = 3, the last tile is 64 + 64 + 1 frames
}
N_ALL = list(SIZES)
COMBOS = [("seq", False), ("seq", True), ("generic", False), ("generic", True)]
ROTATING = [p for p in PATTERNS if p not in ("random_half", "tail_gap")]


def compaction_patterns(N):
    """The six chains of the compaction test: random_half, tail_gap and four of the others, rotating with N."""
    i = N_ALL.index(N)
    return ["random_half", "tail_gap"] + [ROTATING[(4 * i + j) % len(ROTATING)] for j in range(4)]


def expansion_patterns(N, n_chains):
    return [PATTERNS[N_ALL.index(N) % len(PATTERNS)], "random_half"][-n_chains:]


def segs_of(L):
    return [np.array([0.4 + 0.01 * l, 0.6 + 0.02 * l, 0.5 + 0.03 * l, 0.3 + 0.04 * l]) for l in range(L)]


def gapped_batch(S, L, N, names, kind, affine, seed):
    """pose (S, L, N, 5, 3) whose chain c carries the pattern names[c], poisoned for (kind, affine), and the masks."""
    rng = np.random.default_rng(seed)
    tile = tile_geometry(N)["tile"]
    pose = rng.normal(size=(S, L, N, 5, 3))
    masks = np.zeros((S, L, N), bool)
    for c, name in enumerate(names):
        s, l = divmod(c, L)
        masks[s, l] = pattern(name, N, tile, rng)
        pose[s, l] = poison(pose[s, l], masks[s, l], rows_read(kind, affine), rng)
    return pose, masks


@pytest.fixture(scope="module")
def gaps_harness():
    h = load_gaps_harness()
    if h is None:
        pytest.skip("hipcc not available")
    return h


# ---------------------------------------------------------------------------------------------------------------------
# CPU tier
# ---------------------------------------------------------------------------------------------------------------------

def test_every_size_has_the_geometry_it_is_named_for():
    for N, (k, tiles, last_blocks, last_frames) in SIZES.items():
        g = tile_geometry(N)
        assert (g["k"], g["tiles"], g["last_tile_blocks"], g["last_block_frames"]) == (k, tiles, last_blocks, last_frames), N
        assert g["tile"] == 64 * k and (tiles - 1) * g["tile"] < N <= tiles * g["tile"] and tiles <= 1024, N
    tiles = {N: v[1] for N, v in SIZES.items()}
    assert tiles[64] == 1 and tiles[65] == 2                      # the scan kernel starts to run
    assert tiles[4096] == 64 and tiles[4097] == 65                # scan row 0 full / the first carry
    assert tiles[65536] == 1024 and SIZES[65537][0] == 2          # the last k = 1 length and the first k = 2 one
    assert SIZES[131072][:2] == (2, 1024) and SIZES[131073][0] == 3
    # a multi-block last tile with a partial block, which needs k > 1
    assert any(k > 1 and lb > 1 and lf < 64 for k, _, lb, lf in SIZES.values())
    # the rotation of the compaction test brings every pattern to one tile, many tiles with k = 1, and k > 1
    for regime in (lambda k, t: t == 1, lambda k, t: k == 1 and t > 1, lambda k, t: k > 1):
        seen = set()
        for N, (k, t, _, _) in SIZES.items():
            if regime(k, t):
                seen |= set(compaction_patterns(N))
        assert seen == set(PATTERNS)
    assert {expansion_patterns(N, 2)[0] for N in N_ALL if N <= 65601} == set(PATTERNS)


@pytest.mark.parametrize("name", PATTERNS)
def test_every_pattern_has_the_property_it_is_named_for(name):
    for N in N_ALL:
        g = tile_geometry(N)
        tile, tiles = g["tile"], g["tiles"]
        miss = pattern(name, N, tile, np.random.default_rng(N))
        assert miss.shape == (N,) and miss.dtype == bool
        valid = np.flatnonzero(~miss)
        padded = np.zeros(tiles * tile, bool)
        padded[:N] = ~miss
        per_tile = padded.reshape(tiles, tile).sum(axis=1)
        full = N // 64
        per_block = padded[:-(-N // 64) * 64].reshape(-1, 64).sum(axis=1)
        if name == "none":
            assert valid.size == N
        elif name == "all":
            assert valid.size == 0
        elif name == "only_first_valid":
            assert valid.tolist() == [0]
        elif name == "only_last_valid":
            assert valid.tolist() == [N - 1]
        elif name == "first_missing":
            assert np.flatnonzero(miss).tolist() == [0]
        elif name == "alternating":
            assert not miss[0] and (miss[1:] != miss[:-1]).all()
        elif name == "lane0_only":
            assert (per_block == 1).all() and (valid % 64 == 0).all()
        elif name == "lane63_only":
            assert (per_block[:full] == 1).all() and (per_block[full:] == 0).all() and (valid % 64 == 63).all()
        elif name == "empty_tiles":
            assert per_tile[0] > 0
            if tiles >= 3:
                empty = np.flatnonzero(per_tile == 0)
                assert ((empty > 0) & (empty < tiles - 1)).any()     # a count of 0 that is neither first nor last
            if tiles > 64:   # zeros in the middle of a scan row, in row 0 and behind the first carry
                inner = np.flatnonzero((per_tile[1:-1] == 0) & (per_tile[:-2] > 0) & (per_tile[2:] > 0)) + 1
                assert ((inner % 64 > 0) & (inner % 64 < 63) & (inner < 64)).any()
                assert ((inner % 64 > 0) & (inner % 64 < 63) & (inner >= 64)).any() or tiles < 69
        elif name == "gap_across_tile_boundary":
            edges = np.arange(tile, N, tile)
            assert miss[edges].all() and miss[edges - 1].all() and miss.sum() <= 6 * edges.size
            assert (edges.size == 0) == (not miss.any())
            if N >= 8:
                assert not miss[0]
        elif name == "tail_gap":
            n_valid = valid.size
            assert miss[n_valid:].all() and not miss[:n_valid].any()      # one gap, at the end
            if N >= 1024:
                assert N - n_valid > 2 * PAD_BLOCK and n_valid > 0
                assert n_valid % PAD_BLOCK != 0                           # n_valid strictly inside a pad block
            else:
                assert N - n_valid == N - N // 2
        elif name == "random_half":
            assert N < 4096 or 0.4 < miss.mean() < 0.6
            assert N < 63 or (miss.any() and not miss.all())
        elif name == "random_sparse":
            assert N < 4096 or 0.03 < miss.mean() < 0.07
        else:
            raise AssertionError(name)


def test_poison_marks_exactly_the_mask_and_plants_every_special_value():
    rng = np.random.default_rng(5)
    N = 4097
    base = rng.normal(size=(N, 5, 3))
    mask = rng.random(N) < 0.5
    for kind, affine in COMBOS:
        rows = rows_read(kind, affine)
        p = poison(base, mask, rows, rng)
        assert np.array_equal(np_missing(p, kind, affine), mask)
        u = bits(p)
        # every non-finite kind marks some frame; every harmless value stands in a frame that stays
        assert set(NON_FINITE.tolist()) == set(np.unique(u[mask][~np.isfinite(p[mask])]).tolist())
        kept = u[~mask]
        for word in (0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF, 0x0000000000000001, 0x8000000000000000):
            assert (kept == np.uint64(word)).any(), hex(word)
        unread = [r for r in range(5) if r not in rows]
        if unread:
            assert set(NON_FINITE.tolist()) == set(np.unique(kept[:, unread][~np.isfinite(p[~mask][:, unread])]).tolist())
        else:
            assert np.isfinite(p[~mask]).all()


def test_library_tile_geometry_equals_the_python_statement(gaps_harness):
    n = np.arange(1, 140_001)
    tile, tiles = gaps_harness.tile_geometry(1, 140_000)
    g = tile_geometry(n)
    assert np.array_equal(tile, g["tile"]) and np.array_equal(tiles, g["tiles"])
    assert tiles.max() == 1024 and set(np.unique(g["k"]).tolist()) == {1, 2, 3}
    assert ((g["tiles"] - 1) * g["tile"] < n).all() and (n <= g["tiles"] * g["tile"]).all()


def test_the_batched_numpy_construction_equals_the_per_chain_one():
    rng = np.random.default_rng(8)
    seg = [0.4, 0.6, 0.5, 0.3]
    for kind, affine in COMBOS:
        pose, _ = gapped_batch(2, 7, 300, PATTERNS + ["none"], kind, affine, seed=3)
        cp, mp, nv = np_compact_batch(pose, seg, kind, affine)
        ang = rng.normal(size=(2, 7, 300, 7))
        st = rng.integers(-1, 5, size=(2, 7, 300, 4)).astype(np.int32)
        ea, es = np_expand_batch(mp, ang, np.nan), np_expand_batch(mp, st, MISSING)
        for s, l in itertools.product(range(2), range(7)):
            rc, rm, rn = np_compact(pose[s, l], seg, kind, affine)
            assert nv[s, l] == rn and np.array_equal(mp[s, l], rm) and same_bits(cp[s, l], rc), (kind, affine, s, l)
            assert same_bits(ea[s, l], np_expand(rm, ang[s, l], np.nan)) and same_bits(es[s, l], np_expand(rm, st[s, l], MISSING))


@pytest.mark.parametrize("kind,affine", COMBOS)
@pytest.mark.parametrize("N", [N for N in N_ALL if N <= 4097])
def test_host_contract_at_every_small_size_and_pattern(gaps_harness, N, kind, affine):
    rng = np.random.default_rng(1000 + N)
    tile = tile_geometry(N)["tile"]
    seg = rng.uniform(0.2, 0.8, 4)
    base = rng.normal(size=(N, 5, 3))
    ang = bits(rng.normal(size=(N, 7))).copy()
    ang[rng.random((N, 7)) < 0.05] = NON_FINITE[3]      # payloads travel through the expansion as well
    ang = ang.view(np.float64)
    st = rng.integers(-1, 5, size=(N, 4)).astype(np.int32)
    for name in PATTERNS:
        mask = pattern(name, N, tile, rng)
        pose = poison(base, mask, rows_read(kind, affine), rng)
        cpose, mp, nv = gaps_harness.compact(pose, seg, kind, affine)
        ref_c, ref_m, ref_nv = np_compact(pose, seg, kind, affine)
        assert ref_nv == N - mask.sum() == nv, name
        assert np.array_equal(mp, ref_m), name
        assert same_bits(cpose, ref_c), name
        assert same_bits(gaps_harness.expand(mp, ang), np_expand(mp, ang, np.nan)), name
        assert same_bits(gaps_harness.expand(mp, st, MISSING), np_expand(mp, st, MISSING)), name
        width1 = np.ascontiguousarray(st[:, 0])
        assert same_bits(gaps_harness.expand(mp, width1, 0), np_expand(mp, width1, 0)), name


# ---------------------------------------------------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------------------------------------------------

F64_SENTINEL = 0x7FF4C0DEC0DEC0DE     # as bits: no kernel writes this value, and no input holds it
I32_SENTINEL = 0x5EA7BEEF


class Guarded:
    """A device buffer of `shape` carved out of a larger one filled with a sentinel, `rec` elements (one record) of guard
    on either side.  `.t` is the flat tensor to hand to the library."""

    def __init__(self, shape, dtype, rec, data=None):
        import torch
        self.shape, self.rec, self.np_dtype = tuple(shape), rec, np.dtype(dtype)
        self.words, self.sentinel = ((torch.int64, F64_SENTINEL) if self.np_dtype == np.float64
                                     else (torch.int32, I32_SENTINEL))
        n = int(np.prod(self.shape))
        self.big = torch.full((n + 2 * rec,), self.sentinel, dtype=self.words, device="cuda:0")
        self.raw = self.big[rec:rec + n]
        self.t = self.raw.view(torch.float64) if self.np_dtype == np.float64 else self.raw
        if data is not None:
            data = np.ascontiguousarray(data, dtype=self.np_dtype)
            assert data.shape == self.shape
            self.raw.copy_(torch.from_numpy(data.reshape(-1).view(np.int64 if self.np_dtype == np.float64 else np.int32)))

    def numpy(self):
        return self.raw.cpu().numpy().view(self.np_dtype).reshape(self.shape)

    def guards_intact(self):
        return bool((self.big[:self.rec] == self.sentinel).all()) and bool((self.big[-self.rec:] == self.sentinel).all())

    def untouched(self):
        return bool((self.big == self.sentinel).all())


def leg_params(hiplib, segs):
    return [hiplib.leg_params_from_arrays(seg, np.zeros((7, 2)), np.zeros(27)) for seg in segs]


def compact_on_device(hiplib, pose, segs, kind="seq", affine=False):
    """Runs the compaction on guarded buffers and compares every chain with np_compact.  Returns (cpose, map, n_valid)."""
    import torch
    S, L, N = pose.shape[:3]
    d_pose = Guarded((S, L, N, 5, 3), np.float64, 15, pose)
    d_cpose = Guarded((S, L, N, 5, 3), np.float64, 15)
    d_map = Guarded((S, L, N), np.int32, 1)
    d_nv = Guarded((S, L), np.int32, 1)
    hiplib.gaps_compact_device(d_pose.t, S, L, N, leg_params(hiplib, segs), d_cpose.t, d_map.t, d_nv.t, kind=kind,
                               affine=affine)
    torch.cuda.synchronize()
    cp, mp, nv = d_cpose.numpy(), d_map.numpy(), d_nv.numpy()
    for s, l in itertools.product(range(S), range(L)):
        rc, rm, rn = np_compact(pose[s, l], segs[l], kind, affine)
        where = (N, kind, affine, s, l)
        assert nv[s, l] == rn, where
        assert np.array_equal(mp[s, l], rm), where + (int(np.flatnonzero(mp[s, l] != rm)[0]),)
        assert same_bits(cp[s, l], rc), where + (int(np.flatnonzero((bits(cp[s, l]) != bits(rc)).any(axis=(1, 2)))[0]),)
    for name, buf in (("pose", d_pose), ("cpose", d_cpose), ("map", d_map), ("n_valid", d_nv)):
        assert buf.guards_intact(), (N, kind, affine, name)
    assert same_bits(d_pose.numpy(), pose)      # the input is read only
    return cp, mp, nv


@pytest.mark.gpu
@pytest.mark.parametrize("N", N_ALL)
def test_compaction_at_every_geometry_edge(hiplib, N):
    S, L = 2, 3        # six chains on workgroups of four wavefronts: workgroups straddle chains
    names = compaction_patterns(N)
    pose, masks = gapped_batch(S, L, N, names, "seq", False, seed=N)
    cp, mp, nv = compact_on_device(hiplib, pose, segs_of(L))
    assert np.array_equal(nv, (~masks).sum(axis=-1)) and np.array_equal(mp < 0, masks)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [65, 4097, 65601])
def test_kinds_and_fused_alignment_on_device(hiplib, N):
    S, L = 2, 3
    names = ["random_half", "random_sparse", "tail_gap", "alternating", "gap_across_tile_boundary", "none"]
    for kind, affine in COMBOS:
        pose, masks = gapped_batch(S, L, N, names, kind, affine, seed=7 * N)
        cp, mp, nv = compact_on_device(hiplib, pose, segs_of(L), kind, affine)
        assert np.array_equal(mp < 0, masks), (kind, affine)
        # a frame whose only non-finite values lie in rows the solver does not read keeps its slot and its bits
        odd = ~masks & ~np.isfinite(pose).all(axis=(-1, -2))
        assert odd.any() == (len(rows_read(kind, affine)) < 5), (kind, affine)
        for s, l in itertools.product(range(S), range(L)):
            t = np.flatnonzero(odd[s, l])
            assert np.array_equal(mp[s, l][t], np.cumsum(~masks[s, l])[t] - 1), (kind, affine, s, l)
            assert same_bits(cp[s, l][mp[s, l][t]], pose[s, l][t]), (kind, affine, s, l)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [8, 1])
@pytest.mark.parametrize("N", [1, 64, 300, 65537])
def test_filler_is_the_chains_own_leg(hiplib, N, L):
    S = 3
    segs = segs_of(L)
    assert len({tuple(s) for s in segs}) == L
    names = [("all" if s == 2 or (s == 1 and l in (0, 3, 7)) else "random_half") for s in range(S) for l in range(L)]
    pose, masks = gapped_batch(S, L, N, names, "seq", False, seed=N + L)
    cp, mp, nv = compact_on_device(hiplib, pose, segs)
    for s, l in itertools.product(range(S), range(L)):
        if names[s * L + l] != "all":
            continue
        # the straight leg of THIS leg, written out: key point k at (0, 0, -(seg[0] + .. + seg[k-1]))
        filler = np.zeros((5, 3))
        total = 0.0
        for k in range(5):
            filler[k, 2] = -total          # -0.0 for key point 0: the empty sum, negated
            total += segs[l][k] if k < 4 else 0.0
        assert nv[s, l] == 0 and (mp[s, l] == -1).all(), (s, l)
        assert same_bits(cp[s, l], np.broadcast_to(filler, (N, 5, 3)).copy()), (s, l)


def compact_results(rng, S, L, N, sw):
    """Random compact angles, fk, status and nfev; the doubles hold NaN payloads, -0.0 and denormals here and there."""
    out = {}
    for name, w in (("angles", 7), ("fk", 27)):
        a = bits(rng.normal(size=(S, L, N, w))).copy()
        hit = rng.random(a.shape) < 0.02
        a[hit] = np.concatenate([NON_FINITE, bits(np.array([-0.0, 5e-324]))])[rng.integers(0, 8, int(hit.sum()))]
        out[name] = a.view(np.float64)
    out["status"] = rng.integers(-1, 5, size=(S, L, N, sw)).astype(np.int32)
    out["nfev"] = rng.integers(0, 200, size=(S, L, N, sw)).astype(np.int32)
    return out


FILLS = dict(angles=np.nan, fk=np.nan, status=MISSING, nfev=0)


def expand_on_device(hiplib, d_map, d_in, mp, compact, kind, given):
    """Runs the expansion with the optional pairs of `given` into fresh guarded buffers and compares every chain with
    np_expand."""
    import torch
    S, L, N = mp.shape
    d_out = {k: Guarded(v.shape, v.dtype, d_in[k].rec) for k, v in compact.items()}
    opt = {}
    for k in given:
        opt[f"d_c{k}"], opt[f"d_{k}"] = d_in[k].t, d_out[k].t
    hiplib.gaps_expand_device(d_map.t, S, L, N, d_in["angles"].t, d_out["angles"].t, kind=kind, **opt)
    torch.cuda.synchronize()
    where = (N, kind, tuple(given))
    for k in ("angles",) + tuple(given):
        got = d_out[k].numpy()
        for s, l in itertools.product(range(S), range(L)):
            assert same_bits(got[s, l], np_expand(mp[s, l], compact[k][s, l], FILLS[k])), where + (k, s, l)
        assert d_out[k].guards_intact(), where + (k,)
    for k in set(compact) - set(given) - {"angles"}:
        assert d_out[k].untouched(), where + (k,)    # an omitted pair's would-be buffer


@pytest.mark.gpu
@pytest.mark.parametrize("N", N_ALL[:N_ALL.index(65601) + 1] + [131073])
def test_expansion_at_every_geometry_edge(hiplib, N):
    S, L = (1, 2) if N <= 65601 else (1, 1)
    names = expansion_patterns(N, S * L)
    pose, masks = gapped_batch(S, L, N, names, "seq", False, seed=3 * N)
    # maps of the numpy compaction: a failure here is the expansion kernel's
    mp = np.stack([np_compact(pose[0, l], segs_of(L)[l])[1] for l in range(L)])[None]
    assert np.array_equal(mp < 0, masks)
    rng = np.random.default_rng(N)
    d_map = Guarded((S, L, N), np.int32, 1, mp)
    for kind, sw in (("seq", 4), ("generic", 1)):
        compact = compact_results(rng, S, L, N, sw)
        recs = dict(angles=7, fk=27, status=sw, nfev=sw)
        d_in = {k: Guarded(v.shape, v.dtype, recs[k], v) for k, v in compact.items()}
        for r in range(4):
            for given in itertools.combinations(("fk", "status", "nfev"), r):
                expand_on_device(hiplib, d_map, d_in, mp, compact, kind, given)
        for k, buf in d_in.items():      # the inputs are read only
            assert buf.guards_intact() and same_bits(buf.numpy(), compact[k]), (N, kind, k)
    assert d_map.guards_intact() and np.array_equal(d_map.numpy(), mp)


@pytest.mark.gpu
def test_compact_then_expand_round_trip_on_a_side_stream(hiplib):
    import torch
    S, L, N = 2, 3, 65601
    names = compaction_patterns(N)
    segs = segs_of(L)
    pose, masks = gapped_batch(S, L, N, names, "seq", True, seed=99)     # row 0 is not read: payloads ride along
    rng = np.random.default_rng(4)
    cst = rng.integers(-1, 5, size=(S, L, N, 4)).astype(np.int32)
    cnf = rng.integers(0, 200, size=(S, L, N, 4)).astype(np.int32)
    # the numpy composition
    ref = [np_compact(pose[s, l], segs[l], "seq", True) for s in range(S) for l in range(L)]
    rc = np.stack([r[0] for r in ref]).reshape(S, L, N, 15)
    rm = np.stack([r[1] for r in ref]).reshape(S, L, N)
    rn = np.array([r[2] for r in ref], np.int32).reshape(S, L)
    want = dict(angles=np_expand_batch(rm, rc[..., :7], np.nan),
                fk=np_expand_batch(rm, np.concatenate([rc, rc[..., :12]], axis=-1), np.nan),
                status=np_expand_batch(rm, cst, MISSING), nfev=np_expand_batch(rm, cnf, 0))
    d_pose = Guarded((S, L, N, 15), np.float64, 15, pose.reshape(S, L, N, 15))
    d_cpose = Guarded((S, L, N, 15), np.float64, 15)
    d_map, d_nv = Guarded((S, L, N), np.int32, 1), Guarded((S, L), np.int32, 1)
    d_cang, d_cfk = Guarded((S, L, N, 7), np.float64, 7), Guarded((S, L, N, 27), np.float64, 27)
    d_cst, d_cnf = Guarded(cst.shape, np.int32, 4, cst), Guarded(cnf.shape, np.int32, 4, cnf)
    out = dict(angles=Guarded((S, L, N, 7), np.float64, 7), fk=Guarded((S, L, N, 27), np.float64, 27),
               status=Guarded(cst.shape, np.int32, 4), nfev=Guarded(cnf.shape, np.int32, 4))
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    torch.cuda.synchronize()
    for run in range(2):    # the second run starts from a stale map, whose words double as scan scratch
        with torch.cuda.stream(stream):
            hiplib.gaps_compact_device(d_pose.t, S, L, N, leg_params(hiplib, segs), d_cpose.t, d_map.t, d_nv.t,
                                       kind="seq", affine=True, stream=stream)
            c = d_cpose.raw.view(S, L, N, 15)       # int64 words: the stand-ins of a solve result are copies of bits
            d_cang.raw.view(S, L, N, 7).copy_(c[..., :7])
            d_cfk.raw.view(S, L, N, 27).copy_(torch.cat([c, c[..., :12]], dim=-1))
            hiplib.gaps_expand_device(d_map.t, S, L, N, d_cang.t, out["angles"].t, d_cfk=d_cfk.t, d_fk=out["fk"].t,
                                      d_cstatus=d_cst.t, d_status=out["status"].t, d_cnfev=d_cnf.t, d_nfev=out["nfev"].t,
                                      kind="seq", stream=stream)
        stream.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(d_nv.numpy(), rn) and np.array_equal(d_map.numpy(), rm), run
        assert same_bits(d_cpose.numpy(), rc), run
        for k, buf in out.items():
            assert same_bits(buf.numpy(), want[k]), (run, k)
        for buf in [d_pose, d_cpose, d_map, d_nv, d_cang, d_cfk, d_cst, d_cnf] + list(out.values()):
            assert buf.guards_intact(), run
