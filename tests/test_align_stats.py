"""Leg alignment statistics on the GPU (csrc/seqik_align.hip, include/seqik.h "Alignment statistics") against plain numpy.

The operation is exact -- seven series per leg are extracted with numpy's rounding sequence, sorted, and the values at the
requested 0-based ranks returned -- so every comparison here is equality by value (``==``, hence ``-0.0 == 0.0``; the sign
of a zero out of a run of mixed zeros is unspecified) of every returned element, no tolerance.  Reference, restated:

    coordinates       pose[..., 0, a]
    lengths           np.linalg.norm(np.diff(leg, axis=1), axis=2)         = sqrt((dx*dx + dy*dy) + dz*dz)
    order statistics  np.sort(series)[clip(ranks, 0, n - 1)]

CPU tier: the input generators really put the requested ranks where the GPU tests assume (inside a tie run, on the first
and last element, on either side of the sign change, on a denormal), the numpy stand-in of test_alignment.py equals the
reference, and ``AlignPose.leg_affines(on_gpu=True)`` equals the host path / falls back to it on non-finite input.
GPU tier: key counts on both sides of every algorithm switch of the library sort, the grid-stride loop of the extraction,
capacity != count, slabs / sequences / layouts from host and device memory, ``finish`` on another stream than ``add``,
handles of different sizes sharing the pooled arena with the head statistics, ``leg_affines`` on the real library, and the
refusal of host layouts whose chains do not lie inside their chain stride.

Hard inputs (each a (S, L, N, 5, 3) array from a seeded generator):
    quant3 / quant7 / quant64   every coordinate on 3 / 7 / 64 equally filled levels: the 0.45 / 0.55 ranks sit in runs of ties
    constant                    every frame the same key points: all seven series constant
    ulp                         every coordinate c + k ulp(c), k in -2 .. 2
    ascending / descending      all seven series already sorted / sorted the wrong way round
    one_swap                    ascending with two frames exchanged
    symmetric                   every coordinate symmetric about zero, with -0.0, +0.0, +-5e-324 .. +-2.2e-308 around the middle ranks
    pow                         coordinates of magnitude 2**+-500 (the squares 2**+-1000 are still finite), 2**+-600 (dx*dx is inf /
                                underflows to 0: lengths inf and 0) and 2**-520 (dx*dx is a denormal)
    zero_length                 consecutive key points that coincide: dx = dy = dz = 0, length exactly 0
    df3d                        the 1000-frame, six-leg fixture itself
and ``mix``: one leg whose seven series each carry one of these properties at once (see ``mix_leg``), for any N."""
import numpy as np
import pytest

from test_alignment import _FakeAlignStats, df3d  # noqa: F401  (df3d: the module-scoped fixture of test_alignment.py)

from seqikpy_amd import data
from seqikpy_amd.alignment import AlignPose, _quantile_ranks

DBL_MIN = 2.2250738585072014e-308          # the smallest normal double
DEN_MAX = 2.2250738585072009e-308          # the largest denormal
KINDS = ["quant3", "quant7", "quant64", "constant", "ulp", "ascending", "descending", "one_swap", "symmetric", "pow",
         "zero_length"]
HARD_N = 251


# ------------------------------------------------------------------------------------------------------------ reference
def ranks_for(n):
    """The ten ranks of the issue: both clamps, the ends, and the neighbours of numpy's 0.45 / 0.55 quantiles."""
    (lo45, hi45, lo55, hi55), _ = _quantile_ranks(n)
    return [-5, 0, 1, lo45, hi45, lo55, hi55, n - 2, n - 1, n + 7]


def series_of(pose):
    """(S, L, N, 5, 3) -> the seven series of every leg, (L, 7, S * N), in numpy's own arithmetic."""
    pose = np.asarray(pose, dtype=np.float64)
    S, L, N = pose.shape[:3]
    out = np.empty((L, 7, S * N))
    for li in range(L):
        leg = pose[:, li].reshape(S * N, 5, 3)
        out[li, :3] = leg[:, 0, :].T
        with np.errstate(over="ignore", under="ignore"):
            out[li, 3:] = np.linalg.norm(np.diff(leg, axis=1), axis=2).T
    return out


def reference(poses, ranks):
    """Order statistics of the frames of all ``poses`` (a list of (S, L, N, 5, 3) slabs) -> (L, 7, len(ranks))."""
    series = np.concatenate([series_of(p) for p in poses], axis=2)
    n = series.shape[2]
    return np.sort(series, axis=2)[:, :, np.clip(np.asarray(ranks), 0, n - 1)]


def assert_same(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(~(got == want))
    assert bad.size == 0, (what, len(bad), [(tuple(i), got[tuple(i)], want[tuple(i)]) for i in bad[:5]])


# ----------------------------------------------------------------------------------------------------------- generators
def _balanced(values, n, rng):
    """n draws from ``values``, every value equally often (+-1), in random order."""
    return np.asarray(values, dtype=np.float64)[rng.permutation(np.arange(n) % len(values))]


def _symmetric(n, rng):
    """n values symmetric about zero in random order: -0.0 and +0.0, then 8 % of n denormals on either side (5e-324 and
    the largest denormal among them), the smallest normal, then ordinary magnitudes.  The 0.45 / 0.55 ranks (5 % of n
    from the middle) therefore land on a negative / a positive denormal."""
    m = n // 2
    nd = min(max(m - 1, 0), int(np.ceil(0.08 * n)))
    den = rng.integers(1, 2**52, nd).astype(np.float64) * 5e-324
    if nd >= 2:
        den[0], den[1] = 5e-324, DEN_MAX
    rest = max(m - 1 - nd, 0)
    normal = DBL_MIN + np.abs(rng.standard_normal(rest))
    normal[:1] = DBL_MIN
    mag = np.concatenate([[0.0][:m], den, normal])
    vals = np.concatenate([-mag, mag, [0.0] * (n - 2 * m)])
    return vals[rng.permutation(n)]


def _ascending(n):
    t = np.arange(1, n + 1, dtype=np.float64)
    kp = np.empty((n, 5, 3))
    for r in range(5):
        kp[:, r, 0] = (r + 1) * t * 0.125        # coxa x and (dy = dz = 0) all four lengths: t / 8, exactly
        kp[:, r, 1] = 0.5 * t
        kp[:, r, 2] = 0.25 * t - 7.0
    return kp


def hard_leg(kind, n, rng):
    """(n, 5, 3) key points of one leg, of the kind named (module docstring)."""
    if kind.startswith("quant"):
        levels = int(kind[5:])
        kp = np.empty((n, 5, 3))
        for r in range(5):
            for a in range(3):
                kp[:, r, a] = 0.25 * (rng.permutation(np.arange(n) % levels) - levels // 2)
        return kp
    if kind == "constant":
        return np.broadcast_to(rng.standard_normal((5, 3)), (n, 5, 3)).copy()
    if kind == "ulp":
        c = rng.uniform(0.5, 2.0, (5, 3))
        return c + rng.integers(-2, 3, (n, 5, 3)) * np.spacing(c)
    if kind == "ascending":
        return _ascending(n)
    if kind == "descending":
        return _ascending(n)[::-1].copy()
    if kind == "one_swap":
        kp = _ascending(n)
        if n >= 3:
            kp[[n // 3, 2 * n // 3]] = kp[[2 * n // 3, n // 3]]
        return kp
    if kind == "symmetric":
        return np.stack([np.stack([_symmetric(n, rng) for _ in range(3)], axis=1) for _ in range(5)], axis=1)
    if kind == "pow":
        e = _balanced([500.0, -500.0, 600.0, -600.0, -520.0, 0.0], n, rng)
        return rng.uniform(-1.0, 1.0, (n, 5, 3)) * (2.0 ** e)[:, None, None]
    if kind == "zero_length":
        kp = 0.25 * rng.integers(-8, 9, (n, 5, 3))
        for f in range(0, n, 2):
            r = int(rng.integers(0, 4))
            kp[f, r + 1] = kp[f, r]
        return kp[rng.permutation(n)]
    raise ValueError(kind)


def hard_input(kind, S, L, N, seed=0):
    rng = np.random.default_rng([seed, KINDS.index(kind), S, L, N])
    return np.stack([np.stack([hard_leg(kind, N, rng) for _ in range(L)]) for _ in range(S)])


def mix_leg(n, rng):
    """(n, 5, 3) key points of one leg whose seven series are hard in different ways at once:
        coxa x   three equally filled levels -1.5, 0.25, 2.0: the 0.45 / 0.55 ranks lie inside the middle run of ties
        coxa y   ``_symmetric``: the 0.45 rank on a negative, the 0.55 rank on a positive denormal, -0.0 / +0.0 between
        coxa z   1.1 + k ulp, k in -3 .. 3
        coxa length    0.25 k exactly, k in 1 .. 7 (ties); femur and tarsus length: generic values (the rounding sequence);
        tibia length   on a dyadic grid (ties), and by frame class: exactly 0 (coinciding key points), 0 by underflow
                       (2**-600), through a denormal dx*dx (2**-520), about 2**-500 and 2**500, and inf (2**600);
                       the huge classes make the femur / tarsus lengths inf or huge too."""
    kp = np.empty((n, 5, 3))
    kp[:, 0, 0] = _balanced([-1.5, 0.25, 2.0], n, rng)
    kp[:, 0, 1] = _symmetric(n, rng)
    kp[:, 0, 2] = 1.1 + _balanced(np.arange(-3, 4), n, rng) * np.spacing(1.1)
    kp[:, 1] = kp[:, 0]
    kp[:, 1, 0] += 0.25 * _balanced(np.arange(1, 8), n, rng)
    kp[:, 2:4] = 0.25 * rng.integers(-8, 9, (n, 2, 3))
    kp[:, 4] = rng.standard_normal((n, 3))
    cls = rng.permutation(np.arange(n) % 20)
    kp[cls < 3, 3] = kp[cls < 3, 2]
    for c, e, rows in ((3, 600.0, slice(2, 5)), (4, -600.0, slice(2, 4)), (5, -520.0, slice(2, 4)),
                       (6, 500.0, slice(2, 5)), (7, -500.0, slice(2, 4))):
        m = cls == c
        kp[m, rows] = rng.uniform(-1.0, 1.0, kp[m, rows].shape) * 2.0 ** e
    return kp


def mix(S, L, N, seed=0):
    rng = np.random.default_rng([seed, S, L, N])
    return np.stack([np.stack([mix_leg(N, rng) for _ in range(L)]) for _ in range(S)])


# ------------------------------------------------------------------------- what the GPU tests assume about their inputs
def _run(s, k):
    """Length of the run of equal values around rank k of the ascending series s."""
    return int(np.searchsorted(s, s[k], "right") - np.searchsorted(s, s[k], "left"))


def _is_denormal(v):
    return v != 0.0 and abs(v) < DBL_MIN


def check_ranks(n):
    r = ranks_for(n)
    assert r[0] < 0 and r[-1] > n - 1 and 0 in r and n - 1 in r and len(r) == 10
    assert all(0 <= k <= n - 1 for k in r[3:7]) and r[3] <= r[4] and r[5] <= r[6] and r[3] <= r[5]
    return r


def check_mix(pose):
    """The properties ``mix_leg`` promises, on leg 0 of a one-sequence input with N >= 63 frames."""
    n = pose.shape[2]
    assert pose.shape[0] == 1 and n >= 63 and np.isfinite(pose).all()
    _, _, _, lo45, hi45, lo55, hi55 = check_ranks(n)[:7]
    raw = series_of(pose)[0]
    s = np.sort(raw, axis=1)
    x, y, z, coxa, femur, tibia = s[0], s[1], s[2], s[3], s[4], s[5]
    assert x[lo45] == x[hi55] == 0.25 and x[lo45 - 1] == 0.25 and x[hi55 + 1] == 0.25            # inside a tie run
    assert x[0] == -1.5 and x[-1] == 2.0                                                             # first and last
    assert y[lo45] < 0.0 < y[hi55] and y[hi45] < 0.0 < y[lo55]                                       # the sign change
    assert all(_is_denormal(y[k]) for k in (lo45, hi45, lo55, hi55))                                 # on a denormal
    zeros = raw[1][raw[1] == 0.0]
    assert np.signbit(zeros).any() and not np.signbit(zeros).all()                                   # -0.0 and +0.0
    assert (np.abs(y) == 5e-324).sum() == 2 and (np.abs(y) == DEN_MAX).sum() == 2
    assert np.array_equal(np.unique(z), 1.1 + np.arange(-3, 4) * np.spacing(1.1))                    # one ulp apart
    assert set(np.unique(coxa)) == {0.25 * k for k in range(1, 8)} and _run(coxa, lo45) >= 3
    assert tibia[0] == 0.0 and tibia[1] == 0.0 and tibia[-1] == np.inf and tibia[-2] == np.inf       # 0 and inf at the ends
    assert np.isinf(femur[-1]) and np.unique(femur).size > n // 2                                    # generic values
    assert ((tibia > 0) & (tibia < 2.0 ** -510)).any() and ((tibia > 2.0 ** 490) & (tibia < np.inf)).any()


def check_hard(kind, pose):
    """The property each hard input is named for, on every leg of a one-sequence input."""
    n = pose.shape[2]
    assert pose.shape[0] == 1 and np.isfinite(pose).all()
    _, _, _, lo45, hi45, lo55, hi55 = check_ranks(n)[:7]
    raw = series_of(pose)
    srt = np.sort(raw, axis=2)
    for li in range(pose.shape[1]):
        r, s = raw[li], srt[li]
        if kind.startswith("quant"):
            for j in range(3):
                assert s[j][lo45] == s[j][hi45] and s[j][lo55] == s[j][hi55], (kind, li, j)
                assert min(_run(s[j], lo45), _run(s[j], lo55)) >= (3 if kind == "quant64" else 30), (kind, li, j)
                assert np.unique(s[j]).size == int(kind[5:])
        elif kind == "constant":
            assert (s[:, 0] == s[:, -1]).all()
        elif kind == "ulp":
            for j in range(3):
                u = np.unique(s[j])
                assert 2 <= u.size <= 5 and (np.diff(u) <= 2 * np.spacing(u[0])).all() and _run(s[j], lo45) >= 3
        elif kind == "ascending":
            assert np.array_equal(r, s) and (np.diff(s, axis=1) > 0).all()
        elif kind == "descending":
            assert np.array_equal(r[:, ::-1], s) and (np.diff(s, axis=1) > 0).all()
        elif kind == "one_swap":
            assert ((r != s).sum(axis=1) == 2).all()
        elif kind == "symmetric":
            for j in range(3):
                zeros = r[j][r[j] == 0.0]
                assert np.signbit(zeros).any() and not np.signbit(zeros).all()
                assert s[j][lo45] < 0.0 < s[j][hi55] and _is_denormal(s[j][lo45]) and _is_denormal(s[j][hi55])
                assert (np.abs(s[j]) == 5e-324).sum() == 2 and (np.abs(s[j]) == DEN_MAX).sum() == 2
                assert np.array_equal(s[j], -s[j][::-1])
        elif kind == "pow":
            for j in range(3, 7):
                assert s[j][0] == 0.0 and s[j][1] == 0.0 and s[j][-1] == np.inf and s[j][-2] == np.inf
                assert ((s[j] > 0) & (s[j] < 2.0 ** -510)).any() and ((s[j] > 2.0 ** 490) & (s[j] < np.inf)).any()
        elif kind == "zero_length":
            for j in range(3, 7):
                assert s[j][0] == 0.0 and _run(s[j], 0) >= 3 and s[j][-1] > 0.0


def df3d_pose(df3d):
    _, legs, raw = df3d
    return np.stack([raw[f"{l}_leg"] for l in legs])[None]          # (1, 6, 1000, 5, 3)


# -------------------------------------------------------------------------------------------------------- CPU-tier tests
MIX_SIZES_CPU = [63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 65535, 65536, 65537]


def test_the_mix_puts_the_requested_ranks_on_ties_ends_the_sign_change_and_denormals():
    for n in MIX_SIZES_CPU:
        check_mix(mix(1, 1, n))
    for n in (1, 2, 3):                                              # nothing to promise, but well-formed and finite
        assert mix(1, 1, n).shape == (1, 1, n, 5, 3) and np.isfinite(mix(1, 1, n)).all()
        check_ranks(n)


@pytest.mark.parametrize("kind", KINDS)
def test_every_hard_input_has_the_property_it_is_named_for(kind):
    for n in (HARD_N, 1000):
        check_hard(kind, hard_input(kind, 1, 3, n))


def _fake_stats(poses, ranks):
    st = _FakeAlignStats(poses[0].shape[1], 0)
    for p in poses:
        st.add(p)
    return st.finish(ranks)


def test_the_numpy_stand_in_equals_the_reference_on_all_hard_inputs(df3d):
    """``_FakeAlignStats`` (what the CPU tier puts in the GPU's place) and the reference restated above agree."""
    inputs = [hard_input(k, 2, 3, HARD_N) for k in KINDS] + [mix(2, 2, 257), df3d_pose(df3d)]
    for pose in inputs:
        n = pose.shape[0] * pose.shape[2]
        ranks = [k for k in ranks_for(n) if 0 <= k <= n - 1]
        with np.errstate(over="ignore", under="ignore"):
            got = _fake_stats([pose], ranks)
            halves = _fake_stats([pose[:, :, 100:], pose[:, :, :100]], ranks)
        assert_same(got, reference([pose], ranks))
        assert_same(halves, reference([pose], ranks))


def _leg_dict(legs, pose):
    return {f"{l}_leg": pose[0, i] for i, l in enumerate(legs)}


def assert_affines_equal(host, dev, legs, what):
    for leg in legs:
        assert (host[leg][0] == dev[leg][0]).all(), (what, leg, host[leg][0], dev[leg][0])
        assert host[leg][1] == dev[leg][1], (what, leg, host[leg][1], dev[leg][1])
        assert np.array_equal(host[leg][2], dev[leg][2]), (what, leg)


def _affine_inputs(df3d, n):
    _, legs, _ = df3d
    return {"df3d": _leg_dict(legs, df3d_pose(df3d)[:, :, :n]), "quant3": _leg_dict(legs, hard_input("quant3", 1, 6, n))}


def test_leg_affines_through_the_stand_in_equal_the_host_path(df3d, monkeypatch):
    """N = 1, 2, 3: lo == hi or gamma 0 / near 1; 4, 11, 12, 37, 999, 1000: the interpolation weight changes with N."""
    from seqikpy_amd import _lib
    monkeypatch.setattr(_lib, "AlignStats", _FakeAlignStats)
    _, legs, _ = df3d
    for n in (1, 2, 3, 4, 11, 12, 37, 999, 1000):
        for name, cut in _affine_inputs(df3d, n).items():
            al = AlignPose(cut, legs, body_template=data.TEMPLATE_NMF_LOCOMOTION, log_level="ERROR")
            with np.errstate(divide="ignore"):
                assert_affines_equal(al.leg_affines(), al.leg_affines(on_gpu=True), legs, (name, n))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_leg_affines_take_the_host_path_on_non_finite_input_without_opening_a_handle(df3d, monkeypatch, bad):
    from seqikpy_amd import _lib

    class Refuses:
        def __init__(self, *a, **k):
            raise AssertionError("a statistics handle was opened for non-finite input")

    monkeypatch.setattr(_lib, "AlignStats", Refuses)
    _, legs, raw = df3d
    for where in ((0, 0, 0), (517, 3, 2), (999, 4, 1)):
        cut = {k: v.copy() for k, v in raw.items()}
        cut["RM_leg"][where] = bad
        al = AlignPose(cut, legs, body_template=data.TEMPLATE_NMF_LOCOMOTION, log_level="ERROR")
        with np.errstate(invalid="ignore"):
            host, dev = al.leg_affines(), al.leg_affines(on_gpu=True)
        for leg in legs:
            assert np.array_equal(host[leg][0], dev[leg][0], equal_nan=True), (where, leg)
            assert np.array_equal(host[leg][1], dev[leg][1], equal_nan=True), (where, leg)
            assert np.array_equal(host[leg][2], dev[leg][2]), (where, leg)


def test_host_arrays_smaller_than_their_layout_are_refused_before_the_library_sees_them(monkeypatch):
    """``AlignStats.add`` hands the library ``pose_chain * n_seq * n_legs`` doubles of a host array with a layout."""
    from seqikpy_amd import _lib

    def called(*args):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "_call", called)
    st = _lib.AlignStats.__new__(_lib.AlignStats)
    st.n_legs, st._h = 2, None
    with pytest.raises(ValueError, match="holds 149 doubles, the layout addresses 150"):
        st.add(np.zeros(149), n_seq=1, n_frames=5, layout=_lib.planar_layout(5))
    for sizes in ({}, {"n_seq": 1}, {"n_frames": 5}):                # a layout says nothing about the sizes
        with pytest.raises(ValueError, match="n_seq and n_frames are required"):
            st.add(np.zeros(150), layout=_lib.planar_layout(5), **sizes)


# -------------------------------------------------------------------------------------------------------- GPU-tier tests
# Key counts at which the library sort changes its algorithm for 8-byte keys without values on gfx950: see
# test_sizes_by_sort_path.  201072 = (1 << 17) + 70000.
SORT_SWITCHES = [201071, 201072, 201073, 1048575, 1048576, 1048577, 1050623, 1050624, 1050625]
SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 65535, 65536, 65537] + SORT_SWITCHES


def gpu_stats(hiplib, pose, ranks, capacity=None):
    S, L, N = pose.shape[:3]
    with hiplib.AlignStats(L, S * N if capacity is None else capacity) as st:
        st.add(pose)
        return st.finish(ranks)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_sizes_by_sort_path(hiplib, n):
    """One leg of the hard-input mix, capacity == N, at the ten ranks (both clamps included), for N around the wavefront,
    block and tile sizes and on either side of every key count at which the installed rocPRIM (4.2.0, behind hipCUB's
    ``DeviceRadixSort::SortKeys``, default configuration) changes what it runs for ``double`` keys without values:

    * ``rocprim/device/device_radix_sort.hpp``, ``radix_sort_impl``: ``size <= single_sort_items_per_block`` sorts in one
      block; ``block_size * items_per_thread`` = min(256, 256) * min(4, 4) = **1024** from
      ``radix_sort_block_sort_config_base`` in ``rocprim/device/detail/device_config_helper.hpp``
      (``merge_sort_block_size(8) * 2`` = 256, ``min(4, merge_sort_items_per_thread(8))`` = 4).
    * same function: ``size <= merge_sort_limit`` takes the merge sort, above it onesweep;
      ``radix_sort_config<>::merge_sort_limit`` = 1024 * 1024 = **1048576** (``device_radix_sort_config.hpp``).
    * ``rocprim/device/device_merge_sort.hpp``: ``use_mergepath = size > merge_oddeven_config.size_limit``;
      ``detail/config/device_merge_sort_block_merge.hpp`` has no gfx950 entry, so the limit is that of
      ``merge_sort_block_merge_config_base``: (1 << 17) + 70000 = **201072**.
    * onesweep tile: ``default_radix_sort_onesweep_config`` for gfx950, double, ``empty_type`` in
      ``detail/config/device_radix_sort_onesweep.hpp`` is ``kernel_config<512, 12>``, 6144 keys per block; the first
      count above the merge limit whose last block is full is 171 * 6144 = **1050624** (``full_blocks`` in
      ``radix_sort_onesweep_iteration``)."""
    pose = mix(1, 1, n)
    if n >= 63:
        check_mix(pose)
    ranks = check_ranks(n)
    assert_same(gpu_stats(hiplib, pose, ranks), reference([pose], ranks), n)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS + ["df3d"])
def test_every_hard_input_on_the_gpu(hiplib, df3d, kind):
    pose = df3d_pose(df3d) if kind == "df3d" else hard_input(kind, 1, 3, HARD_N)
    if kind != "df3d":
        check_hard(kind, pose)
    ranks = check_ranks(pose.shape[2])
    assert_same(gpu_stats(hiplib, pose, ranks), reference([pose], ranks), kind)


@pytest.mark.gpu
@pytest.mark.parametrize("S,L,N", [(1, 2, 600_001), (3, 8, 50_001)])
def test_grid_stride_extraction(hiplib, S, L, N):
    """More than 4096 blocks x 256 threads = 1 048 576 elements in one ``add``: the extraction kernel's ``i += stride``
    pass.  All seven series of every leg at the ten ranks (n_legs = 8 is the documented upper bound)."""
    assert S * L * N > 4096 * 256
    pose = mix(S, L, N)
    ranks = check_ranks(S * N)
    assert_same(gpu_stats(hiplib, pose, ranks), reference([pose], ranks))


@pytest.mark.gpu
def test_capacity_larger_than_count(hiplib):
    """Series are laid out by capacity, sorted and clamped by count: capacity 5000 filled with 1237, then 3237, then 1."""
    pose = mix(1, 3, 3237, seed=3)
    a, b = np.ascontiguousarray(pose[:, :, :1237]), np.ascontiguousarray(pose[:, :, 1237:])
    with hiplib.AlignStats(3, 5000) as st:
        st.add(a)
        assert_same(st.finish(ranks_for(1237)), reference([a], ranks_for(1237)), "1237 of 5000")
        st.add(b)                                                    # no reset: appended
        r = ranks_for(3237)
        want = reference([pose], r)
        assert_same(st.finish(r), want, "3237 of 5000")
        assert_same(st.finish(r), want, "finish twice")
        with pytest.raises(ValueError, match="bad argument.*more frames than the capacity"):
            st.add(np.ascontiguousarray(pose[:, :, :1764]))         # 3237 + 1764 = 5001
        assert_same(st.finish(r), want, "after a refused add")
        st.add(np.ascontiguousarray(pose[:, :, :1763]))             # exactly full
        full = [pose, pose[:, :, :1763]]
        assert_same(st.finish(ranks_for(5000)), reference(full, ranks_for(5000)), "5000 of 5000")
        st.reset()
        one = np.ascontiguousarray(pose[:, :, 77:78])
        st.add(one)                                                  # add after finish and reset
        assert_same(st.finish(ranks_for(1)), reference([one], ranks_for(1)), "1 of 5000")
        with pytest.raises(ValueError, match="n_ranks must be 1..16"):
            st.finish(list(range(17)))
        st.reset()
        with pytest.raises(ValueError, match="no frames were added"):
            st.finish([0])


@pytest.fixture(scope="module")
def four_sequences():
    """(4, 6, 251, 5, 3): the mix in four sequences of six legs, its ranks and its reference, computed once."""
    pose = mix(4, 6, 251, seed=4)
    pose.setflags(write=False)
    ranks = ranks_for(4 * 251)
    want = reference([pose], ranks)
    want.setflags(write=False)
    return pose, ranks, want


def planar(pose):
    """(S, L, N, 5, 3) -> [chain][5][frame][3], the layout of ``_lib.planar_layout``."""
    return np.ascontiguousarray(pose.transpose(0, 1, 3, 2, 4))


@pytest.mark.gpu
def test_slabs_and_sequences_from_host_memory(hiplib, four_sequences):
    from seqikpy_amd import stream_sharding
    pose, ranks, want = four_sequences
    S, L, N = pose.shape[:3]
    with hiplib.AlignStats(L, S * N) as st:
        st.add(pose)                                                 # n_seq = 4 in one call
        assert_same(st.finish(ranks), want, "one call")
        st.reset()
        for s in reversed(range(S)):                                 # four calls of one sequence, last first
            st.add(np.ascontiguousarray(pose[s:s + 1]))
        assert_same(st.finish(ranks), want, "four calls")
        st.reset()
        # the same frames of every leg as slabs of unequal length: the staging buffer grows (1 -> 250), is reused by a
        # smaller slab (3), and grows again (750)
        frames = pose.transpose(1, 0, 2, 3, 4).reshape(L, S * N, 5, 3)
        start = 0
        for length in (1, 250, 3, 750):
            st.add(np.ascontiguousarray(frames[None, :, start:start + length]))
            start += length
        assert start == S * N
        assert_same(st.finish(ranks), want, "unequal slabs")
        st.reset()
        st.add(planar(pose), n_seq=S, n_frames=N, layout=hiplib.planar_layout(N))
        assert_same(st.finish(ranks), want, "planar, four sequences")
        st.reset()
        st.add(planar(pose[:1]), n_seq=1, n_frames=N, layout=hiplib.planar_layout(N))   # after a larger staging copy
        assert_same(st.finish(ranks_for(N)), reference([pose[:1]], ranks_for(N)), "planar, one sequence")
    # the streaming path's own pass 1: three planar slabs of 100 frames
    slabs = [planar(frames[None, :, 100 * k:100 * (k + 1)]) for k in range(3)]
    got = stream_sharding.align_stats_all_slabs(lambda k: slabs[k], 3, 100, L, ranks_for(300))
    assert_same(got, reference([frames[None, :, :300]], ranks_for(300)), "align_stats_all_slabs")


@pytest.mark.gpu
def test_one_leg_and_eight_legs(hiplib):
    """The documented bounds of n_legs, several sequences each, from host memory."""
    for L in (1, 8):
        p = mix(3, L, 97, seed=L)
        assert_same(gpu_stats(hiplib, p, ranks_for(3 * 97)), reference([p], ranks_for(3 * 97)), L)
    with pytest.raises(ValueError, match="n_legs 1..8"):
        hiplib.AlignStats(9, 10)
    with pytest.raises(ValueError, match="n_legs 1..8"):
        hiplib.AlignStats(0, 10)


@pytest.mark.gpu
def test_device_resident_input_on_a_side_stream(hiplib, four_sequences):
    """Dense, planar and padded layouts of device memory, ``add`` and ``finish`` on one non-default torch stream.  The
    padded layout's filler (chain stride 37 doubles longer than needed, rows 4 doubles apart) is 1e300: read anywhere,
    it would be the last element of a series or make a length inf."""
    import torch
    pose, ranks, want = four_sequences
    S, L, N = pose.shape[:3]
    padded = np.full((S, L, N * 20 + 37), 1e300)
    padded[:, :, :N * 20].reshape(S, L, N, 5, 4)[..., :3] = pose
    assert padded[0, 0, 3] == 1e300 and padded[0, 0, 4] == pose[0, 0, 0, 1, 0]
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    with torch.cuda.stream(side):
        d_dense = torch.from_numpy(np.array(pose)).cuda()
        d_planar = torch.from_numpy(planar(pose)).cuda()
        d_padded = torch.from_numpy(padded).cuda()
    L_ = hiplib.SeqikLayout
    with hiplib.AlignStats(L, S * N) as st:
        st.add(d_dense, n_seq=S, n_frames=N, on_device=True, stream=side)
        assert_same(st.finish(ranks, stream=side), want, "dense")
        st.reset()
        st.add(d_planar, n_seq=S, n_frames=N, layout=hiplib.planar_layout(N), on_device=True, stream=side)
        assert_same(st.finish(ranks, stream=side), want, "planar")
        st.reset()
        st.add(d_padded, n_seq=S, n_frames=N, layout=L_(N * 20 + 37, 4, 20, 0, 0, 0), on_device=True, stream=side)
        assert_same(st.finish(ranks, stream=side), want, "padded")
    side.synchronize()


@pytest.mark.gpu
def test_finish_on_the_default_stream_after_a_synchronised_side_stream_add(hiplib, four_sequences):
    """The documented way to mix streams: ``add`` with device memory is asynchronous on its stream, the caller
    synchronises that stream, and ``finish`` on the default stream (0) sees the frames."""
    import torch
    pose, ranks, want = four_sequences
    S, L, N = pose.shape[:3]
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    with torch.cuda.stream(side):
        d_pose = torch.from_numpy(np.array(pose)).cuda()
    with hiplib.AlignStats(L, S * N) as st:
        st.add(d_pose, n_seq=S, n_frames=N, on_device=True, stream=side)
        side.synchronize()
        assert_same(st.finish(ranks), want, "finish on stream 0")
        assert_same(st.finish(ranks, stream=side), want, "and again on the side stream")


@pytest.mark.gpu
def test_handles_of_different_sizes_and_a_head_call_share_the_pooled_arena(hiplib):
    """``finish`` keeps its one-series sort buffer and the library sort's temporaries in the arena of a pooled host-call
    context, which every host-buffer call borrows and regrows: two handles open at once, 1 leg x 1025 frames and 8 legs
    x 5000 frames, finished small, large, small again with the head statistics (whose uploads take the same arena) in
    between.  No call's scratch may survive as another's input: every result against numpy."""
    from test_head_alignment import fixture_raw, np_series
    small, large = mix(1, 1, 1025, seed=5), mix(1, 8, 5000, seed=6)
    r_small, r_large = ranks_for(1025), ranks_for(5000)
    want_small, want_large = reference([small], r_small), reference([large], r_large)
    _, raw = fixture_raw()
    head_ranks = lambda n: [0, n // 2, n - 1]  # noqa: E731
    with hiplib.AlignStats(1, 1025) as a, hiplib.AlignStats(8, 5000) as b:
        a.add(small)
        b.add(large)
        assert_same(a.finish(r_small), want_small, "small, first")
        assert_same(b.finish(r_large), want_large, "large: the arena grows")
        res = hiplib.head_align_stats(raw["R_head"], raw["L_head"], raw["Thorax"], head_ranks)
        assert_same(a.finish(r_small), want_small, "small, inside the larger arena after the head call")
        assert_same(b.finish(r_large), want_large, "large again")
    assert res["n_nonfinite"] == 0 and res["order"] is not None
    for i, side in enumerate("RL"):
        d, ln, mask = np_series(raw[f"{side}_head"], raw["Thorax"])
        assert res["n_stat"][i] == mask.sum()
        series = [raw[f"{side}_head"][mask, 0, c] for c in range(3)] + [d[mask], ln]
        for j, v in enumerate(series):
            assert np.array_equal(res["order"][i, j], np.sort(v)[head_ranks(len(v))]), (side, j)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 12, 37, 999, 1000])
def test_leg_affines_on_the_real_library(hiplib, df3d, n):
    """N = 1, 2, 3 (lo == hi, gamma 0 or near 1) reached the real sort through nothing so far."""
    _, legs, _ = df3d
    for name, cut in _affine_inputs(df3d, n).items():
        al = AlignPose(cut, legs, body_template=data.TEMPLATE_NMF_LOCOMOTION, log_level="ERROR")
        with np.errstate(divide="ignore"):
            assert_affines_equal(al.leg_affines(), al.leg_affines(on_gpu=True), legs, (name, n))


@pytest.mark.gpu
def test_host_layouts_outside_their_chain_stride_are_refused(hiplib, four_sequences):
    """A host slab is staged as one piece of n_seq * n_legs chain strides: a layout with a stride <= 0, or whose key
    points do not lie inside their chain stride, is a bad argument before any device work, under the text that names the
    rule, and the handle goes on working.  Device memory keeps its own, older refusals."""
    import torch
    pose, _, _ = four_sequences
    S, L, N = 2, 6, 40
    good = np.ascontiguousarray(pose[:S, :, :N])
    ranks = ranks_for(S * N)
    want = reference([good], ranks)
    lay = hiplib.SeqikLayout
    room = np.zeros(S * L * N * 15 + 64)                          # every refused call may address all of it
    room[:good.size] = good.ravel()
    refused = {
        "pose_chain = 0": lay(0, 3, 15, 0, 0, 0),
        "pose_row = 0": lay(15 * N, 0, 15, 0, 0, 0),
        "pose_frame = 0": lay(15 * N, 3, 0, 0, 0, 0),
        "pose_chain < 0": lay(-15 * N, 3, 15, 0, 0, 0),
        "pose_row < 0": lay(15 * N, -3, 15, 0, 0, 0),
        "pose_frame < 0": lay(15 * N, 3, -15, 0, 0, 0),
        "chain stride one short": lay(15 * N - 1, 3, 15, 0, 0, 0),
        "frame-major": lay(15, 3, 15 * S * L, 0, 0, 0),           # [frame][chain][5][3]
        "planar rows past the chain": lay(15 * N, 3 * N + 1, 3, 0, 0, 0),
    }
    with hiplib.AlignStats(L, 3 * S * N) as st:
        for what, layout in refused.items():
            with pytest.raises(ValueError, match="bad argument.*all three pose strides.*> 0.*inside its chain stride"):
                st.add(room, n_seq=S, n_frames=N, layout=layout)
            st.add(good)
            assert_same(st.finish(ranks), want, what)
            st.reset()
        # device memory: the caller owns the extent; a zero chain stride is one chain read over and over
        d = torch.from_numpy(good).cuda()
        with pytest.raises(ValueError, match="bad argument.*pose_chain must be > 0 for more than one chain"):
            st.add(d, n_seq=S, n_frames=N, layout=lay(0, 3, 15, 0, 0, 0), on_device=True)
        for layout in (lay(15 * N, 0, 15, 0, 0, 0), lay(15 * N, 3, 0, 0, 0, 0), lay(-1, 3, 15, 0, 0, 0)):
            with pytest.raises(ValueError, match="bad argument.*layout strides must be positive"):
                st.add(d, n_seq=S, n_frames=N, layout=layout, on_device=True)
        st.add(good)
        assert_same(st.finish(ranks), want, "after the device refusal")
    with hiplib.AlignStats(1, N) as st:                              # ... and is accepted for a single chain
        one = np.ascontiguousarray(good[:1, :1])
        st.add(torch.from_numpy(one).cuda(), n_seq=1, n_frames=N, layout=lay(0, 3, 15, 0, 0, 0), on_device=True)
        torch.cuda.synchronize()
        assert_same(st.finish(ranks_for(N)), reference([one], ranks_for(N)), "single chain, pose_chain = 0")
