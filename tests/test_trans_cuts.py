"""The four round-9 cuts of csrc/seqik_core.hpp keep every bit: divisions and square roots whose value nothing reads as a value.

  A  bit 32   solve_tr_2x2<false>: the rank test lmin > (3 eps)^2 lmax without its eigenvalues where det > 2^-97 (a + c)^2
  B  bit 64   stages 1-3: ||step|| < xtol (xtol + ||x||) decided on the squares, outside a band of 2^-49 around T^2
  C  bit 128  stage 4: sqrt(fl(a0 a0)) == |a0| where the square is a normal number
  E  bit 512  the first multiplier of stage 1's rank-deficient solve without sqrt(0 * alpha_upper)
(D, bit 256, was taken out with its tests: EXPERIMENTS.md 21.4)

CPU tier: each short form against its plain form on the host, compared as integers; the harness reports the branch taken
(tests/harness/trans_cuts_harness.hip).  GPU tier: HIP == C oracle bit for bit on 70 sequences x 6 legs x 6 frames (per leg one
full wavefront and one of six lanes) through every launch path, on three inputs whose branch coverage is asserted first, from
the oracle alone."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from harness_build import build_harness
from pass_cut_support import (LAUNCH_PATHS, assert_equal_reference, bits, first_pass_rows, narrow_limits, oracle_reference,
                              same_bits, solve_on_path)

dp = ctypes.POINTER(ctypes.c_double)
ip = ctypes.POINTER(ctypes.c_int32)
i64p = ctypes.POINTER(ctypes.c_int64)


@pytest.fixture(scope="module")
def tc():
    lib = ctypes.CDLL(build_harness(os.path.join(ROOT, "tests", "harness", "trans_cuts_harness.hip")))
    lib.tc_rank.argtypes = [dp, ctypes.c_int64, ip, ip]
    lib.tc_abc.argtypes = [dp, ctypes.c_int64, dp]
    lib.tc_tr2_compare.restype = ctypes.c_int64
    lib.tc_tr2_compare.argtypes = [dp, ctypes.c_int64, i64p]
    lib.tc_step_below.argtypes = [dp, dp, ctypes.c_int64, ip, ip, ip]
    lib.tc_norm1.argtypes = [dp, ctypes.c_int64, dp, dp, ip]
    lib.tc_first_alpha.argtypes = [dp, ctypes.c_int64, dp, dp]
    return lib


@pytest.fixture(scope="module")
def recorded(tc):
    """First-pass operands of every solve of host runs of run_stage over the shipped recording, all six legs: rows [n][ROW],
    column 27 = stage."""
    return first_pass_rows()


# ---- A: the rank test -------------------------------------------------------------------------------------------------------
def _rank(tc, abc):
    abc = np.ascontiguousarray(abc, dtype=np.float64)
    sure, plain = np.zeros(len(abc), np.int32), np.zeros(len(abc), np.int32)
    tc.tc_rank(abc.ctypes.data_as(dp), len(abc), sure.ctypes.data_as(ip), plain.ctypes.data_as(ip))
    return sure.astype(bool), plain.astype(bool)


def _abc(tc, ops):
    ops = np.ascontiguousarray(ops, dtype=np.float64)
    abc = np.zeros((len(ops), 3))
    tc.tc_abc(ops.ctypes.data_as(dp), len(ops), abc.ctypes.data_as(dp))
    return abc


def _made_up_systems(rng, n):
    """3 x 2 systems [n][13] whose second column is the first times a factor plus a perturbation of relative size 2^-10 ..
    2^-60, with diag_h of 0 or small positive values"""
    ops = np.zeros((n, 13))
    u = rng.normal(0.0, 1.0, (n, 3)) * 10.0 ** rng.uniform(-3, 1, (n, 1))
    w = rng.normal(0.0, 1.0, (n, 3)) * np.linalg.norm(u, axis=1, keepdims=True)
    eps = 2.0 ** -rng.integers(10, 61, (n, 1)).astype(np.float64)
    k = rng.choice([1.0, -1.0, 0.5, 3.0, 1e-3], (n, 1))
    ops[:, 0:6:2] = u
    ops[:, 1:6:2] = k * u + eps * w
    ops[:, 6:8] = np.where(rng.random((n, 2)) < 0.5, 0.0, 10.0 ** rng.uniform(-30, -2, (n, 2)))
    ops[:, 8:11] = rng.normal(0.0, 0.5, (n, 3))
    ops[:, 11] = 10.0 ** rng.uniform(-3, 1, n)
    return ops


def test_rank_guard_is_never_sure_of_a_false(tc, recorded):
    rng = np.random.default_rng(3200)
    two = recorded[(recorded[:, 27] == 2) | (recorded[:, 27] == 3)][:, :13]
    assert len(two) == 1200
    real = _abc(tc, two)
    sure, plain = _rank(tc, real)
    assert not np.any(sure & ~plain)
    assert np.all(plain) and sure.sum() > 1000            # the shipped recording is full rank, and the guard sees it
    made = _abc(tc, _made_up_systems(rng, 200_000))
    sets = {"made up": made}
    # exact zeros: b = 0, a or c = 0, everything 0; exactly dependent columns (small integers: a c - b b == 0 exactly)
    z = made[:3000].copy()
    z[:1000, 1] = 0.0
    z[1000:2000, rng.integers(0, 2, 1000) * 2] = 0.0
    z[2000:2500] = 0.0
    q = rng.integers(1, 9, (500, 3)).astype(np.float64)
    kk = rng.choice([1.0, 2.0, -0.5], 500)
    z[2500:, 0], z[2500:, 1], z[2500:, 2] = (q * q).sum(1), kk * (q * q).sum(1), kk * kk * (q * q).sum(1)
    sets["zeros"] = z
    for e in (400, -400):
        sets[f"scaled 2^{e}"] = np.concatenate([real, made[:50_000]]) * 2.0 ** e
    # s * s overflows / a c overflows / ((a - c) / 2)^2 overflows while K s^2 would not; the guard's own arithmetic underflows
    big = np.concatenate([real, made[:20_000]])
    for e in (498, 500, 511, 520, 560, 600, 1000):
        sets[f"scaled 2^{e}"] = big * 2.0 ** e
    lop = big.copy()
    lop[:, 0] *= 2.0 ** 540
    lop[:, 1] *= 2.0 ** 520
    lop[:, 2] *= 2.0 ** 500
    sets["lopsided, large"] = lop
    for e in (-401, -402, -450, -500, -520, -1000):
        sets[f"scaled 2^{e}"] = big * 2.0 ** e
    nan = big[:3000].copy()
    nan[np.arange(3000), rng.integers(0, 3, 3000)] = np.nan
    sets["NaN"] = nan
    inf = big[:3000].copy()
    inf[np.arange(3000), rng.integers(0, 3, 3000)] = np.inf
    sets["inf"] = inf
    seen_sure = seen_unsure_true = seen_false = 0
    for name, abc in sets.items():
        with np.errstate(all="ignore"):
            sure, plain = _rank(tc, abc)
        assert not np.any(sure & ~plain), (name, abc[np.flatnonzero(sure & ~plain)[0]])
        with np.errstate(all="ignore"):
            s = abc[:, 0] + abc[:, 2]
        assert not np.any(sure & ~((s > 2.0 ** -401) & (s < 2.0 ** 498))), name
        if name in ("NaN", "inf", "lopsided, large") or name.endswith(("2^600", "2^1000", "2^-450", "2^-500", "2^-520", "2^-1000")):
            assert not np.any(sure), name                 # the guard's own arithmetic left its range: the exact branch
        seen_sure += int(sure.sum())
        seen_unsure_true += int((~sure & plain).sum())
        seen_false += int((~plain).sum())
    assert seen_sure > 100_000 and seen_unsure_true > 1000 and seen_false > 1000   # both branches, and both answers


def test_tr2_with_rank_guard_equals_plain(tc, recorded):
    rng = np.random.default_rng(3201)
    two = recorded[(recorded[:, 27] == 2) | (recorded[:, 27] == 3)][:, :13]
    made = _made_up_systems(rng, 30_000)
    scaled = []
    for e in (400, -400):   # Jh by 2^(e/2) scales a, b, c by 2^e
        s = np.concatenate([two, made[:5000]])
        s[:, :6] *= 2.0 ** (e // 2)
        s[:, 6:8] *= 2.0 ** e
        scaled.append(s)
    nan = made[:2000].copy()
    nan[np.arange(2000), rng.integers(0, 8, 2000)] = np.nan
    ops = np.ascontiguousarray(np.concatenate([two, made] + scaled + [nan]))
    first = ctypes.c_int64(-1)
    with np.errstate(all="ignore"):
        bad = tc.tc_tr2_compare(ops.ctypes.data_as(dp), len(ops), ctypes.byref(first))
    assert bad == 0, (bad, first.value, ops[first.value])
    sure, plain = _rank(tc, _abc(tc, ops))
    assert sure.sum() > 10_000 and (~sure).sum() > 5000 and (~plain).sum() > 1000


# ---- B: the xtol test on the squares ----------------------------------------------------------------------------------------
def _step_below(tc, S, T):
    S, T = np.ascontiguousarray(S, dtype=np.float64), np.ascontiguousarray(T, dtype=np.float64)
    plain, cut, br = (np.zeros(len(S), np.int32) for _ in range(3))
    tc.tc_step_below(S.ctypes.data_as(dp), T.ctypes.data_as(dp), len(S), plain.ctypes.data_as(ip), cut.ctypes.data_as(ip),
                     br.ctypes.data_as(ip))
    return plain, cut, br


def test_step_below_on_the_squares_equals_the_square_root(tc, recorded):
    rng = np.random.default_rng(6400)
    T = np.unique(recorded[:, 24])            # xtol (xtol + ||x||) of the run's own x
    assert len(T) > 1000 and np.all((T > 1e-16) & (T < 1e-6))
    T = np.concatenate([T, [1e-16, 1e-8 * (1e-8 + 1e-300)]])
    # S within +-64 ulp of fl(T T) ...
    base = bits(T * T).astype(np.int64)
    S = np.concatenate([(base + k).view(np.float64) for k in range(-64, 65)])
    TT = np.tile(T, 129)
    plain, cut, br = _step_below(tc, S, TT)
    assert np.array_equal(plain, cut)
    # (an ulp is 2^-53 .. 2^-52 of the value: the band of 2^-49 reaches 8 .. 16 ulp to either side)
    assert np.sum(br == 0) > 10_000 and np.sum(br == 1) > 10_000 and np.sum(br == 2) > 10_000   # all three outcomes
    k_of = np.repeat(np.arange(-64, 65), len(T))
    assert np.all(br[np.abs(k_of) <= 6] == 2) and np.all(br[np.abs(k_of) >= 20] != 2)
    # ... within 1e-13 of it (both sides of both band edges), and far away
    rel = np.concatenate([np.linspace(-1e-13, 1e-13, 2001), [-0.5, -1e-3, 1e-3, 1.0, 1e6]])
    S2 = (T[:, None] * T[:, None] * (1.0 + rel[None, :])).ravel()
    T2 = np.repeat(T, len(rel))
    plain2, cut2, br2 = _step_below(tc, S2, T2)
    assert np.array_equal(plain2, cut2)
    assert np.sum(br2 == 0) > 10_000 and np.sum(br2 == 1) > 10_000 and np.sum(br2 == 2) > 10_000   # all three outcomes
    assert np.all(plain2[br2 == 1] == 1) and np.all(plain2[br2 == 0] == 0)
    # the edges of the band themselves, +- 3 ulp
    for f in (1.0 - 2.0 ** -49, 1.0 + 2.0 ** -49):
        e = bits((T * T) * f).astype(np.int64)
        Se = np.concatenate([(e + k).view(np.float64) for k in range(-3, 4)])
        pe, ce, _ = _step_below(tc, Se, np.tile(T, 7))
        assert np.array_equal(pe, ce)
    # S of 0, subnormal, inf, NaN; T of inf, NaN, huge (T T overflows)
    Ss = np.array([0.0, -0.0, 5e-324, 1e-310, 2.2250738585072014e-308, 1e-40, 1.0, 1e300, np.inf, np.nan])
    Ts = np.concatenate([T[:5], [np.inf, np.nan, 2.0 ** 512, 2.0 ** 600, 1e-16]])
    S3, T3 = np.repeat(Ss, len(Ts)), np.tile(Ts, len(Ss))
    with np.errstate(all="ignore"):
        p3, c3, b3 = _step_below(tc, S3, T3)
    assert np.array_equal(p3, c3)
    small = (S3 < 1e-300) & np.isfinite(T3)
    assert np.all(b3[small] == 1) and np.all(c3[small] == 1)          # zero and underflowed sums: certainly below
    assert np.all(b3[np.isnan(S3) | np.isnan(T3)] == 2)               # NaN: the plain form
    assert np.all(b3[np.isinf(S3) & (T3 >= 2.0 ** 512)] == 2)


# ---- C: one unknown ---------------------------------------------------------------------------------------------------------
def test_norm_of_one_unknown_is_the_absolute_value(tc):
    rng = np.random.default_rng(12800)
    m = 1.0 + rng.random(4000)
    near = np.concatenate([(bits(np.array([1.0, 2.0])).astype(np.int64)[:, None] + np.arange(-40, 41)[None, :]).ravel()
                           .view(np.float64), np.sqrt(2.0) + np.arange(-40, 41) * 2.0 ** -52, m])
    xs = [np.ldexp(near, e) for e in range(-1074, 1024, 7)]          # every seventh binade, subnormals to the top
    xs += [np.ldexp(m[:64], e) for e in range(-1080, 1024)]          # all binades
    xs.append(np.array([0.0, 5e-324, 2.0 ** -537, 2.0 ** -511, 2.0 ** -510.5, 2.0 ** -510, 2.0 ** 511, 2.0 ** 511.9,
                        2.0 ** 512, 1.7976931348623157e308, np.inf, np.nan]))
    x = np.concatenate(xs)
    x = np.ascontiguousarray(np.concatenate([x, -x]))
    plain, cut, sf = np.zeros_like(x), np.zeros_like(x), np.zeros(len(x), np.int32)
    with np.errstate(all="ignore"):
        tc.tc_norm1(x.ctypes.data_as(dp), len(x), plain.ctypes.data_as(dp), cut.ctypes.data_as(dp), sf.ctypes.data_as(ip))
        sq = x * x
    assert np.all(same_bits(plain, cut)), x[np.flatnonzero(~same_bits(plain, cut))[:5]]
    assert np.all(same_bits(plain, np.sqrt(sq)))
    sf = sf.astype(bool)
    assert np.array_equal(sf, ((sq >= 2.0 ** -1021) & np.isfinite(sq)) | (x == 0.0))
    assert sf.sum() > 100_000 and (~sf).sum() > 50_000
    assert np.all(bits(cut[sf]) == bits(np.abs(x[sf])))
    # squares that underflow to a subnormal or to zero, and squares that overflow: the plain form ran
    assert not np.any(sf[(np.abs(x) > 0) & (np.abs(x) < 2.0 ** -511)]) and not np.any(sf[np.abs(x) >= 2.0 ** 512])
    assert not np.any(sf[np.isnan(x)])


# ---- E: the first multiplier -------------------------------------------------------------------------------------------------
def test_first_multiplier_without_its_square_root(tc):
    rng = np.random.default_rng(51200)
    au = np.concatenate([[0.0, -0.0, 5e-324, 1e-310, 1e-300, 1.0, 1e300, 1.7976931348623157e308, np.inf, -np.inf, np.nan, -1.0,
                          -1e-320], 10.0 ** rng.uniform(-30, 30, 5000)])
    au = np.ascontiguousarray(au)
    plain, cut = np.zeros_like(au), np.zeros_like(au)
    with np.errstate(all="ignore"):
        tc.tc_first_alpha(au.ctypes.data_as(dp), len(au), plain.ctypes.data_as(dp), cut.ctypes.data_as(dp))
    assert np.all(same_bits(plain, cut)), au[np.flatnonzero(~same_bits(plain, cut))[:5]]
    fin = np.isfinite(au) & (au > 0)
    assert np.all(bits(cut[fin]) == bits(0.001 * au[fin]))
    assert cut[au == np.inf][0] == np.inf and np.isnan(cut[np.isnan(au)][0])
    assert bits(cut[:2]).tolist() == bits(plain[:2]).tolist()   # the zero keeps alpha_upper's sign in both forms


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------
S_GPU, N_GPU = 70, 6   # per leg: one full wavefront and one of six lanes
SEEDS = dict(iid=909, still=909, narrow=909)


def _gpu_case(kind):
    from oracle import c_oracle
    from seqikpy_amd import data, synthetic, utils
    legs = data.LEGS
    body = utils.calculate_body_size(data.TEMPLATE_NMF_LOCOMOTION, legs)
    pose = synthetic.synthetic_pose(S_GPU, N_GPU, legs, data.BOUNDS_LOCOMOTION, body, data.TEMPLATE_NMF_LOCOMOTION,
                                    variant="iid", seed=SEEDS[kind])
    if kind == "still":       # the same pose in every frame: from the second frame on the steps are exactly zero or tiny
        pose = np.ascontiguousarray(np.broadcast_to(pose[:, :, :1], pose.shape))
    cases = []
    for leg in legs:
        seg, b, seeds = c_oracle.leg_params(leg, data.BOUNDS_LOCOMOTION, body, data.INITIAL_ANGLES_LOCOMOTION)
        b, seeds = b.copy(), seeds.copy()
        if kind == "narrow":  # limits 1e-8 apart on one joint of every stage: steps around the xtol threshold
            narrow_limits(b, seeds)
        cases.append((seg, b, seeds))
    return pose, cases


def _oracle_branch_stats(pose, cases):
    """The oracle's branch counters (its statistics build) over the input's own chains: [kind][counter], kind 0 = stage 1,
    kind 1 = stages 2 and 3; counter 1 = Gauss-Newton step inside the region, 3 = root loop entered, 6 = reflective calls."""
    odir = os.path.join(ROOT, "oracle")
    subprocess.check_call(["make", "-C", odir, "-s", "stats"])
    L = ctypes.CDLL(os.path.join(odir, "_build", "libseqik_oracle_stats.so"))
    L.oracle_seq_leg.restype = ctypes.c_int
    L.oracle_seq_leg.argtypes = [dp, ctypes.c_int64, dp, dp, dp, ctypes.c_int, ctypes.c_int, dp, dp, ip, ip, i64p, ip, dp]
    L.oracle_stats_reset.argtypes = [ctypes.c_int]
    L.oracle_stats_reset(1)
    n = pose.shape[2]
    for li, (seg, b, seeds) in enumerate(cases):
        seg, b, seeds = (np.ascontiguousarray(a, dtype=np.float64) for a in (seg, b, seeds))
        for s in range(pose.shape[0]):
            p = np.ascontiguousarray(pose[s, li], dtype=np.float64)
            ang, st, nf = np.zeros((n, 7)), np.zeros((n, 4), np.int32), np.zeros((n, 4), np.int32)
            ef, es = ctypes.c_int64(-1), ctypes.c_int32(-1)
            rc = L.oracle_seq_leg(p.ctypes.data_as(dp), n, seg.ctypes.data_as(dp), b.ctypes.data_as(dp), seeds.ctypes.data_as(dp),
                                  1, 4, ang.ctypes.data_as(dp), None, st.ctypes.data_as(ip), nf.ctypes.data_as(ip),
                                  ctypes.byref(ef), ctypes.byref(es), None)
            assert rc == 0
    out = (ctypes.c_longlong * 48)()
    L.oracle_stats_get(out)
    L.oracle_stats_reset(0)
    return np.array(list(out)).reshape(2, 24)


@functools.lru_cache(maxsize=None)
def _gpu_case_with_reference(kind):
    """pose, per-leg parameters and the C oracle's results for `kind`, computed once and shared read-only.  Before anything
    runs on the GPU the case shows, from the oracle alone, that its chains reach the branches the cuts changed."""
    pose, cases = _gpu_case(kind)
    ref = oracle_reference(pose, cases)
    st = _oracle_branch_stats(pose, cases)
    assert st[0, 6] > 0 and st[1, 6] > 0, st[:, 6]     # reflective calls, stage 1 and stages 2 / 3
    assert st[0, 3] + st[1, 3] > 0, st[:, 3]           # root loops entered (A's full-rank branch outside the region, E)
    assert st[1, 1] > 0, st[1, 1]                      # Gauss-Newton steps inside the region (A)
    status, nfev = ref["status"], ref["nfev"]
    if kind == "narrow":
        assert np.any((status == 3) | (status == 4)) and np.any(status == 2)   # both outcomes of the xtol test (B, C)
    if kind == "still":
        assert np.any((status == 1) & (nfev == 1))     # solves that end on their start point
    return pose, cases, ref


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(LAUNCH_PATHS))
@pytest.mark.parametrize("kind", ["iid", "still", "narrow"])
def test_launch_paths_equal_the_oracle_bit_for_bit(hiplib, kind, path):
    pose, cases, ref = _gpu_case_with_reference(kind)
    assert_equal_reference(solve_on_path(hiplib, pose, cases, ref, path), ref, path, n_chains=S_GPU * 6)
