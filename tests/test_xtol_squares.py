"""The round-10 cut of csrc/seqik_core.hpp keeps every bit: bit 1024 of SEQIK_PASS_CUTS, the xtol test ||step|| < xtol (xtol +
||x||) of a pass decided from X = ||x||^2 and S = ||step||^2 (xtol_test) -- sure true below XTOL_SQ_LO X, sure false above
XTOL_SQ_HI X, for 2^-20 <= X < 2^100 -- without the root under ||x|| and without T.

CPU tier: the literals against exact arithmetic; the guarded and the plain decision on the host, with the branch taken
(tests/harness/xtol_squares_harness.hip), and every sure decision against a root that is 2 ulp off on the unfavourable side;
whole host runs of run_stage with and without the bit.  GPU tier: HIP == C oracle bit for bit on 70 sequences x 6 legs x 6
frames (per leg one full wavefront and one of six lanes) through every launch path, on three inputs; that the chains of
each input reach both outcomes of the xtol test is asserted first, from the oracle alone."""
import ctypes
import functools
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT, LegParamsC, load_golden
from harness_build import BUILD_DIR, build_harness
from pass_cut_support import (LAUNCH_PATHS, assert_equal_reference, bits, first_pass_rows, leg_struct, narrow_limits,
                              oracle_reference, solve_on_path)

dp = ctypes.POINTER(ctypes.c_double)
ip = ctypes.POINTER(ctypes.c_int32)
i64p = ctypes.POINTER(ctypes.c_int64)
HARNESS = os.path.join(ROOT, "tests", "harness", "xtol_squares_harness.hip")
XTOL = 1e-8


def _load(extra_flags=(), out_dir=None):
    # (-Bsymbolic: the two builds of the harness hold run_stage under the same names; each must call its own)
    lib = ctypes.CDLL(build_harness(HARNESS, out_dir, ("-Wl,-Bsymbolic", *extra_flags)))
    lib.xs_pass_cuts.restype = ctypes.c_int32
    lib.xs_constants.argtypes = [dp]
    lib.xs_xtol_test.argtypes = [dp, dp, ctypes.c_int64, ctypes.c_int32, ip, ip, ip, dp]
    lib.xs_run_chain.restype = ctypes.c_int
    lib.xs_run_chain.argtypes = [dp, ctypes.c_int64, ctypes.POINTER(LegParamsC), dp, dp, ip, ip]
    return lib


@pytest.fixture(scope="module")
def xs():
    lib = _load()
    assert lib.xs_pass_cuts() & 1024
    return lib


@pytest.fixture(scope="module")
def xs_without():
    lib = _load(("-DSEQIK_PASS_CUTS=1023",), os.path.join(BUILD_DIR, "pass_cuts_1023"))
    assert lib.xs_pass_cuts() == 1023
    return lib


def test_the_literals_are_what_the_argument_takes_them_for(xs):
    c = np.zeros(2)
    xs.xs_constants(c.ctypes.data_as(dp))
    lo, hi = Fraction(float(c[0])), Fraction(float(c[1]))
    sq = Fraction(XTOL) ** 2                      # of the double 1e-8, not of the real number
    assert float(c[0]) == float(sq * (1 - Fraction(1, 2 ** 40))) and float(c[1]) == float(sq * (1 + Fraction(1, 2 ** 14)))
    assert lo < sq * (1 - Fraction(1, 2 ** 41))
    assert hi > sq * (1 + Fraction(15, 16) * Fraction(1, 2 ** 14))      # 2^-14.1 = 0.933 x 2^-14
    assert abs(Fraction(XTOL) * 10 ** 8 - 1) < Fraction(1, 2 ** 54)


def _run(xs, X, step, na):
    X = np.ascontiguousarray(X, dtype=np.float64)
    step = np.ascontiguousarray(step, dtype=np.float64)
    assert step.shape == (len(X), 2)
    plain, cut, br = (np.zeros(len(X), np.int32) for _ in range(3))
    S = np.zeros(len(X))
    xs.xs_xtol_test(X.ctypes.data_as(dp), step.ctypes.data_as(dp), len(X), na, plain.ctypes.data_as(ip), cut.ctypes.data_as(ip),
                    br.ctypes.data_as(ip), S.ctypes.data_as(dp))
    return plain, cut, br, S


def _ulps(a, k):
    """the positive doubles a moved by k ulp each (a [n], k [m]) -> [n * m], a-major"""
    return (bits(a).astype(np.int64)[:, None] + np.asarray(k, np.int64)[None, :]).ravel().view(np.float64)


def _steps_for(S, na, rng):
    """steps whose sum of squares is the wanted S to within an ulp or two: one unknown as the root, two unknowns as a
    first component just short of the root and a second that makes up the difference under the fma"""
    S = np.asarray(S, dtype=np.float64)
    step = np.zeros((len(S), 2))
    sign = rng.choice([-1.0, 1.0], (len(S), 2))
    if na == 1:
        step[:, 0] = np.sqrt(S)
    else:
        step[:, 0] = np.sqrt(S) * (1.0 - rng.uniform(2.0 ** -30, 0.5, len(S)))
        step[:, 1] = np.sqrt(np.maximum(S - step[:, 0] * step[:, 0], 0.0))
    return step * sign


def _T(X):
    return XTOL * (XTOL + np.sqrt(X))      # (the host's root is IEEE's, as numpy's)


def _check_margins(X, S, br):
    """every sure decision against a square root that is 2 ulp off on the unfavourable side, on both sides of the comparison
    (what the device's sqrt_ is allowed; the oracle's is exact to half an ulp)"""
    def off(a, k):
        for _ in range(abs(k)):
            a = np.nextafter(a, np.inf if k > 0 else -np.inf)
        return a
    with np.errstate(all="ignore"):
        t, f = br == 1, br == 0
        assert np.all(off(np.sqrt(S[t]), 2) < XTOL * (XTOL + off(np.sqrt(X[t]), -2)))
        assert not np.any(off(np.sqrt(S[f]), -2) < XTOL * (XTOL + off(np.sqrt(X[f]), 2)))
        assert np.all((X[br != 2] >= 2.0 ** -20) & (X[br != 2] < 2.0 ** 100))


@pytest.mark.parametrize("na", [2, 1])
def test_decision_on_the_squares_equals_the_plain_form(xs, na):
    rng = np.random.default_rng(102400 + na)
    rows = first_pass_rows()
    # ||x||^2 of the run's own x (column 24 = xtol (xtol + ||x||)), and sizes up to both ends of the range
    X_rec = np.unique((rows[:, 24] / XTOL - XTOL) ** 2)[::8]
    assert len(X_rec) > 100 and np.all((X_rec >= 2.0 ** -20) & (X_rec < 2.0 ** 100))
    edges = np.array([2.0 ** -20, 2.0 ** 100])
    X_edge = np.concatenate([_ulps(edges, [-2, -1, 0, 1, 2]), [2.0 ** -21, 2.0 ** -19, 2.0 ** 99, 2.0 ** 101]])
    X_mid = 2.0 ** rng.uniform(-20, 100, 60)
    X = np.concatenate([X_rec, X_edge, X_mid])
    T2 = _T(X) ** 2
    seen = np.zeros(3, np.int64)
    seen_cut = np.zeros(2, np.int64)

    def check(Xs, Ss):
        step = _steps_for(Ss, na, rng)
        plain, cut, br, S = _run(xs, Xs, step, na)
        assert np.array_equal(plain, cut), (Xs[plain != cut][:3], S[plain != cut][:3])
        assert np.all(cut[br == 1] == 1) and np.all(cut[br == 0] == 0)
        _check_margins(Xs, S, br)
        seen[:] += np.bincount(br, minlength=3)
        seen_cut[:] += np.bincount(cut[br == 2], minlength=2)
        return br, S

    # S within +-64 ulp of T^2 (one unknown reaches every other ulp or so: its square moves by two per ulp of the step) ...
    k = np.arange(-64, 65)
    br, S = check(np.repeat(X, len(k)), _ulps(T2, k))
    assert np.all(br == 2)                   # next to T^2 itself: always the plain form
    # ... within 1e-4 relative of it: in range, both ends of that lie beyond the band (-1e-4 below c_lo X for every X, +1e-4
    # above c_hi X = T^2 (1 + 6.1e-5 - 2 xtol / ||x||))
    rel = np.concatenate([np.linspace(-1e-4, 1e-4, 801), [-0.5, -1e-3, 1e-3, 1.0, 1e6]])
    br, S = check(np.repeat(X, len(rel)), (T2[:, None] * (1.0 + rel[None, :])).ravel())
    in_range = np.repeat((X >= 2.0 ** -20) & (X < 2.0 ** 100), len(rel))
    rel_of = np.tile(rel, len(X))
    assert np.all(br[~in_range] == 2)
    assert np.all(br[in_range & (rel_of <= -0.99e-4)] == 1) and np.all(br[in_range & (rel_of >= 0.99e-4)] == 0)
    assert np.all(br[in_range & (rel_of >= 0.0) & (rel_of <= 2e-5)] == 2)
    # the edges of the band themselves, +-3 ulp
    c = np.zeros(2)
    xs.xs_constants(c.ctypes.data_as(dp))
    ok = (X >= 2.0 ** -20) & (X < 2.0 ** 100)
    for lit in c:
        check(np.repeat(X[ok], 7), _ulps(lit * X[ok], np.arange(-3, 4)))
    assert np.all(seen > 5000), seen           # all three outcomes: a guard that never fires cannot pass
    assert np.all(seen_cut > 1000), seen_cut   # and both answers of the plain form behind the guard


def test_zero_subnormal_infinite_and_nan(xs):
    tiny, big = 1e-170, 1e160                  # squares that underflow to zero / overflow; 1e-160 squares to a subnormal
    step = np.array([[0.0, 0.0], [-0.0, 0.0], [tiny, 0.0], [-tiny, tiny], [1e-160, 0.0], [2.0 ** -537, 0.0],
                     [1.4916681462400413e-154, 0.0], [big, 0.0], [-big, big], [1e200, 0.0], [np.inf, 0.0], [np.nan, 0.0],
                     [1e-9, 0.0], [1.0, 0.0]])
    Xs = np.array([0.0, 5e-324, 1e-310, 2.0 ** -21, 2.0 ** -20, 1.0, 7.5, 1e20, 2.0 ** 99, 2.0 ** 100, 1e300, np.inf, np.nan])
    for na in (2, 1):
        st = step.copy()
        if na == 2:
            st = np.concatenate([st, st[:, ::-1], [[1.0, np.nan], [np.nan, np.nan], [np.inf, np.inf]]])
        X = np.repeat(Xs, len(st))
        s = np.tile(st, (len(Xs), 1))
        with np.errstate(all="ignore"):
            plain, cut, br, S = _run(xs, X, s, na)
            assert np.array_equal(plain, cut), (X[plain != cut], s[plain != cut])
            _check_margins(X, S, br)
            in_range = (X >= 2.0 ** -20) & (X < 2.0 ** 100)
            assert np.all(br[~in_range] == 2)                                  # NaN, inf, zero, out of range: plain
            assert np.all(br[np.isnan(S)] == 2)
            under = in_range & (S < 2.0 ** -1022)                              # zero and underflowed squares: sure true
            over = in_range & np.isinf(S)                                      # overflowed squares: sure false
            assert under.sum() >= 30 and over.sum() >= 20
            assert np.all(br[under] == 1) and np.all(cut[under] == 1)
            assert np.all(br[over] == 0) and np.all(cut[over] == 0)
            # stage 4 compares |step0| with T where the square is normal, the root of the square elsewhere: the same
            # answer as the oracle's root of the square everywhere
            if na == 1:
                assert np.array_equal(cut == 1, np.sqrt(S) < _T(X))


def test_first_pass_steps_of_the_recording(xs):
    rows = first_pass_rows()
    X = (rows[:, 24] / XTOL - XTOL) ** 2
    step = rows[:, 15:17] * rows[:, 25:27]      # d p_h: the first trial step of every solve
    for na, sel in ((2, rows[:, 27] < 4), (1, rows[:, 27] == 4)):
        plain, cut, br, S = _run(xs, X[sel], step[sel], na)
        assert np.array_equal(plain, cut)
        _check_margins(X[sel], S, br)
        assert np.mean(br != 2) > 0.99          # a real pass is decided on the squares


def _host_run(lib, pose, lp):
    n = len(pose)
    ang, fk = np.zeros((n, 7)), np.zeros((n, 27))
    st, nf = np.zeros((n, 4), np.int32), np.zeros((n, 4), np.int32)
    rc = lib.xs_run_chain(pose.ctypes.data_as(dp), n, ctypes.byref(lp), ang.ctypes.data_as(dp), fk.ctypes.data_as(dp),
                          st.ctypes.data_as(ip), nf.ctypes.data_as(ip))
    assert rc == 0
    return ang, fk, st, nf


def test_run_stage_on_the_host_with_and_without_the_bit(xs, xs_without):
    z = load_golden("df3d_100")
    for leg in [str(l) for l in z["legs"]]:
        pose = np.ascontiguousarray(z[f"{leg}_pose"], dtype=np.float64)
        lp = leg_struct(z[f"{leg}_seg"], z[f"{leg}_bounds"], z[f"{leg}_seeds"])
        new, old = _host_run(xs, pose, lp), _host_run(xs_without, pose, lp)
        assert np.array_equal(bits(new[0]), bits(old[0])) and np.array_equal(bits(new[1]), bits(old[1])), leg
        assert np.array_equal(new[2], old[2]) and np.array_equal(new[3], old[3]), leg
        assert np.all(new[3] > 0) and np.any(new[2] > 1)   # solves ran, and some ended on the ftol / xtol tests


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------
S_GPU, N_GPU = 70, 6   # per leg: one full wavefront and one of six lanes
SEED = 1010


def _gpu_case(kind):
    from oracle import c_oracle
    from seqikpy_amd import data, synthetic, utils
    legs = data.LEGS
    body = utils.calculate_body_size(data.TEMPLATE_NMF_LOCOMOTION, legs)
    pose = synthetic.synthetic_pose(S_GPU, N_GPU, legs, data.BOUNDS_LOCOMOTION, body, data.TEMPLATE_NMF_LOCOMOTION,
                                    variant="iid", seed=SEED)
    if kind == "still":       # the same pose in every frame: steps that shrink through the band's neighbourhood
        pose = np.ascontiguousarray(np.broadcast_to(pose[:, :, :1], pose.shape))
    cases = []
    for leg in legs:
        seg, b, seeds = c_oracle.leg_params(leg, data.BOUNDS_LOCOMOTION, body, data.INITIAL_ANGLES_LOCOMOTION)
        b, seeds = b.copy(), seeds.copy()
        if kind == "narrow":  # limits 1e-8 apart on one joint of every stage: steps around the xtol threshold
            narrow_limits(b, seeds)
        cases.append((seg, b, seeds))
    return pose, cases


def _oracle_trial_counts(pose, cases):
    """From the oracle's statistics build over the input's own chains: reflective calls of stage 1 and of stages 2 / 3 (trial
    steps, each followed by one xtol test)"""
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
    return np.array(list(out)).reshape(2, 24)[:, 6]


@functools.lru_cache(maxsize=None)
def _gpu_case_with_reference(kind):
    """pose, per-leg parameters and the C oracle's results for `kind`, computed once and shared read-only.  Before anything
    runs on the GPU the case shows, from the oracle alone, that its chains take trial steps in every stage and that the
    xtol test comes out both ways: every trial step of every chain runs xtol_test, a solve that ends by status 3 / 4 had it
    true, one that ends by status 2 or goes on after a trial had it false."""
    pose, cases = _gpu_case(kind)
    ref = oracle_reference(pose, cases)
    trials = _oracle_trial_counts(pose, cases)
    assert trials[0] > 0 and trials[1] > 0, trials
    status, nfev = ref["status"], ref["nfev"]
    # trials that did not end the solve: in every stage, except that a stage whose only joint is held between limits 1e-8
    # apart may end every solve on its first trial
    assert np.all(np.any(nfev > 2, axis=(0, 1, 2))[:3 if kind == "narrow" else 4])
    if kind in ("narrow", "still"):
        assert np.any((status == 3) | (status == 4))           # the xtol test true
    assert np.any(status == 2)                                 # ... and false where the ftol test was true
    return pose, cases, ref


PATHS = [p for p in LAUNCH_PATHS]   # fused, queue128, staged (+ diagnostics), pipeline, exact frame chunks, stage subsets


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("kind", ["iid", "still", "narrow"])
def test_launch_paths_equal_the_oracle_bit_for_bit(hiplib, kind, path):
    pose, cases, ref = _gpu_case_with_reference(kind)
    assert_equal_reference(solve_on_path(hiplib, pose, cases, ref, path), ref, path, n_chains=S_GPU * 6)
