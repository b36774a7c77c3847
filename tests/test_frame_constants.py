"""The two round-8 cuts of csrc/seqik_core.hpp keep every bit.

  bit 8   stages 2-4: the translation of the frame after the active links is a constant of the frame (StageProblem::t_act,
          stage_translation); the evaluations of a pass form only the third column of the rotation beside it
          (residual_sc<STAGE, true>), and the frame stored at a frame's end takes its translation from t_act;
  bit 16  solve_tr_2x2 keeps the Gauss-Newton step and its norm from the trust-region test for the first phi / ratio.

CPU tier: each short form against its plain form on the host, compared as integers (tests/harness/frame_const_harness.hip).
GPU tier: HIP == C oracle bit for bit on 70 sequences x 6 legs x 6 frames of iid key points (per leg one full wavefront and
one of six lanes; lanes start their frames in different passes, so a translation left over from another frame on any launch
path shows), through every launch path, with shipped limits and with a limit range of 1e-8 on one joint of every stage."""
import ctypes
import functools
import os

import numpy as np
import pytest

from conftest import ROOT, LegParamsC
from harness_build import build_harness
from pass_cut_support import (LAUNCH_PATHS, assert_equal_reference, first_pass_rows, leg_struct, narrow_limits,
                              oracle_reference, shipped_legs, solve_on_path)

dp = ctypes.POINTER(ctypes.c_double)
i64p = ctypes.POINTER(ctypes.c_int64)


@pytest.fixture(scope="module")
def fc():
    lib = ctypes.CDLL(build_harness(os.path.join(ROOT, "tests", "harness", "frame_const_harness.hip")))
    lib.fc_prefixes.restype = ctypes.c_int
    lib.fc_prefixes.argtypes = [ctypes.c_int32, ctypes.POINTER(LegParamsC), dp, ctypes.c_int64, dp, dp]
    lib.fc_compare.restype = ctypes.c_int
    lib.fc_compare.argtypes = [ctypes.c_int32, dp, dp, dp, dp, ctypes.c_int64, i64p, i64p]
    lib.fc_sincos.argtypes = [dp, ctypes.c_int64, dp]
    lib.fc_tr2_compare.restype = ctypes.c_int64
    lib.fc_tr2_compare.argtypes = [dp, ctypes.c_int64, i64p, ctypes.POINTER(ctypes.c_int32), dp, dp, i64p]
    return lib


# ---- bit 8: hoisted residual == general residual; frame at the frame's end ---------------------------------------------------
N_SETS = 24000   # operand sets per stage


def _sincos_pool(fc, rng):
    """sin / cos pairs: of random angles, of +-0, of the quadrant boundaries (the doubles next to k pi / 2 and those doubles'
    neighbours), and the exact values a boundary would have (zeros of both signs, +-1)."""
    x = [rng.uniform(-np.pi, np.pi, 400), np.array([0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300])]
    for k in range(-4, 5):
        b = np.float64(k) * (np.pi / 2)
        x.append(np.array([b, np.nextafter(b, np.inf), np.nextafter(b, -np.inf)]))
    x = np.ascontiguousarray(np.concatenate(x))
    sc = np.zeros((x.size, 2))
    fc.fc_sincos(x.ctypes.data_as(dp), x.size, sc.ctypes.data_as(dp))
    exact = np.array([[0.0, 1.0], [-0.0, 1.0], [1.0, 0.0], [1.0, -0.0], [-1.0, 0.0], [-1.0, -0.0], [0.0, -1.0], [-0.0, -1.0]])
    return np.concatenate([sc, exact])


def _operand_sets(fc, oracle, stage, rng):
    legs = shipped_legs(oracle)
    pres, tzs = [], []
    per_leg = 300
    for seg, b, seeds in legs:
        lb, ub = np.asarray(b)[:, 0], np.asarray(b)[:, 1]
        ang = np.ascontiguousarray(lb + rng.random((per_leg, 7)) * (ub - lb))       # random in-limit angles
        ang[:8, :] = np.where(rng.random((8, 7)) < 0.5, 0.0, -0.0)                 # ... and angles of +-0 where they are allowed
        ang[:8] = np.clip(ang[:8], lb, ub)
        pre, tz = np.zeros((per_leg, 12)), np.zeros(3)
        assert fc.fc_prefixes(stage, ctypes.byref(leg_struct(seg, b, seeds)), ang.ctypes.data_as(dp), per_leg,
                              pre.ctypes.data_as(dp), tz.ctypes.data_as(dp)) == 0
        pres.append(pre)
        tzs.append(np.broadcast_to(tz, (per_leg, 3)))
    pre, tz = np.concatenate(pres), np.concatenate(tzs)
    # the shipped segment lengths are what make_leg_consts put there (the active links carry 0 or -segment)
    assert np.all(tz[:, 2] < 0) and np.all((tz[:, :2] <= 0))
    # made-up prefixes: the identity, and real ones with exact zeros / negative zeros written into r and t
    ident = np.zeros((1, 12))
    ident[0, [0, 4, 8]] = 1.0
    zeroed = pre[rng.integers(0, len(pre), 600)].copy()
    mask = rng.random(zeroed.shape) < 0.35
    zeroed[mask] = np.where(rng.random(mask.sum()) < 0.5, 0.0, -0.0)
    pool_pre = np.concatenate([pre, ident, -ident, zeroed])
    pool_tz = np.concatenate([tz, tz[:2], tz[rng.integers(0, len(tz), 600)]])
    sc_pool = _sincos_pool(fc, rng)
    n = N_SETS
    pick = rng.integers(0, len(pool_pre), n)
    P, TZ = pool_pre[pick].copy(), pool_tz[pick].copy()
    # tz_a / tz_b of exactly 0 (either sign) beside the shipped ones
    z = rng.random(n)
    TZ[z < 0.15, 0] = 0.0
    TZ[(z >= 0.15) & (z < 0.3), 1] = 0.0
    TZ[(z >= 0.3) & (z < 0.35), :2] = -0.0
    # ... and a shipped segment length on either active link (stages 2 and 3 ship tz_a = 0, stage 4 has no link b)
    TZ[(z >= 0.35) & (z < 0.5), 0] = TZ[(z >= 0.35) & (z < 0.5), 2]
    TZ[(z >= 0.5) & (z < 0.65), 1] = TZ[(z >= 0.5) & (z < 0.65), 2]
    tg = rng.normal(0.0, 0.8, (n, 3))
    tg[rng.random(n) < 0.05] = 0.0
    tg[rng.random(n) < 0.05] = -0.0
    sc = np.concatenate([sc_pool[rng.integers(0, len(sc_pool), n)], sc_pool[rng.integers(0, len(sc_pool), n)]], axis=1)
    return [np.ascontiguousarray(a) for a in (P, TZ, tg, sc)]


@pytest.mark.parametrize("stage", [2, 3, 4])
def test_hoisted_residual_and_end_frame_equal_the_general_form(oracle, fc, stage):
    rng = np.random.default_rng(800 + stage)
    P, TZ, tg, sc = _operand_sets(fc, oracle, stage, rng)
    n = len(P)
    assert n >= 20000
    # the special operands are really in the sets
    assert np.sum(P == 0.0) > 1000 and np.sum(np.signbit(P) & (P == 0.0)) > 300
    assert np.sum(TZ[:, 0] == 0.0) > 1000 and np.sum(TZ[:, 1] == 0.0) > 1000
    assert np.sum(TZ[:, 0] < 0.0) > 1000 and np.sum(TZ[:, 1] < 0.0) > 1000
    assert np.sum(sc == 0.0) > 500 and np.sum(np.abs(sc) == 1.0) > 500
    bad = np.zeros(2, np.int64)
    first = ctypes.c_int64(-1)
    assert fc.fc_compare(stage, P.ctypes.data_as(dp), TZ.ctypes.data_as(dp), tg.ctypes.data_as(dp), sc.ctypes.data_as(dp), n,
                         bad.ctypes.data_as(i64p), ctypes.byref(first)) == 0
    k = first.value
    assert bad.tolist() == [0, 0], (bad, k, P[k], TZ[k], tg[k], sc[k])


# ---- bit 16: solve_tr_2x2 with the Gauss-Newton step kept == plain -----------------------------------------------------------
def _tr2(fc, ops):
    ops = np.ascontiguousarray(ops, dtype=np.float64)
    n = len(ops)
    counts, branch, gn, out = np.zeros(3, np.int64), np.zeros(n, np.int32), np.zeros(n), np.zeros((n, 3))
    first = ctypes.c_int64(-1)
    bad = fc.fc_tr2_compare(ops.ctypes.data_as(dp), n, counts.ctypes.data_as(i64p),
                            branch.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), gn.ctypes.data_as(dp), out.ctypes.data_as(dp),
                            ctypes.byref(first))
    return bad, first.value, counts, branch, gn, out


@pytest.fixture(scope="module")
def recorded_ops(fc):
    """First-pass operands of solve_tr_2x2 (stages 2 and 3, the full-rank two-unknown stages) from host runs of run_stage on
    the shipped recording, all six legs."""
    rows = first_pass_rows()
    ops = np.ascontiguousarray(rows[(rows[:, 27] == 2) | (rows[:, 27] == 3)][:, :13])
    assert len(ops) == 1200 and np.all(np.isfinite(ops))
    ops.setflags(write=False)
    return ops


def test_tr2_kept_step_equals_plain_on_recorded_operands(fc, recorded_ops):
    bad, first, counts, branch, gn, _ = _tr2(fc, recorded_ops)
    assert bad == 0, (bad, first, recorded_ops[first])
    assert counts.sum() == len(recorded_ops) == 1200
    assert counts[0] == 0   # stages 2 and 3 are full rank on the recording
    # later passes of a solve see the same matrices with a smaller radius and a warm multiplier: the recorded ones again
    # with Delta scaled by 2^-k and alpha warm
    rng = np.random.default_rng(16)
    total = np.zeros(3, np.int64)
    for k in range(1, 24):
        ops = recorded_ops.copy()
        ops[:, 11] *= 2.0 ** -k
        ops[:, 12] = np.where(rng.random(len(ops)) < 0.5, 0.0, 10.0 ** rng.uniform(-12, 2, len(ops)))
        bad, first, counts, *_ = _tr2(fc, ops)
        assert bad == 0, (k, bad, first, ops[first])
        total += counts
    assert total[1] > 500 and total[2] > 5000   # both full-rank branches, on real matrices


def test_tr2_kept_step_equals_plain_on_every_branch(fc, recorded_ops):
    rng = np.random.default_rng(1600)
    n = 4000
    made = np.zeros((n, 13))
    made[:, :6] = rng.normal(0.0, 1.0, (n, 6)) * 10.0 ** rng.uniform(-3, 1, (n, 1))
    made[:, 6:8] = np.where(rng.random((n, 2)) < 0.3, 0.0, 10.0 ** rng.uniform(-8, 0, (n, 2)))
    made[:, 8:11] = rng.normal(0.0, 0.5, (n, 3))
    made[:, 11] = 1.0
    base = np.concatenate([recorded_ops, made])
    _, _, counts, branch, gn, _ = _tr2(fc, base)
    full = base[branch > 0]
    gn = gn[branch > 0]
    assert len(full) > 4000 and np.all(gn > 0)

    def with_delta(delta, alpha=0.0):
        ops = full.copy()
        ops[:, 11] = delta
        ops[:, 12] = alpha
        return ops

    warm = 10.0 ** rng.uniform(-10, 3, len(full))
    cases = {
        "inside": (with_delta(gn * 4.0), 1),
        "on the radius": (with_delta(gn), 1),                                   # norm == Delta: still the Gauss-Newton step
        "one ulp outside": (with_delta(np.nextafter(gn, 0.0)), 2),              # norm one ulp above Delta
        "far outside": (with_delta(gn * 1e-6), 2),
        "Delta 1e-300": (with_delta(1e-300), 2),
        "Delta 1e300": (with_delta(1e300), 1),
        "warm alpha, outside": (with_delta(gn * 0.3, warm), 2),
        "warm alpha, inside": (with_delta(gn * 2.0, warm), 1),
    }
    # lmin under the rank threshold: collinear columns and no diagonal term (det = 0 or a rounding error of it)
    m = 500
    # (small integers times a power of two: a, b, c and a c - b b are exact, so the determinant is exactly 0)
    u = rng.integers(1, 9, (m, 3)) * rng.choice([-1.0, 1.0], (m, 3)) * 2.0 ** rng.integers(-6, 3, (m, 1))
    defi = np.zeros((m, 13))
    defi[:, 0:6:2] = u
    defi[:, 1:6:2] = u * rng.choice([0.0, 1.0, 2.0, -0.5], (m, 1))
    defi[:, 8:11] = rng.normal(0.0, 0.5, (m, 3))
    defi[:, 11] = 10.0 ** rng.uniform(-3, 1, m)
    defi[:, 12] = np.where(rng.random(m) < 0.5, 0.0, 10.0 ** rng.uniform(-6, 1, m))
    cases["rank deficient"] = (defi, 0)
    for name, (ops, want) in cases.items():
        bad, first, counts, branch, _, out = _tr2(fc, ops)
        assert bad == 0, (name, bad, first, ops[first])
        # the harness's own branch counters: every row of the case took the branch it was made for
        assert counts[want] == len(ops) and np.all(branch == want), (name, counts)
        if want == 1:
            assert np.all(out[:, 2] == 0.0)            # alpha_io is reset by the Gauss-Newton return
        if name in ("one ulp outside", "far outside", "warm alpha, outside"):
            step = np.hypot(out[:, 0], out[:, 1])
            assert np.allclose(step, ops[:, 11], rtol=1e-12, atol=0)   # the step was rescaled onto the radius


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------
S_GPU, N_GPU = 70, 6   # per leg: one full wavefront and one of six lanes


def _gpu_case(kind):
    from oracle import c_oracle
    from seqikpy_amd import data, synthetic, utils
    legs = data.LEGS
    body = utils.calculate_body_size(data.TEMPLATE_NMF_LOCOMOTION, legs)
    pose = synthetic.synthetic_pose(S_GPU, N_GPU, legs, data.BOUNDS_LOCOMOTION, body, data.TEMPLATE_NMF_LOCOMOTION,
                                    variant="iid", seed=808)
    cases = []
    for leg in legs:
        seg, b, seeds = c_oracle.leg_params(leg, data.BOUNDS_LOCOMOTION, body, data.INITIAL_ANGLES_LOCOMOTION)
        b, seeds = b.copy(), seeds.copy()
        if kind == "narrow":
            narrow_limits(b, seeds)
        cases.append((seg, b, seeds))
    return pose, cases


@functools.lru_cache(maxsize=None)
def _gpu_case_with_reference(kind):
    """pose, per-leg parameters and the C oracle's results for `kind`, computed once and shared read-only"""
    pose, cases = _gpu_case(kind)
    return pose, cases, oracle_reference(pose, cases)


# shipped limits through every launch path; the narrow limits (general fd_step, joints pinned between limits 1e-8 apart)
# once per kernel family
GPU_RUNS = [("base", p) for p in LAUNCH_PATHS] + [("narrow", p) for p in ("fused", "staged_diag", "pipeline")]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,path", GPU_RUNS)
def test_launch_paths_equal_the_oracle_bit_for_bit(hiplib, kind, path):
    pose, cases, ref = _gpu_case_with_reference(kind)
    assert_equal_reference(solve_on_path(hiplib, pose, cases, ref, path), ref, path, n_chains=S_GPU * 6)
