"""The three per-pass cuts of csrc/seqik_core.hpp keep every bit.

  A. fd_step_wide: where a joint's limits are wide against the finite-difference step (StageConst::fd_wide, fd_limits_wide)
     _adjust_scheme_to_bounds' distance logic cannot fire and the step is `violated ? -h : h`;
  B. sincos_cw applies the quadrant signs by XOR into the sign bit;
  C. stage 1's end-effector evaluation with the identity prefix written out (residual_sc_stage1).

CPU tier: each short form against its general form / the oracle on the host (tests/harness/pass_path_harness.hip).
GPU tier: HIP == C oracle bit for bit on the smallest batch that has full and ragged wavefronts, through the fused kernel,
the chain queue, the staged launch and the stage pipeline, with shipped limits, with limits that clear the flag of part A,
and with limits / seeds of exactly 0 and open bounds."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT, LegParamsC
from harness_build import build_harness
from pass_cut_support import (assert_equal_reference, bits, leg_struct, narrow_limits,
                              oracle_reference, pin_seed, shipped_legs, solve_on_path)

dp = ctypes.POINTER(ctypes.c_double)
RSTEP = 2.0 ** -26


@pytest.fixture(scope="module")
def pp():
    lib = ctypes.CDLL(build_harness(os.path.join(ROOT, "tests", "harness", "pass_path_harness.hip")))
    lib.pp_sincos_mismatches.restype = ctypes.c_int64
    lib.pp_sincos_mismatches.argtypes = [ctypes.c_void_p, dp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    lib.pp_leg_consts.argtypes = [ctypes.POINTER(LegParamsC), dp, ctypes.POINTER(ctypes.c_int32)]
    lib.pp_fd_limits_wide.restype = ctypes.c_int32
    lib.pp_fd_limits_wide.argtypes = [ctypes.c_double, ctypes.c_double]
    lib.pp_fd_steps.argtypes = [dp, ctypes.c_int64, ctypes.c_double, ctypes.c_double, dp, dp]
    lib.pp_fd_jacobian.argtypes = [dp, dp, dp, ctypes.c_int32, dp]
    lib.pp_stage1_eval.argtypes = [ctypes.c_double] * 5 + [dp, dp, dp]
    return lib


def _leg_consts(pp, seg, bounds, seeds):
    out, flags = np.zeros((4, 2, 6)), np.zeros(4, np.int32)
    pp.pp_leg_consts(ctypes.byref(leg_struct(seg, bounds, seeds)), out.ctypes.data_as(dp),
                     flags.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    return out, flags


# ---- B: sincos_cw == oracle_sincos ------------------------------------------------------------------------------------------
def test_sincos_sign_bits_equal_the_oracle(oracle, pp):
    rng = np.random.default_rng(20250707)
    xs = [rng.uniform(-8.0, 8.0, 1_000_000), np.array([0.0, -0.0])]
    # every quadrant boundary in [-8, 8] (odd multiples of pi / 4, where rint(x * 2 / pi) steps) and every multiple of
    # pi / 2 (where the reduced argument changes sign), +- 4 ulp
    for k in range(-11, 12):
        for b in (np.float64(k) * (np.pi / 4),):
            near = [b]
            for _ in range(4):
                near.append(np.nextafter(near[-1], np.inf))
            lo = b
            for _ in range(4):
                lo = np.nextafter(lo, -np.inf)
                near.append(lo)
            xs.append(np.array(near))
    # the host constants of the six shipped legs: the points themselves ...
    consts = [_leg_consts(pp, *leg)[0] for leg in shipped_legs(oracle)]
    for c in consts:
        xs.append(c[:, :, [0, 3]].ravel())
    x = np.ascontiguousarray(np.concatenate(xs))
    first = ctypes.c_int64(-1)
    ref = ctypes.cast(oracle.lib().oracle_sincos, ctypes.c_void_p)
    bad = pp.pp_sincos_mismatches(ref, x.ctypes.data_as(dp), x.size, ctypes.byref(first))
    assert bad == 0, (bad, first.value, x[first.value] if first.value >= 0 else None)
    # ... and the stored sin / cos (StageConst::sc_lb / sc_ub, computed by make_leg_consts with the same routine)
    for c in consts:
        for st in range(4):
            for j in range(2):
                for o in (0, 3):
                    s, co = oracle.sincos(c[st, j, o])
                    assert bits([s, co]).tolist() == bits(c[st, j, o + 1:o + 3]).tolist()


# ---- A: fd_step_wide == fd_step wherever the flag is set ---------------------------------------------------------------------
def _fd_points(lb, ub):
    lo = lb if np.isfinite(lb) else (ub - 7.0 if np.isfinite(ub) else -7.0)
    hi = ub if np.isfinite(ub) else (lb + 7.0 if np.isfinite(lb) else 7.0)
    pts = [lo, hi, np.nextafter(lo, hi), np.nextafter(np.nextafter(lo, hi), hi), np.nextafter(hi, lo),
           np.nextafter(np.nextafter(hi, lo), lo)]
    if lo <= 0.0 <= hi:
        pts += [0.0, -0.0]
    grid = np.linspace(lo, hi, 4001)
    # ... and points within a few steps of either limit, where x + h leaves the limits
    edge = np.concatenate([lo + np.linspace(0, 4, 41) * RSTEP * max(1.0, abs(lo)), hi - np.linspace(0, 4, 41) * RSTEP * max(1.0, abs(hi))])
    x = np.concatenate([pts, grid, edge])
    return np.ascontiguousarray(x[(x >= lo) & (x <= hi)])


def _fd_both(pp, x, lb, ub):
    g, w = np.zeros_like(x), np.zeros_like(x)
    pp.pp_fd_steps(x.ctypes.data_as(dp), x.size, lb, ub, g.ctypes.data_as(dp), w.ctypes.data_as(dp))
    return g, w


def test_fd_step_wide_equals_fd_step_on_shipped_and_mirrored_limits(oracle, pp):
    pairs = set()
    for seg, b, seeds in shipped_legs(oracle):
        for lb, ub in b:
            pairs.add((float(lb), float(ub)))
            pairs.add((float(-ub), float(-lb)))   # the mirrored leg's limits
        _, flags = _leg_consts(pp, seg, b, seeds)
        assert flags.tolist() == [3, 3, 3, 3]     # every shipped stage takes the short form
    pairs.add((-np.pi, np.pi))                    # the claw link's limits
    assert len(pairs) >= 5
    flipped = 0
    for lb, ub in sorted(pairs):
        assert pp.pp_fd_limits_wide(lb, ub) == 1
        x = _fd_points(lb, ub)
        g, w = _fd_both(pp, x, lb, ub)
        assert np.array_equal(bits(g), bits(w)), (lb, ub)
        flipped += int(np.sum(np.signbit(g) != np.signbit(np.where(x >= 0, 1.0, -1.0))))
    assert flipped > 100   # the sign flip next to a limit was exercised


def test_fd_step_flag_threshold_and_infinite_bounds(pp):
    # made-up limits on either side of the threshold ub - lb >= 4 RSTEP max(1, |lb|, |ub|)
    for centre in (0.0, 0.3, -2.5, 40.0):
        m = max(1.0, abs(centre))
        thr = 4.0 * RSTEP * m
        for width, want in ((0.25 * thr, 0), (0.9 * thr, 0), (1.2 * thr, 1), (2.0 * thr, 1), (1e-8, 0), (1e-3, 1)):
            lb, ub = centre - width / 2, centre + width / 2
            assert pp.pp_fd_limits_wide(lb, ub) == want, (centre, width)
            x = _fd_points(lb, ub)
            g, w = _fd_both(pp, x, lb, ub)
            if want:
                assert np.array_equal(bits(g), bits(w)), (lb, ub)
            elif width <= RSTEP * m:
                # narrower than one step: the general routine's `!fitting` replacement fires and the short form would be
                # wrong -- which is why the flag must be clear here
                assert not np.array_equal(bits(g), bits(w)), (lb, ub)
    for lb, ub in ((-np.inf, 0.7), (-0.7, np.inf), (-np.inf, np.inf), (-np.inf, 0.0), (0.0, np.inf)):
        assert pp.pp_fd_limits_wide(lb, ub) == 1
        x = _fd_points(lb, ub)
        g, w = _fd_both(pp, x, lb, ub)
        assert np.array_equal(bits(g), bits(w)), (lb, ub)


def test_fd_jacobian_takes_the_general_routine_when_the_flag_is_clear(pp):
    """fd_jacobian with the stage's flag as run_stage forms it == fd_jacobian forced onto the general routine: wide limits
    (short form), one narrow joint (flag clear: general), points on and next to the limits."""
    rng = np.random.default_rng(5)
    for case in range(400):
        lb = rng.uniform(-2.0, 0.0, 2)
        ub = lb + rng.choice([1e-8, 3e-8, 1e-7, 0.5, 3.0], 2)
        if case % 7 == 0:
            ub[rng.integers(0, 2)] = np.inf
        u = rng.choice([0.0, 1.0, 1e-9, 1.0 - 1e-9, rng.random()], 2)
        x = lb + u * np.where(np.isfinite(ub), ub - lb, 1.0)
        x = np.clip(x, lb, ub)
        outs = []
        for general in (0, 1):
            J = np.zeros(6)
            pp.pp_fd_jacobian(x.ctypes.data_as(dp), lb.ctypes.data_as(dp), ub.ctypes.data_as(dp), general, J.ctypes.data_as(dp))
            outs.append(J)
        assert np.array_equal(bits(outs[0]), bits(outs[1])), (case, lb, ub, x)


# ---- C: stage 1's evaluation, closed form == general form, zero signs included ----------------------------------------------
def test_stage1_closed_form_equals_the_chain_product(pp):
    rng = np.random.default_rng(11)
    angles = [0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300, 1e-9, -1e-9]
    for q in range(4):                                  # one angle per quadrant and sign: all sign combinations of sin / cos
        angles += [q * np.pi / 2 + 0.4, -(q * np.pi / 2 + 0.4)]
    angles += list(rng.uniform(-np.pi, np.pi, 24))
    targets = [np.zeros(3), -np.zeros(3), np.array([0.3, -0.2, 0.9]), np.array([0.0, -0.0, -0.4])]
    n = 0
    seen = set()
    for xa in angles:
        for xb in angles:
            sa, ca, sb, cb = np.sin(xa), np.cos(xa), np.sin(xb), np.cos(xb)
            seen.add((np.signbit(sa), np.signbit(ca), np.signbit(sb), np.signbit(cb)))
            for tz in (-0.4, 0.4, -1e-3, 2.5):         # tz_last = -coxa length; both signs
                for tg in targets:
                    g, c = np.zeros(6), np.zeros(6)
                    pp.pp_stage1_eval(sa, ca, sb, cb, tz, np.ascontiguousarray(tg).ctypes.data_as(dp), g.ctypes.data_as(dp),
                                      c.ctypes.data_as(dp))
                    assert bits(g).tolist() == bits(c).tolist(), (xa, xb, tz, tg, g, c)
                    n += 1
    assert len(seen) == 16 and n > 20000


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------
S_GPU, N_GPU = 130, 8   # per leg: two full wavefronts and one of two lanes


def _gpu_case(kind):
    """(pose [S, 6, N, 5, 3], [(seg, bounds, seeds)] per leg) -- iid key points drawn inside the SHIPPED limits, solved with
    shipped limits ("base"), with a range of 1e-8 on one joint of every stage ("narrow": clears part A's flag) or with
    limits / seeds of exactly 0 and open bounds ("edge": zero sines in stage 1, infinite bounds)."""
    from oracle import c_oracle
    from seqikpy_amd import data, synthetic, utils
    legs = data.LEGS
    body = utils.calculate_body_size(data.TEMPLATE_NMF_LOCOMOTION, legs)
    pose = synthetic.synthetic_pose(S_GPU, N_GPU, legs, data.BOUNDS_LOCOMOTION, body, data.TEMPLATE_NMF_LOCOMOTION,
                                    variant="iid", seed=707)
    cases = []
    for li, leg in enumerate(legs):
        seg, b, seeds = c_oracle.leg_params(leg, data.BOUNDS_LOCOMOTION, body, data.INITIAL_ANGLES_LOCOMOTION)
        b, seeds = b.copy(), seeds.copy()
        if kind == "narrow":
            narrow_limits(b, seeds)
        elif kind == "edge":
            if li % 2 == 0:
                b[0] = (-np.pi, 0.0)   # ThC_yaw: upper limit exactly 0, seed 0 on it
            else:
                b[0] = (0.0, np.pi)    # ... lower limit exactly 0
            pin_seed(seeds, 0, 0.0)
            b[1] = (0.0, b[1][1]) if li < 3 else (b[1][0], 0.0)   # ThC_pitch: a limit of exactly 0, seed exactly 0
            pin_seed(seeds, 1, 0.0)
            b[2] = (-np.inf, b[2][1])                             # ThC_roll: one open bound
            b[4] = (b[4][0], np.inf) if li % 3 else (-np.inf, np.inf)
            pin_seed(seeds, 3, 0.0)                               # CTr_pitch seed exactly 0 (inside its limits)
        cases.append((seg, b, seeds))
    return pose, cases


@pytest.fixture(scope="module", params=["base", "narrow", "edge"])
def gpu_case(request):
    pose, cases = _gpu_case(request.param)
    return request.param, pose, cases, oracle_reference(pose, cases)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fused", "queue128", "staged", "staged_diag", "pipeline"])
def test_launch_paths_equal_the_oracle_bit_for_bit(hiplib, pp, gpu_case, path):
    kind, pose, cases, ref = gpu_case
    flags = [_leg_consts(pp, *c)[1].tolist() for c in cases]
    if kind == "narrow":
        assert all(f != 3 for fl in flags for f in fl)      # the general fd_step runs in every stage
    else:
        assert all(fl == [3, 3, 3, 3] for fl in flags)
    assert_equal_reference(solve_on_path(hiplib, pose, cases, ref, path), ref, path)
    if kind == "edge":
        # the zero-operand cases were reached: stage-1 angles that ended exactly on a limit of 0 were moved to +-2^-1074
        # or stayed 0, whose sine is a (signed) zero or the smallest subnormal
        assert np.sum(np.abs(ref["angles"][..., :2]) <= 5e-324) > 0
