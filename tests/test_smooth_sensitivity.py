"""Error bars of the smoothed trajectory (include/seqik_smooth_sensitivity.h): the C ABI's refusals, the header against the
ninth signature table, the rule's identities by ``==`` on the host-run rule (against seqik_refine_sensitivity where the
frames do not couple, halves against the whole, a batch against its trajectories, one half_width inside another, held
rows, zero weights, the bad-sigma bit), the Python surface through a stand-in for ``_lib._call``, and on the GPU every
output of the kernels against the host-run rule bit for bit.  The accuracy of the linear part and of the whole rule:
tests/test_smooth_sensitivity_accuracy.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from angle_map_support import gpu_lib
from conftest import DOFS, ROOT, load_golden
from refine_sens_support import refine_sens_harness  # noqa: F401
from smooth_sens_support import (BAD_INPUT, BAD_SIGMA, NOT_PD, GPU_FRAMES, GPU_WIDTHS, SUBSETS, check_device_against_host,  # noqa: F401
                                 gpu_case, harness_call, same_bits, smooth_sens_harness, smoothed_window)
from smooth_support import harness_call as smooth_call
from smooth_support import shipped_window, smooth_harness  # noqa: F401
from test_capi_symbols import assert_same_class, header_prototypes

SYMBOLS = ["seqik_smooth_sensitivity", "seqik_smooth_sensitivity_device", "seqik_smooth_sensitivity_workspace_bytes"]
QNAN = np.uint64(0x7FF8000000000000)
HEADER = "seqik_smooth_sensitivity.h"


def only_the_one_nan(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return (a.view(np.uint64)[np.isnan(a)] == QNAN).all()


def positive_zero(a):
    return not np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).any()


# ---------------------------------------------------------------------------------------------------------------------
# CPU tier
# ---------------------------------------------------------------------------------------------------------------------

def test_header_declares_exactly_the_new_entry_points(hiplib):
    raw = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "ALLOCATES NOTHING AND WAITS FOR NOTHING" in raw and "captured into a graph" in raw
    assert "1364 bytes per leg-frame" in raw and "NOT of H^-1" in raw
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(seqik_[a-z_]+)\s*\(", text)))
    assert declared == sorted(SYMBOLS)
    assert sorted(hiplib.SMOOTH_SENS_SIGNATURES) == [HEADER]
    assert hiplib.SMOOTH_SENS_EXPORTED_SYMBOLS == [s[0] for s in hiplib.SMOOTH_SENS_SIGNATURES[HEADER]]
    assert sorted(hiplib.SMOOTH_SENS_EXPORTED_SYMBOLS) == declared
    # a ninth table: disjoint from the other eight, which keep their headers
    tables = (hiplib.SIGNATURES, hiplib.EXTENSION_SIGNATURES, hiplib.STREAM_GAPS_SIGNATURES, hiplib.JACOBIAN_SIGNATURES,
              hiplib.SENSITIVITY_SIGNATURES, hiplib.REFINE_SIGNATURES, hiplib.SMOOTH_SIGNATURES,
              hiplib.REFINE_SENS_SIGNATURES)
    assert not set(declared) & {s[0] for table in tables for sigs in table.values() for s in sigs}
    assert all(HEADER not in table for table in tables) and len(hiplib.SIGNATURES) == 6
    lib = hiplib.load()
    assert lib.seqik_abi_version() == 7 == hiplib.ABI_VERSION
    assert "seqik_smooth_sens.hip" in hiplib.COMPILE_UNITS and "seqik_smooth_sens.hpp" in hiplib.CSRC_HEADERS
    assert "seqik_smooth_sens" not in " ".join(hiplib.KERNEL_SOURCES + hiplib.LATENCY_SOURCES)
    assert f'"{HEADER}"' in open(os.path.join(ROOT, "setup.py")).read()
    assert "#define SEQIK_SMOOTHSENS_FLAG_NOT_PD (1 << 8)\n" in raw and hiplib.SMOOTH_SENS_FLAG_NOT_PD == NOT_PD
    assert "#define SEQIK_SMOOTHSENS_FLAG_BAD_INPUT (1 << 16)\n" in raw and hiplib.SMOOTH_SENS_FLAG_BAD_INPUT == BAD_INPUT
    assert "#define SEQIK_SMOOTHSENS_FLAG_BAD_SIGMA (1 << 17)\n" in raw and hiplib.SMOOTH_SENS_FLAG_BAD_SIGMA == BAD_SIGMA
    assert "#define SEQIK_SMOOTHSENS_MAX_HALF_WIDTH 32\n" in raw and hiplib.SMOOTH_SENS_MAX_HALF_WIDTH == 32
    protos = header_prototypes(HEADER)
    table = {sig[0]: sig[1:] for sig in hiplib.SMOOTH_SENS_SIGNATURES[HEADER]}
    assert sorted(table) == sorted(protos) == declared
    counts = dict(zip(SYMBOLS, (17, 19, 4)))
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name][0], list(table[name][1:])
        assert len(argtypes) == len(params) == counts[name], (name, params)
        assert_same_class(ret, restype, False, name)
        for p, a in zip(params, argtypes):
            assert_same_class(p, a, True, name)
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_bad_arguments_are_refused_before_anything_touches_hip(hiplib):
    """Every SEQIK_ERR_BAD_ARG case of the header, raised on a machine without a GPU, by both entry points and by the
    workspace query; a call with no leg-frames returns OK without a launch."""
    lib = hiplib.load()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    ang, pose, sig = np.zeros((1, 2, 3, 7)), np.zeros((1, 2, 3, 5, 3)), np.ones((1, 2, 3, 4))
    out, flg = np.zeros((1, 2, 3, 5 * 84)), np.zeros((1, 2, 3), np.int32)
    a, p, g, o, f = (ang.ctypes.data_as(dp), pose.ctypes.data_as(dp), sig.ctypes.data_as(dp), out.ctypes.data_as(dp),
                     flg.ctypes.data_as(ip))
    sm = lambda *v: (ctypes.c_double * 7)(*v)  # noqa: E731
    ok_s, neg_s, nan_s, inf_s = sm(*[0.1] * 7), sm(0.1, 0.1, -1e-9, 0.1, 0.1, 0.1, 0.1), sm(*[np.nan] * 7), sm(0, 0, 0, 0, 0, 0, np.inf)
    good = (hiplib.SeqikLegParams * 2)()
    for l in range(2):
        for i in range(4):
            good[l].seg[i] = 0.5
    bad_seg = (hiplib.SeqikLegParams * 2)()
    bad_seg[1].seg[2] = np.inf
    huge = 2 ** 63 // (8 * 84) + 1
    t = 1e-6
    #        angles pose n_seq n_legs n_frames legs kind kp_weight kp_sigma smooth tol W sens std grad flags
    cases = [("n_legs", (a, p, 1, 0, 3, good, 0, None, None, ok_s, t, 0, o, None, None, None)),
             ("n_legs", (a, p, 1, 9, 3, good, 0, None, None, None, t, 0, o, None, None, None)),
             ("negative", (a, p, -1, 2, 3, good, 0, None, None, ok_s, t, 0, o, None, None, None)),
             ("negative", (a, p, 1, 2, -3, good, 0, None, None, ok_s, t, 0, o, None, None, None)),
             ("angles", (None, p, 1, 2, 3, good, 0, None, None, ok_s, t, 0, o, None, None, None)),
             ("pose", (a, None, 1, 2, 3, good, 0, None, None, ok_s, t, 0, o, None, None, None)),
             ("legs", (a, p, 1, 2, 3, None, 0, None, None, ok_s, t, 0, o, None, None, None)),
             ("no output", (a, p, 1, 2, 3, good, 0, None, None, ok_s, t, 0, None, None, None, None)),
             ("no output", (a, p, 1, 2, 3, good, 0, g, g, None, t, 2, None, None, None, None)),
             ("std needs kp_sigma", (a, p, 1, 2, 3, good, 0, None, None, ok_s, t, 0, o, o, None, None)),
             ("std needs kp_sigma", (a, p, 1, 2, 3, good, 0, g, None, ok_s, t, 0, None, o, o, f)),
             ("generic chain", (a, p, 1, 2, 3, good, 1, None, None, ok_s, t, 0, o, None, None, None)),
             ("generic chain", (a, p, 1, 2, 3, good, 1, None, g, None, t, 1, None, o, None, f)),
             ("kind", (a, p, 1, 2, 3, good, 2, None, None, ok_s, t, 0, o, None, None, None)),
             ("kind", (a, p, 1, 2, 3, good, -1, None, None, ok_s, t, 0, None, None, None, f)),
             ("segment", (a, p, 1, 2, 3, bad_seg, 0, None, None, ok_s, t, 0, o, None, None, None)),
             ("bound_tol", (a, p, 1, 2, 3, good, 0, None, None, ok_s, -1e-6, 0, o, None, None, None)),
             ("bound_tol", (a, p, 1, 2, 3, good, 0, None, None, ok_s, np.nan, 0, None, None, o, None)),
             ("bound_tol", (a, p, 1, 2, 3, good, 0, None, None, ok_s, np.inf, 0, None, None, None, f)),
             ("smooth", (a, p, 1, 2, 3, good, 0, None, None, neg_s, t, 0, o, None, None, None)),
             ("smooth", (a, p, 1, 2, 3, good, 0, None, g, nan_s, t, 0, None, o, None, None)),
             ("smooth", (a, p, 1, 2, 3, good, 0, None, None, inf_s, t, 2, None, None, None, f)),
             ("half_width", (a, p, 1, 2, 3, good, 0, None, None, ok_s, t, -1, o, None, None, None)),
             ("half_width", (a, p, 1, 2, 3, good, 0, None, None, ok_s, t, 33, o, None, None, None)),
             ("half_width", (a, p, 1, 2, 3, good, 0, None, g, None, t, 2 ** 31 - 1, None, o, None, f)),
             ("too many", (a, p, huge, 1, 1, good, 0, None, None, ok_s, t, 0, o, None, None, None)),
             ("too many", (a, p, 1, 1, huge, good, 0, None, None, ok_s, t, 0, None, None, None, f)),
             ("too many", (a, p, 2 ** 40, 2, 2 ** 40, good, 0, None, None, ok_s, t, 0, None, None, o, None)),
             ("too many", (a, p, huge // 60, 1, 1, good, 0, None, None, ok_s, t, 32, o, None, None, None))]
    ws = np.zeros(16 * 1024, dtype=np.uint8)
    w = ws.ctypes.data_as(ctypes.c_void_p)
    for what, args in cases:
        for fn, last in ((lib.seqik_smooth_sensitivity, (-1,)), (lib.seqik_smooth_sensitivity_device, (w, ws.nbytes, None))):
            assert fn(*args, *last) == hiplib.ERR_ARG, (what, fn.__name__)
            msg = lib.seqik_last_error().decode()
            assert msg.startswith("seqik_smooth_sensitivity: ") and what.split()[0] in msg, (what, msg)
    # the workspace: its size, and the device entry's refusals of one that is null, short or misaligned
    need = lib.seqik_smooth_sensitivity_workspace_bytes(1, 2, 3, 0)
    assert 6 * 1364 <= need <= 6 * 1364 + 11 * 256 and need == hiplib.smooth_sensitivity_workspace_bytes(1, 2, 3)
    assert lib.seqik_smooth_sensitivity_workspace_bytes(1, 2, 3, 32) == need      # (it does not depend on half_width)
    assert lib.seqik_smooth_sensitivity_workspace_bytes(0, 2, 3, 0) == 0
    for bad in ((1, 0, 3, 0), (1, 9, 3, 0), (-1, 2, 3, 0), (1, 2, -3, 0), (1, 2, 3, -1), (1, 2, 3, 33), (huge, 1, 1, 0)):
        assert lib.seqik_smooth_sensitivity_workspace_bytes(*bad) == -1
        assert lib.seqik_last_error().decode().startswith("seqik_smooth_sensitivity: ")
        with pytest.raises(ValueError):
            hiplib.smooth_sensitivity_workspace_bytes(*bad)
    fine = (a, p, 1, 2, 3, good, 0, None, None, ok_s, t, 0, o, None, None, None)
    wa = ws.ctypes.data
    for what, tail in (("workspace is null", (None, need, None)), ("workspace is null", (w, need - 1, None)),
                       ("workspace is null", (w, 0, None)), ("8-byte aligned", (ctypes.c_void_p(wa + 4), need, None))):
        assert lib.seqik_smooth_sensitivity_device(*fine, *tail) == hiplib.ERR_ARG
        assert what in lib.seqik_last_error().decode()
    for args in ((a, p, 0, 2, 3, good, 0, None, None, ok_s, t, 0, o, None, o, f), (a, p, 1, 2, 0, good, 0, g, g, None, 0.0, 2, o, o, o, f)):
        assert lib.seqik_smooth_sensitivity(*args, -1) == 0
        assert lib.seqik_smooth_sensitivity_device(*args, None, 0, None) == 0     # (no leg-frames: no workspace is needed)
    assert not out.any() and not flg.any()
    # the Python wrappers: shapes and arguments
    params = [hiplib.leg_params_from_arrays(np.full(4, 0.5), np.zeros((7, 2)), np.zeros(27))] * 2
    with pytest.raises(ValueError, match="no output"):
        hiplib.smooth_sensitivity(ang, pose, params, want_sens=False, want_grad=False, want_flags=False)
    with pytest.raises(ValueError, match="std needs kp_sigma"):
        hiplib.smooth_sensitivity(ang, pose, params, want_std=True)
    with pytest.raises(ValueError, match="pose must have shape"):
        hiplib.smooth_sensitivity(ang, pose[..., :4, :], params)
    with pytest.raises(ValueError, match="kp_sigma must broadcast"):
        hiplib.smooth_sensitivity(ang, pose, params, kp_sigma=np.ones(3))
    with pytest.raises(ValueError, match="kp_weight must broadcast"):
        hiplib.smooth_sensitivity(ang, pose, params, kp_weight=np.ones(3))
    with pytest.raises(ValueError, match="half_width must lie in"):
        hiplib.smooth_sensitivity(ang, pose, params, half_width=33)
    with pytest.raises(ValueError, match="smooth must be a scalar"):
        hiplib.smooth_sensitivity(ang, pose, params, smooth=np.ones(3))
    with pytest.raises(ValueError, match="smooth must be finite"):
        hiplib.smooth_sensitivity(ang, pose, params, smooth=-1.0)


def test_uncoupled_frames_have_the_bits_of_refine_sensitivity(smooth_sens_harness, refine_sens_harness, smooth_harness):  # noqa: F811
    """smooth all zero, and N = 1 at any smooth: the offset-0 sens, std, grad and flags of seqik_refine_sensitivity, at
    every half_width; the off-centre blocks are +0.0."""
    for leg, lo, hi in (("RF", 272, 296), ("LF", 276, 308)):
        q, pose, seg, bounds = smoothed_window(smooth_harness, leg, lo, hi)
        sigma = np.random.default_rng(5).uniform(0.005, 0.05, (len(q), 4))
        ref = refine_sens_harness.run(q, pose, seg, bounds, kp_sigma=sigma)
        # (the smoothed angles are no minimum of the per-frame fit: some of its Hessians are not positive definite there, and
        # without coupling this rule says the same, frame by frame)
        assert not (ref["flags"] & BAD_INPUT).any()
        for W in (0, 3):
            got = smooth_sens_harness.run_one(q, pose, seg, bounds, smooth=0.0, kp_sigma=sigma, half_width=W)
            assert same_bits(got["sens"][:, W], ref["sens"]) and same_bits(got["std"], ref["std"])
            assert same_bits(got["grad"], ref["grad"]) and np.array_equal(got["flags"], ref["flags"])
            assert positive_zero(np.delete(got["sens"], W, axis=1))
        for t in (0, 7, len(q) - 1):       # N = 1: no pair, whatever smooth
            one = smooth_sens_harness.run_one(q[t:t + 1], pose[t:t + 1], seg, bounds, smooth=3.0, kp_sigma=sigma[t:t + 1],
                                              half_width=2)
            assert same_bits(one["sens"][0, 2], ref["sens"][t]) and same_bits(one["std"][0], ref["std"][t])
            assert same_bits(one["grad"][0:1], ref["grad"][t:t + 1]) and one["flags"][0] == ref["flags"][t]
            assert positive_zero(one["sens"][0, [0, 1, 3, 4]])
        # and the penalty does change the answer
        on = smooth_sens_harness.run_one(q, pose, seg, bounds, smooth=0.1, kp_sigma=sigma)
        assert not same_bits(on["sens"][:, 0], ref["sens"]) and np.isfinite(on["std"]).all()


def test_identities_of_the_rule(smooth_sens_harness, smooth_harness):  # noqa: F811
    q, pose, seg, bounds = smoothed_window(smooth_harness, "RF", 272, 296)
    q2, pose2, seg2, bounds2 = smoothed_window(smooth_harness, "LF", 276, 300)
    N = len(q)
    sigma = np.random.default_rng(6).uniform(0.005, 0.05, (N, 4))
    run = smooth_sens_harness.run_one
    w5 = run(q, pose, seg, bounds, kp_sigma=sigma, half_width=5)
    w2 = run(q, pose, seg, bounds, kp_sigma=sigma, half_width=2)
    w0 = run(q, pose, seg, bounds, kp_sigma=sigma, half_width=0)
    assert not (w5["flags"] & ~0x7F).any() and np.isfinite(w5["sens"]).all() and only_the_one_nan(w5["sens"])
    # the sens of W = 2 is the middle of the sens of W = 5; std, grad and flags do not depend on W
    assert same_bits(w2["sens"], w5["sens"][:, 3:8]) and same_bits(w0["sens"], w5["sens"][:, 5:6])
    for k in ("std", "grad"):
        assert same_bits(w0[k], w5[k]) and same_bits(w2[k], w5[k])
    assert np.array_equal(w0["flags"], w5["flags"]) and np.array_equal(w2["flags"], w5["flags"])
    # blocks whose source lies outside 0..N-1 are +0.0, the others are not zero
    for t in range(N):
        for d in range(11):
            inside = 0 <= t + d - 5 < N
            assert positive_zero(w5["sens"][t, d]) != inside, (t, d)
    # the coupling stiffens: the smoothed angles answer less to their own frame's noise than the same rule without penalty
    free = (w0["flags"][:, None] >> np.arange(7)) & 1 == 0
    loose = run(q, pose, seg, bounds, smooth=0.0, kp_sigma=sigma)
    free &= np.isfinite(loose["std"]) & ((loose["flags"][:, None] >> np.arange(7)) & 1 == 0)
    assert free.sum() > 7 * N // 2 and np.median(w0["std"][free] / loose["std"][free]) < 1.0
    # a bad frame in the middle: the bits of the two halves run alone
    for t_bad, how in ((11, "angle"), (12, "pose")):
        qb, pb = q.copy(), pose.copy()
        if how == "angle":
            qb[t_bad, 3] = np.nan
        else:
            pb[t_bad, 2, 1] = np.inf
        whole = run(qb, pb, seg, bounds, kp_sigma=sigma, half_width=3)
        first = run(qb[:t_bad], pb[:t_bad], seg, bounds, kp_sigma=sigma[:t_bad], half_width=3)
        second = run(qb[t_bad + 1:], pb[t_bad + 1:], seg, bounds, kp_sigma=sigma[t_bad + 1:], half_width=3)
        for k in ("sens", "std", "grad"):
            assert same_bits(whole[k][:t_bad], first[k]) and same_bits(whole[k][t_bad + 1:], second[k]), (k, how)
            assert np.isnan(whole[k][t_bad]).all() and only_the_one_nan(whole[k])
        assert np.array_equal(whole["flags"][:t_bad], first["flags"]) and whole["flags"][t_bad] == BAD_INPUT
        assert np.array_equal(whole["flags"][t_bad + 1:], second["flags"])
        # ... and it differs from the run without the bad frame next to it, and not far from it
        assert not same_bits(whole["sens"][t_bad - 1], w5["sens"][t_bad - 1, 2:9])
    # a bad frame at the edge of the recording: blocks outside 0..N-1 stay +0.0, those inside are NaN
    qb = q.copy()
    qb[0, 0] = np.nan
    edge = run(qb, pose, seg, bounds, half_width=2)
    assert positive_zero(edge["sens"][0, :2]) and np.isnan(edge["sens"][0, 2:]).all()
    # a batch run together equals each trajectory run alone (two sequences x two different legs)
    ang = np.stack([np.stack([q, q2]), np.stack([q[::-1], q2[::-1]])])
    pp = np.stack([np.stack([pose, pose2]), np.stack([pose[::-1], pose2[::-1]])])
    sg = np.stack([np.stack([sigma, 2 * sigma]), np.stack([sigma[::-1], sigma])])
    both = smooth_sens_harness.run(ang, pp, [seg, seg2], [bounds, bounds2], kp_sigma=sg, half_width=2)
    for s in range(2):
        for l, (sg_l, b_l) in enumerate(((seg, bounds), (seg2, bounds2))):
            alone = run(ang[s, l], pp[s, l], sg_l, b_l, kp_sigma=sg[s, l], half_width=2)
            for k in ("sens", "std", "grad"):
                assert same_bits(both[k][s, l], alone[k]), (k, s, l)
            assert np.array_equal(both["flags"][s, l], alone["flags"])
    # requests: what is not asked for changes nothing of what is
    for want in (("sens",), ("flags",), ("grad",), ("flags", "grad")):
        part = run(q, pose, seg, bounds, half_width=2, want=want)
        for k in want:
            assert np.array_equal(part[k], w2[k]) if k == "flags" else same_bits(part[k], w2[k]), (k, want)
    only_std = run(q, pose, seg, bounds, kp_sigma=sigma, want=())
    assert same_bits(only_std["std"], w0["std"])


def test_held_rows_weights_and_the_sigma_bit(smooth_sens_harness, smooth_harness):  # noqa: F811
    q, pose, seg, bounds = smoothed_window(smooth_harness, "RF", 272, 296)
    N = len(q)
    run = smooth_sens_harness.run_one
    sigma = np.full((N, 4), 0.01)
    # held rows are +0.0 at every offset and the std of a held joint is +0.0: the limits of two joints collapsed onto a
    # value inside the window, so that whichever way the full gradient pushes, about half of the frames hold them
    base = run(q, pose, seg, bounds, kp_sigma=sigma, half_width=3)
    b2 = np.array(bounds, dtype=np.float64).copy()
    for j in (1, 4):
        b2[j] = np.median(q[:, j])
    pinned = run(q, pose, seg, b2, kp_sigma=sigma, half_width=3)
    held = (pinned["flags"][:, None] >> np.arange(7)) & 1 == 1
    assert not (pinned["flags"] & ~0x7F).any() and held[:, [1, 4]].any() and not held[:, [1, 4]].all()
    for t, j in zip(*np.where(held)):
        assert positive_zero(pinned["sens"][t, :, j]) and positive_zero(pinned["std"][t, j])
    assert np.isfinite(pinned["sens"]).all() and (pinned["std"][~held] > 0).all()
    assert not same_bits(pinned["sens"], base["sens"])
    off = run(q, pose, seg, b2, kp_sigma=sigma, half_width=3, tol=0.0)       # bound_tol = 0 disables the rule
    assert not off["flags"].any()
    # zero-weight columns are +0.0 at every offset with NaN in that key point; the other columns are those of a finite pose
    w = np.ones((N, 4))
    w[:, 1] = 0.0
    w[5, 3] = 0.0
    pn = pose.copy()
    pn[:, 2] = np.nan
    pn[5, 4] = np.nan
    qw = smooth_harness.run_one(shipped_window("RF", 272, 296)[0], pn, seg, bounds, smooth=0.1, weight=w)["angles"]
    zw = run(qw, pn, seg, bounds, weight=w, kp_sigma=sigma, half_width=3)
    zf = run(qw, pose, seg, bounds, weight=w, kp_sigma=sigma, half_width=3)
    assert not (zw["flags"] & BAD_INPUT).any() and all(same_bits(zw[k], zf[k]) for k in ("sens", "std", "grad"))
    assert positive_zero(zw["sens"][:, :, :, 1]) and np.isfinite(zw["sens"]).all()
    for d in range(7):                    # the claw of frame 5, seen from frame 5 + 3 - d
        t = 5 + 3 - d
        assert positive_zero(zw["sens"][t, d, :, 3]) and np.abs(zw["sens"][t, d, :, 0]).max() > 0
    # all weights x 2: the bits of weights 1 -- sens; H and B both carry the square, the penalty does not, so this holds
    # where the frames do not couple, and with the penalty x 4
    one = run(q, pose, seg, bounds, half_width=2, tol=0.0, want=("sens",))
    two = run(q, pose, seg, bounds, weight=2.0 * np.ones((N, 4)), smooth=0.4, half_width=2, tol=0.0, want=("sens",))
    assert same_bits(one["sens"], two["sens"])
    one0 = run(q, pose, seg, bounds, smooth=0.0, half_width=2, tol=0.0, want=("sens", "flags"))
    two0 = run(q, pose, seg, bounds, weight=2.0 * np.ones((N, 4)), smooth=0.0, half_width=2, tol=0.0, want=("sens", "flags"))
    assert same_bits(one0["sens"], two0["sens"]) and np.array_equal(one0["flags"], two0["flags"])
    # bit 17: a negative or non-finite sigma of a key point WITH weight on a good frame: that frame's bit, NaN std in the
    # whole run (here: up to the bad frame 15), sens, grad and the other flag bits untouched
    qb = q.copy()
    qb[15, 0] = np.nan
    ws = np.ones((N, 4))
    ws[3, 2] = 0.0
    clean = run(qb, pose, seg, bounds, weight=ws, kp_sigma=sigma, half_width=1)
    # the sigma of a key point WITHOUT weight is not read, nor is any sigma of a bad frame: whatever stands there, every
    # output has the bits of the clean run and no bit 17 is set
    for unread in (np.nan, np.inf, -np.inf, -0.01, 1e300):
        sg = sigma.copy()
        sg[3, 2] = unread
        sg[15] = unread
        got = run(qb, pose, seg, bounds, weight=ws, kp_sigma=sg, half_width=1)
        assert np.array_equal(got["flags"], clean["flags"]) and not (got["flags"] & BAD_SIGMA).any()
        assert all(same_bits(got[k], clean[k]) for k in ("sens", "std", "grad"))
    assert np.isfinite(clean["std"][np.arange(N) != 15]).all() and (clean["std"][3] > 0).any()
    for bad_value in (-0.01, np.nan, np.inf):
        sg = sigma.copy()
        sg[4, 1] = bad_value
        sg[3, 2] = np.nan            # no weight: not read
        sg[15, 0] = np.nan           # a bad frame: bit 16 alone
        got = run(qb, pose, seg, bounds, weight=ws, kp_sigma=sg, half_width=1)
        assert np.array_equal(got["flags"], clean["flags"] | np.where(np.arange(N) == 4, BAD_SIGMA, 0))
        assert got["flags"][15] == BAD_INPUT
        assert same_bits(got["sens"], clean["sens"]) and same_bits(got["grad"], clean["grad"])
        free = (clean["flags"][:15, None] >> np.arange(7)) & 1 == 0
        assert np.isnan(got["std"][:15][free]).all() and only_the_one_nan(got["std"])
        assert same_bits(got["std"][16:], clean["std"][16:]) and np.isfinite(got["std"][16:]).all()
        nosig = run(qb, pose, seg, bounds, weight=ws, half_width=1)       # std not requested: the sigmas are not read
        assert np.array_equal(nosig["flags"], clean["flags"])


def test_python_surface_on_the_shipped_window(hiplib, smooth_sens_harness, smooth_harness, monkeypatch):  # noqa: F811
    from seqikpy_amd.data import BOUNDS, INITIAL_ANGLES, SEGMENTS
    from seqikpy_amd.kinematic_chain import KinematicChainGeneric, KinematicChainSeq
    from seqikpy_amd.leg_inverse_kinematics import LegInvKinGeneric, LegInvKinSeq
    z = load_golden("anipose_shipped")
    legs, lo, hi = ["RF", "LF"], 272, 296
    N = hi - lo
    ik = LegInvKinSeq({f"{l}_leg": z[f"{l}_pose"][lo:hi] for l in legs}, KinematicChainSeq(BOUNDS, legs), INITIAL_ANGLES,
                      log_level="ERROR")
    ja = {f"Angle_{l}_{d}": z[f"{l}_angles"][lo:hi, i] for l in legs for i, d in enumerate(DOFS)}
    real_call = hiplib._call
    monkeypatch.setattr(hiplib, "_call", harness_call(smooth_sens_harness, smooth_call(smooth_harness, real_call)))
    smoothed = ik.run_smooth(ja, smooth=0.1)
    assert sorted(ik.smooth_report["RF"]) == ["cost", "frame_info", "largest_change", "reason", "rejected", "steps"]
    out = ik.run_smooth_sensitivity(smoothed, smooth=0.1, half_width=2)
    assert list(out) == ["RF_leg", "LF_leg"]
    sig_n4 = np.random.default_rng(2).uniform(0.005, 0.05, (N, 4))
    for l in legs:
        res = out[f"{l}_leg"]
        assert sorted(res) == ["flags", "grad", "sens"]
        assert res["sens"].shape == (N, 5, 7, 4, 3) and res["flags"].shape == (N,) and res["grad"].shape == (N,)
        assert res["flags"].dtype == np.int32 and np.isfinite(res["sens"]).all()
        seg = [ik.kinematic_chain_class.body_size[f"{l}_{s}"] for s in SEGMENTS]
        bounds = np.array([ik.kinematic_chain_class.bounds_dof[f"{l}_{d}"] for d in DOFS])
        ang = np.stack([smoothed[f"Angle_{l}_{d}"] for d in DOFS], 1)
        kp = ik._fk_key_points(l, z[f"{l}_pose"][lo:hi])
        ref = smooth_sens_harness.run_one(ang, kp, seg, bounds, smooth=0.1, half_width=2)
        assert same_bits(res["sens"], ref["sens"]) and np.array_equal(res["flags"], ref["flags"])
        assert same_bits(res["grad"], ref["grad"])
        for sigma in (0.02, np.array([0.01, 0.02, 0.03, 0.04]), sig_n4, {"RF": 0.02, "LF": sig_n4}):
            unc = ik.angle_uncertainty(sigma, smoothed, fit="smooth", smooth=0.1)
            assert list(unc) == [f"Angle_{m}_{d}" for m in legs for d in DOFS]
            s = sigma[l] if isinstance(sigma, dict) else sigma
            ref_std = smooth_sens_harness.run_one(ang, kp, seg, bounds, smooth=0.1, kp_sigma=np.broadcast_to(s, (N, 4)))["std"]
            assert same_bits(np.stack([unc[f"Angle_{l}_{d}"] for d in DOFS], 1), ref_std)
    # smooth belongs to fit="smooth", and fit="smooth" needs it
    with pytest.raises(ValueError, match="smooth belongs to fit='smooth'"):
        ik.angle_uncertainty(0.02, smoothed, fit="refine", smooth=0.1)
    with pytest.raises(ValueError, match="smooth belongs to fit='smooth'"):
        ik.angle_uncertainty(0.02, smoothed, smooth=0.1)
    with pytest.raises(ValueError, match="fit must be"):
        ik.angle_uncertainty(0.02, smoothed, fit="smooth")
    with pytest.raises(ValueError, match="fit must be"):
        ik.angle_uncertainty(0.02, smoothed, fit="other")
    # weights reach the rule
    w = np.array([1.0, 0.0, 1.0, 1.0])
    sm_w = ik.run_smooth(ja, smooth=0.1, key_point_weight=w)
    out_w = ik.run_smooth_sensitivity(sm_w, smooth=0.1, key_point_weight=w, half_width=1)
    assert not out_w["RF_leg"]["sens"][:, :, :, 1].any() and np.abs(out_w["RF_leg"]["sens"][:, :, :, [0, 2, 3]]).max() > 0
    # the stored angles are the default
    ik.joint_angles_dict = smoothed
    assert same_bits(ik.run_smooth_sensitivity(smooth=0.1, half_width=2)["LF_leg"]["sens"], out["LF_leg"]["sens"])
    # _lib.smooth_sensitivity: what is asked for, and nothing else
    params = [ik._leg_params(l) for l in legs]
    ang = np.stack([np.stack([smoothed[f"Angle_{l}_{d}"] for d in DOFS], 1) for l in legs])[None]
    pose = np.stack([ik._fk_key_points(l, z[f"{l}_pose"][lo:hi]) for l in legs])[None]
    only = hiplib.smooth_sensitivity(ang, pose, params, kp_sigma=0.02, want_sens=False, want_grad=False, want_flags=False)
    assert only["sens"] is None and only["flags"] is None and only["grad"] is None and only["std"].shape == (1, 2, N, 7)
    full = hiplib.smooth_sensitivity(ang, pose, params, half_width=4)
    assert full["std"] is None and full["sens"].shape == (1, 2, N, 9, 7, 4, 3) and full["flags"].shape == (1, 2, N)
    # the generic chain has no such quantity
    zg = load_golden("generic_rf_100")
    gen = LegInvKinGeneric({"RF_leg": zg["RF_pose"]}, KinematicChainGeneric(BOUNDS, ["RF"]), INITIAL_ANGLES, log_level="ERROR")
    for call in (lambda: gen.run_smooth_sensitivity(), lambda: gen.angle_uncertainty(0.02, fit="smooth", smooth=0.1)):
        with pytest.raises(ValueError, match="not a function of the key points"):
            call()


# ---------------------------------------------------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(hiplib):
    return gpu_lib(hiplib)


@pytest.mark.gpu
@pytest.mark.parametrize("N", GPU_FRAMES)
def test_gpu_kernels_equal_the_host_rule_bit_for_bit(lib, smooth_sens_harness, N):  # noqa: F811
    """2 sequences x 3 legs (three different segment sets and limits) x N frames with weights, zero-weight NaN key points,
    held joints and, for N >= 3, a bad frame in the middle; sens only, std only, flags + grad only and all four, at
    half_width 0 and 2; guards around every buffer and the workspace; the default plan."""
    for W in GPU_WIDTHS:
        c = gpu_case(smooth_sens_harness, N, W)
        for want in SUBSETS:
            check_device_against_host(lib, c, want)


@pytest.mark.gpu
def test_gpu_one_workgroup_of_64_in_a_fresh_process(lib, smooth_sens_harness, tmp_path):  # noqa: F811
    """SEQIK_SMOOTHSENS_BLOCK=64 SEQIK_SMOOTHSENS_GRID=1, set in a fresh child process, on 12 sequences x 3 legs x 5 frames:
    72 sweep items and 180 frames, so every kernel takes its grid stride."""
    c = gpu_case(smooth_sens_harness, 5, 2, S=12)
    path = str(tmp_path / "case.npz")
    np.savez(path, case=np.array(c, dtype=object))
    env = dict(os.environ, SEQIK_SMOOTHSENS_BLOCK="64", SEQIK_SMOOTHSENS_GRID="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "smooth_sens_support.py"), path], env=env,
                         capture_output=True, text=True, timeout=300, cwd=os.path.join(ROOT, "tests"))
    assert out.returncode == 0 and "CHILD OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


@pytest.mark.gpu
def test_gpu_host_entry_equals_device_entry_and_a_replayed_graph(lib, smooth_sens_harness):  # noqa: F811
    import torch
    W = 2
    c = gpu_case(smooth_sens_harness, 65, W)
    S, L, N = c["ang"].shape[:3]
    params = [lib.leg_params_from_arrays(s, b, np.zeros(27)) for s, b in zip(c["segs"], c["bounds"])]
    ref = c["with_std"]
    host = lib.smooth_sensitivity(c["ang"], c["pose"], params, smooth=c["smooth"], kp_weight=c["weight"], kp_sigma=c["sigma"],
                                  half_width=W)
    assert all(same_bits(host[k], ref[k]) for k in ("sens", "std", "grad"))
    assert host["flags"].dtype == np.int32 and np.array_equal(host["flags"], ref["flags"])
    plain = lib.smooth_sensitivity(c["ang"], c["pose"], params, smooth=c["smooth"], kp_weight=c["weight"], half_width=W,
                                   want_flags=False, want_grad=False)
    assert plain["std"] is None and plain["flags"] is None and same_bits(plain["sens"], c["no_std"]["sens"])
    d_ang, d_pose, d_w, d_sig = (torch.from_numpy(c[k]).cuda() for k in ("ang", "pose", "weight", "sigma"))
    ws_bytes = lib.smooth_sensitivity_workspace_bytes(S, L, N, W)
    d_ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")
    fresh = lambda: (torch.full((S, L, N, 2 * W + 1, 7, 4, 3), 7.0, dtype=torch.float64, device="cuda"),  # noqa: E731
                     torch.full((S, L, N, 7), 7.0, dtype=torch.float64, device="cuda"),
                     torch.full((S, L, N), 7.0, dtype=torch.float64, device="cuda"),
                     torch.full((S, L, N), 7, dtype=torch.int32, device="cuda"))

    def enqueue(bufs, stream):
        lib.smooth_sensitivity_device(d_ang, d_pose, S, L, N, params, d_ws, ws_bytes, d_kp_weight=d_w, d_kp_sigma=d_sig,
                                      d_sens=bufs[0], d_std=bufs[1], d_grad=bufs[2], d_flags=bufs[3], smooth=c["smooth"],
                                      half_width=W, stream=stream)

    def check(bufs):
        assert same_bits(bufs[0].cpu().numpy(), host["sens"]) and same_bits(bufs[1].cpu().numpy(), host["std"])
        assert same_bits(bufs[2].cpu().numpy(), host["grad"]) and np.array_equal(bufs[3].cpu().numpy(), host["flags"])

    s = torch.cuda.Stream()
    bufs = fresh()
    with torch.cuda.stream(s):
        enqueue(bufs, s)
    s.synchronize()
    check(bufs)
    # the device entry allocates nothing and waits for nothing: captured into a graph and replayed once
    gbufs = fresh()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        enqueue(gbufs, torch.cuda.current_stream())
    for b in gbufs:
        b.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    check(gbufs)
    with pytest.raises(ValueError, match="expected a int32 tensor"):
        lib.smooth_sensitivity_device(d_ang, d_pose, S, L, N, params, d_ws, ws_bytes, d_flags=bufs[1])
    # empty input: no launch, the output is not touched
    keep = bufs[0].clone()
    lib.smooth_sensitivity_device(d_ang.data_ptr(), d_pose.data_ptr(), 0, L, N, params, 0, 0, d_sens=bufs[0].data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(keep.view(torch.int64), bufs[0].view(torch.int64))


@pytest.mark.gpu
def test_gpu_run_smooth_with_sigma_equals_the_two_host_calls(lib):
    """``run_smooth(key_point_sigma=0.01)`` on RF 0:600 of the shipped recording -- the smoothed angles stay on the device
    between the two units -- equals ``smooth_legs`` then ``smooth_sensitivity`` through host buffers, bit for bit."""
    from seqikpy_amd.data import BOUNDS, INITIAL_ANGLES
    from seqikpy_amd.kinematic_chain import KinematicChainSeq
    from seqikpy_amd.leg_inverse_kinematics import LegInvKinSeq
    z = load_golden("anipose_shipped")
    pose = z["RF_pose"][:600]
    ik = LegInvKinSeq({"RF_leg": pose}, KinematicChainSeq(BOUNDS, ["RF"]), INITIAL_ANGLES, log_level="ERROR")
    ja = {f"Angle_RF_{d}": z["RF_angles"][:600, i] for i, d in enumerate(DOFS)}
    smoothed = ik.run_smooth(ja, smooth=0.1, key_point_sigma=0.01)
    report = ik.smooth_report["RF"]
    assert sorted(report) == ["cost", "frame_info", "largest_change", "reason", "rejected", "sens_flags", "std", "steps"]
    assert report["std"].shape == (600, 7)
    params = [ik._leg_params("RF")]
    ang = z["RF_angles"][:600][None, None]
    kp = ik._fk_key_points("RF", pose)[None, None]
    first = lib.smooth_legs(ang, kp, params, smooth=0.1)
    second = lib.smooth_sensitivity(first["angles"], kp, params, smooth=0.1, kp_sigma=0.01, want_sens=False, want_grad=False)
    assert same_bits(np.stack([smoothed[f"Angle_RF_{d}"] for d in DOFS], 1), first["angles"][0, 0])
    assert same_bits(report["cost"], first["cost"][0, 0]) and np.array_equal(report["frame_info"], first["frame_info"][0, 0])
    assert same_bits(report["std"], second["std"][0, 0]) and np.array_equal(report["sens_flags"], second["flags"][0, 0])
    assert np.isfinite(report["std"]).all() and (report["std"][report["sens_flags"] == 0] > 0).all()
    # without the argument nothing changes, and angle_uncertainty(fit="smooth") is the same quantity
    plain = ik.run_smooth(ja, smooth=0.1)
    assert sorted(ik.smooth_report["RF"]) == ["cost", "frame_info", "largest_change", "reason", "rejected", "steps"]
    assert all(same_bits(plain[k], smoothed[k]) for k in smoothed)
    unc = ik.angle_uncertainty(0.01, smoothed, fit="smooth", smooth=0.1)
    assert same_bits(np.stack([unc[f"Angle_RF_{d}"] for d in DOFS], 1), report["std"])
