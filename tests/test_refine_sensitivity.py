"""Error bars of the whole-leg refinement: exact-Hessian sensitivity of the refined angles (include/
seqik_refine_sensitivity.h, csrc/seqik_refine_sens.hpp / seqik_refine_sens.hip).

CPU tier: the header, the signature table and the exports; every SEQIK_ERR_BAD_ARG case through the C ABI without a GPU;
the properties of the host-run rule (tests/harness/refine_sens_harness.hip) on the refined shipped frames and made-up
legs; bad input; the staged re-enactment; the pivot path of the factorisation; the Python surface -- ``_lib.
refine_sensitivity``, ``LegInvKinSeq.run_refine_sensitivity`` / ``angle_uncertainty(fit="refine")`` -- with the library
call answered by the host-run rule.  GPU tier (``-m gpu``): the kernel against the host-run rule bit for bit over sizes
around the quarter-record pass and the wavefront, every output subset, guards, the default plan and -- in a fresh child
process -- one workgroup of 64; both entry points; ``run_refine(key_point_sigma=...)`` against the two host calls.

The accuracy and the meaning of the rule: tests/test_refine_sensitivity_accuracy.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from angle_map_support import gpu_lib, same_bits
from conftest import DOFS, ROOT, load_golden
from refine_sens_support import (BAD_INPUT, EPS, FD_FRAMES, GPU_FRAMES, NOT_PD, SUBSETS, TOL, check_device_against_host,  # noqa: F401
                                 gpu_case, harness_call, mp_rule, numpy_rule, numpy_std, refine_rule_harness,
                                 refine_sens_harness, refined_inputs)
from refine_support import GTOL, reason
from test_capi_symbols import assert_same_class, header_prototypes

SYMBOLS = ["seqik_refine_sensitivity", "seqik_refine_sensitivity_device"]
QNAN = np.uint64(0x7FF8000000000000)


def only_the_one_nan(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return (a.view(np.uint64)[np.isnan(a)] == QNAN).all()


# ---------------------------------------------------------------------------------------------------------------------
# CPU tier
# ---------------------------------------------------------------------------------------------------------------------

def test_header_declares_exactly_the_new_entry_points(hiplib):
    raw = open(os.path.join(ROOT, "include", "seqik_refine_sensitivity.h")).read()
    assert "sens_F[.][k][c] = H_FF^-1 (w_k J_k,F,c)" in raw and "ONLY at angles that minimise that fit" in raw
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(seqik_[a-z_]+)\s*\(", text)))
    assert declared == sorted(SYMBOLS)
    assert sorted(hiplib.REFINE_SENS_SIGNATURES) == ["seqik_refine_sensitivity.h"]
    assert hiplib.REFINE_SENS_EXPORTED_SYMBOLS == [s[0] for s in hiplib.REFINE_SENS_SIGNATURES["seqik_refine_sensitivity.h"]]
    assert sorted(hiplib.REFINE_SENS_EXPORTED_SYMBOLS) == declared
    # an eighth table: disjoint from the other seven, which keep their headers
    tables = (hiplib.SIGNATURES, hiplib.EXTENSION_SIGNATURES, hiplib.STREAM_GAPS_SIGNATURES, hiplib.JACOBIAN_SIGNATURES,
              hiplib.SENSITIVITY_SIGNATURES, hiplib.REFINE_SIGNATURES, hiplib.SMOOTH_SIGNATURES)
    assert not set(declared) & {s[0] for table in tables for sigs in table.values() for s in sigs}
    assert all("seqik_refine_sensitivity.h" not in table for table in tables) and len(hiplib.SIGNATURES) == 6
    lib = hiplib.load()
    assert lib.seqik_abi_version() == 7 == hiplib.ABI_VERSION
    assert "seqik_refine_sens.hip" in hiplib.COMPILE_UNITS and "seqik_refine_sens.hpp" in hiplib.CSRC_HEADERS
    assert "seqik_refine_sens" not in " ".join(hiplib.KERNEL_SOURCES + hiplib.LATENCY_SOURCES)
    assert '"seqik_refine_sensitivity.h"' in open(os.path.join(ROOT, "setup.py")).read()
    assert "#define SEQIK_REFSENS_FLAG_NOT_PD (1 << 8)\n" in raw and hiplib.REFINE_SENS_FLAG_NOT_PD == NOT_PD
    assert "#define SEQIK_REFSENS_FLAG_BAD_INPUT (1 << 16)\n" in raw and hiplib.REFINE_SENS_FLAG_BAD_INPUT == BAD_INPUT
    # the table against the prototypes: count and class, and what the loaded library is bound with
    protos = header_prototypes("seqik_refine_sensitivity.h")
    table = {sig[0]: sig[1:] for sig in hiplib.REFINE_SENS_SIGNATURES["seqik_refine_sensitivity.h"]}
    assert sorted(table) == sorted(protos) == declared
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name][0], list(table[name][1:])
        assert len(argtypes) == len(params) == 15, (name, params)
        assert_same_class(ret, restype, False, name)
        for p, a in zip(params, argtypes):
            assert_same_class(p, a, True, name)
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_bad_arguments_are_refused_before_anything_touches_hip(hiplib):
    """Every SEQIK_ERR_BAD_ARG case of the header, raised on a machine without a GPU, by both entry points; a call with
    no leg-frames returns OK without a launch."""
    lib = hiplib.load()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    ang, pose, sig = np.zeros((1, 2, 3, 7)), np.zeros((1, 2, 3, 5, 3)), np.ones((1, 2, 3, 4))
    out, flg = np.zeros((1, 2, 3, 84)), np.zeros((1, 2, 3), np.int32)
    a, p, g, o, f = (ang.ctypes.data_as(dp), pose.ctypes.data_as(dp), sig.ctypes.data_as(dp), out.ctypes.data_as(dp),
                     flg.ctypes.data_as(ip))
    good = (hiplib.SeqikLegParams * 2)()
    for l in range(2):
        for i in range(4):
            good[l].seg[i] = 0.5
    bad_seg = (hiplib.SeqikLegParams * 2)()
    bad_seg[1].seg[2] = np.inf
    huge = 2 ** 63 // (8 * 84) + 1
    t = 1e-6
    #        angles pose n_seq n_legs n_frames legs kind kp_weight kp_sigma tol sens std grad flags
    cases = [("n_legs", (a, p, 1, 0, 3, good, 0, None, None, t, o, None, None, None)),
             ("n_legs", (a, p, 1, 9, 3, good, 0, None, None, t, o, None, None, None)),
             ("negative", (a, p, -1, 2, 3, good, 0, None, None, t, o, None, None, None)),
             ("negative", (a, p, 1, 2, -3, good, 0, None, None, t, o, None, None, None)),
             ("angles", (None, p, 1, 2, 3, good, 0, None, None, t, o, None, None, None)),
             ("pose", (a, None, 1, 2, 3, good, 0, None, None, t, o, None, None, None)),
             ("legs", (a, p, 1, 2, 3, None, 0, None, None, t, o, None, None, None)),
             ("no output", (a, p, 1, 2, 3, good, 0, None, None, t, None, None, None, None)),
             ("no output", (a, p, 1, 2, 3, good, 0, g, g, t, None, None, None, None)),
             ("std needs kp_sigma", (a, p, 1, 2, 3, good, 0, None, None, t, o, o, None, None)),
             ("std needs kp_sigma", (a, p, 1, 2, 3, good, 0, g, None, t, None, o, o, f)),
             ("generic chain", (a, p, 1, 2, 3, good, 1, None, None, t, o, None, None, None)),
             ("generic chain", (a, p, 1, 2, 3, good, 1, None, g, t, None, o, None, f)),
             ("kind", (a, p, 1, 2, 3, good, 2, None, None, t, o, None, None, None)),
             ("kind", (a, p, 1, 2, 3, good, -1, None, None, t, None, None, None, f)),
             ("segment", (a, p, 1, 2, 3, bad_seg, 0, None, None, t, o, None, None, None)),
             ("bound_tol", (a, p, 1, 2, 3, good, 0, None, None, -1e-6, o, None, None, None)),
             ("bound_tol", (a, p, 1, 2, 3, good, 0, None, None, np.nan, None, None, o, None)),
             ("bound_tol", (a, p, 1, 2, 3, good, 0, None, None, np.inf, None, None, None, f)),
             ("too many", (a, p, huge, 1, 1, good, 0, None, None, t, o, None, None, None)),
             ("too many", (a, p, 1, 1, huge, good, 0, None, None, t, None, None, None, f)),
             ("too many", (a, p, 2 ** 40, 2, 2 ** 40, good, 0, None, None, t, None, None, o, None))]
    for what, args in cases:
        for fn, last in ((lib.seqik_refine_sensitivity, -1), (lib.seqik_refine_sensitivity_device, None)):
            assert fn(*args, last) == hiplib.ERR_ARG, (what, fn.__name__)
            msg = lib.seqik_last_error().decode()
            assert msg.startswith("seqik_refine_sensitivity: ") and what.split()[0] in msg, (what, msg)
    for args in ((a, p, 0, 2, 3, good, 0, None, None, t, o, None, o, f), (a, p, 1, 2, 0, good, 0, g, g, 0.0, o, o, o, f)):
        assert lib.seqik_refine_sensitivity(*args, -1) == 0 and lib.seqik_refine_sensitivity_device(*args, None) == 0
    assert not out.any() and not flg.any()
    # the Python wrappers: shapes and arguments
    params = [hiplib.leg_params_from_arrays(np.full(4, 0.5), np.zeros((7, 2)), np.zeros(27))] * 2
    with pytest.raises(ValueError, match="no output"):
        hiplib.refine_sensitivity(ang, pose, params, want_sens=False, want_grad=False, want_flags=False)
    with pytest.raises(ValueError, match="std needs kp_sigma"):
        hiplib.refine_sensitivity(ang, pose, params, want_std=True)
    with pytest.raises(ValueError, match="pose must have shape"):
        hiplib.refine_sensitivity(ang, pose[..., :4, :], params)
    with pytest.raises(ValueError, match="kp_sigma must broadcast"):
        hiplib.refine_sensitivity(ang, pose, params, kp_sigma=np.ones(3))
    with pytest.raises(ValueError, match="kp_weight must broadcast"):
        hiplib.refine_sensitivity(ang, pose, params, kp_weight=np.ones(3))
    with pytest.raises(ValueError, match=r"shape \(S, L, N, 7\)"):
        hiplib.refine_sensitivity(ang[0], pose, params)


def test_properties_on_the_refined_frames(refine_sens_harness, refine_rule_harness):  # noqa: F811
    """Held rows, std, the held bits and grad against the refinement's own report, the one NaN, the staged re-enactment:
    on every refined leg-frame of the shipped recording and of the made-up legs."""
    n_held = n_not_pd = n_flag_cases = n_reason0 = 0
    for name, q, pose, seg, b, info in refined_inputs(refine_rule_harness):
        shipped = name in ("RF", "LF")
        sigma = np.random.default_rng(len(q)).uniform(0.005, 0.05, (len(q), 4))
        got = refine_sens_harness.run(q, pose, seg, b, kp_sigma=sigma)
        sens, std, grad, flags = got["sens"], got["std"], got["grad"], got["flags"]
        assert not (flags & ~(0x7F | NOT_PD)).any(), name
        held = (flags[:, None] >> np.arange(7)) & 1 == 1
        not_pd = (flags & NOT_PD) != 0
        n_held, n_not_pd = n_held + held.any(1).sum(), n_not_pd + not_pd.sum()
        # a held row is +0.0 by bits, and so is its std; the rows of F are the one NaN where a pivot was not positive
        assert not sens[held].view(np.uint64).any() and not std[held].view(np.uint64).any(), name
        free_nan = ~held & not_pd[:, None]
        assert np.isnan(sens[free_nan]).all() and np.isnan(std[free_nan]).all(), name
        assert np.isfinite(sens[~free_nan]).all() and np.isfinite(std[~free_nan]).all(), name
        assert only_the_one_nan(sens) and only_the_one_nan(std) and np.isfinite(grad).all(), name
        if shipped:      # (the refinement can stop where its cost stalls without being at a strict minimum: a few frames)
            print(f"{name}: {int(not_pd.sum())} of {len(q)} refined frames not a strict minimum (stop reasons "
                  f"{sorted(set(reason(info[not_pd]).tolist()))}), {int(held.any(1).sum())} with a held joint")
            assert not_pd.mean() < 0.02, name
        # std is the header's formula applied to sens, within 4 ulp
        ref = numpy_std(sens, sigma)
        fin = np.isfinite(ref)
        assert np.array_equal(np.isnan(std), ~fin) and (np.abs(std[fin] - ref[fin]) <= 4 * np.spacing(ref[fin])).all(), name
        # without sigma: the same record, no std
        plain = refine_sens_harness.run(q, pose, seg, b)
        assert plain["std"] is None and same_bits(plain["sens"], sens) and np.array_equal(plain["flags"], flags)
        assert same_bits(plain["grad"], grad)
        # flags + grad alone (no solve is made), and bound_tol = 0 switches the held rule off
        fg = refine_sens_harness.run(q, pose, seg, b, want=("grad", "flags"))
        assert fg["sens"] is None and np.array_equal(fg["flags"], flags) and same_bits(fg["grad"], grad)
        assert not (refine_sens_harness.run(q, pose, seg, b, tol=0.0, want=("flags",))["flags"] & 0x7F).any()
        # against the refinement's own report and the numpy restatement
        bar = GTOL * np.sum(seg) ** 2
        lb, ub = b[:, 0], b[:, 1]
        for i in range(len(q)):
            ref_i = numpy_rule(q[i], pose[i], seg, b)
            scale = 1.0 + np.abs(pose[i, 1:] - pose[i, 0]).max() / np.sum(seg)
            # within rounding: g_a sums products |J| |r| <= len (len + |t|), each with a few eps of the chain's error
            assert abs(grad[i] - ref_i["grad"]) <= 256 * EPS * scale, (name, i, grad[i], ref_i["grad"])
            candidate = (q[i] - lb <= TOL) | (ub - q[i] <= TOL)
            if (np.abs(ref_i["g"][candidate]) > bar).all():
                n_flag_cases += 1
                assert (flags[i] & 0x7F) == (info[i] & 0x7F), (name, i, flags[i], info[i])
            if reason(info[i]) == 0:
                n_reason0 += 1
                assert grad[i] <= GTOL, (name, i, grad[i])
        # the kernel's staged pass (four lanes per record, values arriving key point by key point) on the host
        m = len(q) // 16 * 16
        assert same_bits(refine_sens_harness.staged(q[:m], pose[:m], seg, b), sens[:m]), name
    print(f"{n_held} leg-frames with a held joint, {n_not_pd} not a strict minimum, {n_flag_cases} held-bit comparisons, "
          f"{n_reason0} stopped on the gradient")
    assert n_held > 100 and n_not_pd > 10 and n_flag_cases > 1000 and n_reason0 > 300


def test_weights(refine_sens_harness):  # noqa: F811
    """What the derivation gives for weights: H carries w_k^2 and so does the right-hand side w_k J_k (J_k carries one w_k
    itself), so multiplying every weight by the same factor leaves sens unchanged -- tested with (2, 2, 2, 2) against the
    200-bit yardstick of weights 1, inside that yardstick's bar (a power of two scales every product exactly: the bits are
    the same, too).  A key point with weight exactly 0 is not read: NaN in it changes nothing, its columns are +0.0, and
    the other columns are those of the fit without it (without the claw that fit has no strict minimum: bit 8)."""
    z = load_golden("anipose_shipped")
    from refine_support import numpy_refine
    for leg in ("RF", "LF"):
        seg, b = z[f"{leg}_seg"], z[f"{leg}_bounds"]
        for fr in FD_FRAMES[::3]:
            pose = z[f"{leg}_pose"][fr][:5]
            q = numpy_refine(z[f"{leg}_angles"][fr], pose, seg, b)[0]
            mp = mp_rule(q, pose, seg, b)
            scale = np.abs(mp["sens"]).max()
            bar = 100 * max(np.abs(numpy_rule(q, pose, seg, b)["sens"] - mp["sens"]).max() / scale, EPS)
            one = refine_sens_harness.run(q[None], pose[None], seg, b)
            two = refine_sens_harness.run(q[None], pose[None], seg, b, weight=2.0)
            assert np.abs(two["sens"][0] - mp["sens"]).max() / scale <= bar, (leg, fr)
            assert same_bits(two["sens"], one["sens"]) and np.array_equal(two["flags"], one["flags"])
            assert same_bits(two["grad"], 4 * one["grad"])
            for k in range(4):
                w = np.ones(4)
                w[k] = 0.0
                qk = numpy_refine(q, pose, seg, b, weight=w)[0]
                hole = pose.copy()
                hole[k + 1] = np.nan
                got = refine_sens_harness.run(qk[None], hole[None], seg, b, weight=w, kp_sigma=0.01)
                same = refine_sens_harness.run(qk[None], pose[None], seg, b, weight=w, kp_sigma=0.01)
                assert all(same_bits(got[x], same[x]) for x in ("sens", "std", "grad")), (leg, fr, k)
                assert np.array_equal(got["flags"], same["flags"])
                if k == 3:      # without the claw TiTa_pitch moves nothing: H has a zero row, the fit no strict minimum
                    free = (got["flags"][0] >> np.arange(7)) & 1 == 0
                    assert got["flags"][0] & NOT_PD and (got["sens"][0][free].view(np.uint64) == QNAN).all()
                    continue
                assert got["flags"][0] & ~0x7F == 0 and np.isfinite(got["sens"]).all() and np.isfinite(got["std"]).all()
                assert not got["sens"][0][:, k].view(np.uint64).any(), (leg, fr, k)
                mpk = mp_rule(qk, pose, seg, b, weight=w)
                assert mpk["flags"] == got["flags"][0] or not mpk["robust"]
                if mpk["robust"]:
                    sk = np.abs(mpk["sens"]).max()
                    bk = 100 * max(np.abs(numpy_rule(qk, pose, seg, b, weight=w)["sens"] - mpk["sens"]).max() / sk, EPS)
                    assert np.abs(got["sens"][0] - mpk["sens"]).max() / sk <= bk, (leg, fr, k)


def test_not_a_minimum_sets_bit_8_and_nan_rows(refine_sens_harness, refine_rule_harness):  # noqa: F811
    """Angles that are not a strict minimum of the whole-leg fit: the made-up legs (targets far out of reach and on the
    origin) have leg-frames where the 200-bit yardstick says H_FF is indefinite at the refinement's result (a target on
    the base leaves the three thorax-coxa rotations without effect); and the pivot path of the factorisation alone, on
    hand-made matrices."""
    n = 0
    for name, q, pose, seg, b, _ in refined_inputs(refine_rule_harness)[2:12]:
        got = refine_sens_harness.run(q, pose, seg, b, kp_sigma=0.01)
        for i in np.where(got["flags"] & NOT_PD)[0]:
            mp = mp_rule(q[i], pose[i], seg, b)
            if not mp["robust"]:
                continue
            n += 1
            assert mp["flags"] == got["flags"][i], (name, i)
            held = (got["flags"][i] >> np.arange(7)) & 1 == 1
            assert (got["sens"][i][~held].view(np.uint64) == QNAN).all() and (got["std"][i][~held].view(np.uint64) == QNAN).all()
            assert not got["sens"][i][held].view(np.uint64).any() and not got["std"][i][held].view(np.uint64).any()
    assert n >= 5
    rng = np.random.default_rng(8)
    A = rng.standard_normal((7, 9))
    H = A @ A.T
    L, pd = refine_sens_harness.factor(H)
    assert pd and np.abs(L @ L.T - H).max() <= 64 * EPS * np.abs(H).max()
    assert np.abs(L - np.linalg.cholesky(H)).max() <= 1e3 * EPS * np.linalg.cond(H)
    for j in (0, 3, 6):                      # a pivot that is not positive: in the first row, inside, in the last
        bad = H.copy()
        bad[j, j] = -1.0 if j == 0 else H[j, j] - 1.0001 * L[j, j] ** 2
        assert not refine_sens_harness.factor(bad)[1], j
        assert refine_sens_harness.factor(bad, held=1 << j)[1], j       # ... and held out of the way, it is not met
    zero = H.copy()
    zero[6, 6] = H[6, 6] - L[6, 6] ** 2      # a pivot of (about) 0 is not positive either
    zero[6, 6] -= 8 * np.spacing(H[6, 6])
    assert not refine_sens_harness.factor(zero)[1]
    # held rows and columns are the identity's: the factor of the rest is that of the smaller matrix
    Lh, pd = refine_sens_harness.factor(H, held=0b0100101)
    keep = [1, 3, 4, 6]
    assert pd and np.abs(Lh[np.ix_(keep, keep)] - np.linalg.cholesky(H[np.ix_(keep, keep)])).max() <= 1e3 * EPS * np.linalg.cond(H)
    assert all(Lh[j, j] == 1.0 and not np.delete(Lh[j], j).any() and not np.delete(Lh[:, j], j).any() for j in (0, 2, 5))
    nanH = H.copy()
    nanH[4, 2] = np.nan
    assert not refine_sens_harness.factor(nanH)[1]


def test_bad_input_gives_nan_and_bit_16_on_that_leg_frame_alone(refine_sens_harness, refine_rule_harness):  # noqa: F811
    name, q, pose, seg, b, _ = refined_inputs(refine_rule_harness)[0]
    q, pose = q[:32].copy(), pose[:32].copy()
    w, sigma = np.ones((32, 4)), np.full((32, 4), 0.01)
    clean = refine_sens_harness.run(q, pose, seg, b, weight=w, kp_sigma=sigma)
    kinds = [("angle NaN", lambda: q.__setitem__((1, 3), np.nan)), ("angle inf", lambda: q.__setitem__((4, 0), np.inf)),
             ("angle outside the domain", lambda: q.__setitem__((6, 6), 1e300)),
             ("pose[0] NaN", lambda: pose.__setitem__((9, 0, 1), np.nan)),
             ("key point inf", lambda: pose.__setitem__((12, 3, 2), -np.inf)),
             ("weight negative", lambda: w.__setitem__((15, 2), -1.0)), ("weight NaN", lambda: w.__setitem__((18, 0), np.nan)),
             ("weight inf", lambda: w.__setitem__((21, 3), np.inf)), ("sigma NaN", lambda: sigma.__setitem__((24, 1), np.nan)),
             ("sigma inf", lambda: sigma.__setitem__((27, 2), np.inf))]
    rows = [1, 4, 6, 9, 12, 15, 18, 21, 24, 27]
    for _, poke in kinds:
        poke()
    got = refine_sens_harness.run(q, pose, seg, b, weight=w, kp_sigma=sigma)
    bad = np.zeros(32, bool)
    bad[rows] = True
    assert (got["flags"][bad] == BAD_INPUT).all() and not (got["flags"][~bad] & BAD_INPUT).any()
    for k in ("sens", "std", "grad"):
        assert (got[k][bad].view(np.uint64) == QNAN).all(), k
        assert same_bits(got[k][~bad], clean[k][~bad]), k
    assert np.array_equal(got["flags"][~bad], clean["flags"][~bad])
    # the sigma is read for std only: without std those two leg-frames are clean
    nos = refine_sens_harness.run(q, pose, seg, b, weight=w)
    assert (nos["flags"][[24, 27]] == clean["flags"][[24, 27]]).all() and same_bits(nos["sens"][[24, 27]], clean["sens"][[24, 27]])
    assert (nos["flags"][rows[:8]] == BAD_INPUT).all()
    # a segment length that is not finite (the C ABI refuses it; the rule itself treats it as bad input)
    inf_seg = np.array(seg, dtype=np.float64)
    inf_seg[1] = np.inf
    assert (refine_sens_harness.run(q[:2], pose[:2], inf_seg, b)["flags"] == BAD_INPUT).all()


def test_python_surface_on_the_df3d_fixture(hiplib, refine_sens_harness, refine_rule_harness, monkeypatch):  # noqa: F811
    from seqikpy_amd.data import BOUNDS, INITIAL_ANGLES, SEGMENTS
    from seqikpy_amd.kinematic_chain import KinematicChainGeneric, KinematicChainSeq
    from seqikpy_amd.leg_inverse_kinematics import LegInvKinGeneric, LegInvKinSeq
    z = load_golden("df3d_100")
    legs = ["RF", "LF"]
    N = 100
    ik = LegInvKinSeq({f"{l}_leg": z[f"{l}_pose"] for l in legs}, KinematicChainSeq(BOUNDS, legs), INITIAL_ANGLES,
                      log_level="ERROR")
    ja = {f"Angle_{l}_{d}": z[f"{l}_angles"][:, i] for l in legs for i, d in enumerate(DOFS)}
    sig_n4 = np.random.default_rng(2).uniform(0.005, 0.05, (N, 4))
    # fit="sequential" (the default) gives the bits it gave before this unit existed: the call the old code made
    from test_sensitivity import harness_call as sequential_call
    from sensitivity_support import SensHarness
    from harness_build import build_harness
    seq_harness = SensHarness(build_harness(os.path.join(ROOT, "tests", "harness", "sensitivity_harness.hip")))
    real_call = hiplib._call
    monkeypatch.setattr(hiplib, "_call", sequential_call(seq_harness, real_call))
    for sigma in (0.02, sig_n4):
        old = ik.angle_uncertainty(sigma, ja)
        assert list(old) == list(ik.angle_uncertainty(sigma, ja, fit="sequential"))
        for l in legs:
            seg = [ik.kinematic_chain_class.body_size[f"{l}_{s}"] for s in SEGMENTS]
            bounds = np.array([ik.kinematic_chain_class.bounds_dof[f"{l}_{d}"] for d in DOFS])
            _, ref, _ = seq_harness.run(z[f"{l}_angles"], z[f"{l}_pose"][:, :5], seg, bounds, kp_sigma=sigma)
            for fit in ({}, dict(fit="sequential")):
                got = ik.angle_uncertainty(sigma, ja, **fit)
                assert same_bits(np.stack([got[f"Angle_{l}_{d}"] for d in DOFS], 1), ref)
    with pytest.raises(ValueError, match="fit must be"):
        ik.angle_uncertainty(0.02, ja, fit="smooth")
    with pytest.raises(ValueError, match="key_point_weight belongs to fit='refine'"):
        ik.angle_uncertainty(0.02, ja, key_point_weight=1.0)
    # the refinement and its error bars, both answered by the host-run rules
    monkeypatch.setattr(hiplib, "_call", harness_call(refine_sens_harness, refine_rule_harness, real_call))
    refined, _ = ik.run_refine(ja)
    out = ik.run_refine_sensitivity(refined)
    assert list(out) == ["RF_leg", "LF_leg"]
    for l in legs:
        res = out[f"{l}_leg"]
        assert sorted(res) == ["flags", "grad", "sens"]
        assert res["sens"].shape == (N, 7, 4, 3) and res["flags"].shape == (N,) and res["grad"].shape == (N,)
        assert res["flags"].dtype == np.int32 and not (res["flags"] & ~0x7F).any() and np.isfinite(res["sens"]).all()
        stopped_on_gradient = reason(ik.refine_report[l]["info"]) == 0
        assert (res["grad"][stopped_on_gradient] <= GTOL).all() and np.median(res["grad"]) < 1e-8
        seg = [ik.kinematic_chain_class.body_size[f"{l}_{s}"] for s in SEGMENTS]
        bounds = np.array([ik.kinematic_chain_class.bounds_dof[f"{l}_{d}"] for d in DOFS])
        ang = np.stack([refined[f"Angle_{l}_{d}"] for d in DOFS], 1)
        ref = refine_sens_harness.run(ang, z[f"{l}_pose"][:, :5], seg, bounds)
        assert same_bits(res["sens"], ref["sens"]) and np.array_equal(res["flags"], ref["flags"])
        assert same_bits(res["grad"], ref["grad"])
        # the sequential angles are not a minimum of the whole-leg fit, and grad says so
        seq = refine_sens_harness.run(z[f"{l}_angles"], z[f"{l}_pose"][:, :5], seg, bounds)
        assert np.median(seq["grad"]) > 1e3 * GTOL
    # sigma: a scalar, (4,), (N, 4) and a per-leg dictionary; std is the numpy reduction of sens
    for sigma in (0.02, np.array([0.01, 0.02, 0.03, 0.04]), sig_n4, {"RF": 0.02, "LF": sig_n4}):
        unc = ik.angle_uncertainty(sigma, refined, fit="refine")
        assert list(unc) == [f"Angle_{l}_{d}" for l in legs for d in DOFS]
        for l in legs:
            s = sigma[l] if isinstance(sigma, dict) else sigma
            ref = numpy_std(out[f"{l}_leg"]["sens"], np.broadcast_to(s, (N, 4)))
            got = np.stack([unc[f"Angle_{l}_{d}"] for d in DOFS], 1)
            held = (out[f"{l}_leg"]["flags"][:, None] >> np.arange(7)) & 1 == 1
            assert got.shape == (N, 7) and np.allclose(got, ref, rtol=1e-14, atol=0)
            assert not got[held].any() and (got[~held] > 0).all()     # 0 for a held joint and nowhere else
    with pytest.raises(ValueError, match="key_point_sigma must be a scalar"):
        ik.angle_uncertainty(np.ones((N, 3)), refined, fit="refine")
    # weights reach the rule: a key point without weight has no influence
    w = np.array([1.0, 0.0, 1.0, 1.0])
    refined_w, _ = ik.run_refine(ja, key_point_weight=w)
    out_w = ik.run_refine_sensitivity(refined_w, key_point_weight=w)
    assert not out_w["RF_leg"]["sens"][:, :, 1].any() and np.nansum(np.abs(out_w["RF_leg"]["sens"][:, :, [0, 2, 3]])) > 0
    unc_w = ik.angle_uncertainty(0.02, refined_w, fit="refine", key_point_weight=w)
    assert np.allclose(unc_w["Angle_RF_ThC_yaw"], numpy_std(out_w["RF_leg"]["sens"], np.full((N, 4), 0.02))[:, 0], rtol=1e-14,
                       equal_nan=True)
    # the stored angles are the default
    ik.joint_angles_dict = refined
    assert same_bits(ik.run_refine_sensitivity()["LF_leg"]["sens"], out["LF_leg"]["sens"])
    # _lib.refine_sensitivity: what is asked for, and nothing else
    params = [ik._leg_params(l) for l in legs]
    ang = np.stack([np.stack([refined[f"Angle_{l}_{d}"] for d in DOFS], 1) for l in legs])[None]
    pose = np.stack([z[f"{l}_pose"][:, :5] for l in legs])[None]
    only = hiplib.refine_sensitivity(ang, pose, params, kp_sigma=0.02, want_sens=False, want_grad=False, want_flags=False)
    assert only["sens"] is None and only["flags"] is None and only["grad"] is None and only["std"].shape == (1, 2, N, 7)
    full = hiplib.refine_sensitivity(ang, pose, params)
    assert full["std"] is None and full["sens"].shape == (1, 2, N, 7, 4, 3) and full["flags"].shape == (1, 2, N)
    assert full["grad"].shape == (1, 2, N)
    # the generic chain has no such quantity
    zg = load_golden("generic_rf_100")
    gen = LegInvKinGeneric({"RF_leg": zg["RF_pose"]}, KinematicChainGeneric(BOUNDS, ["RF"]), INITIAL_ANGLES, log_level="ERROR")
    for call in (lambda: gen.run_refine_sensitivity(), lambda: gen.angle_uncertainty(0.02, fit="refine")):
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
def test_gpu_kernel_equals_the_host_rule_bit_for_bit(lib, refine_sens_harness, N):  # noqa: F811
    """2 sequences x 3 legs (three different segment sets and limits) x N frames with weights, zero-weight NaN key points
    and bad leg-frames; sens only, std only, flags + grad only and all four; guards around every buffer; the default
    plan (per lane) and the staged quarter-record store path (SEQIK_REFSENS_STAGED=1)."""
    c = gpu_case(refine_sens_harness, N)
    for want in SUBSETS:
        for staged in ("0", "1"):
            check_device_against_host(lib, c, want, staged)
    assert "SEQIK_REFSENS_STAGED" not in os.environ
    check_device_against_host(lib, c, SUBSETS[-1], staged="")     # (an empty value is atoi's 0: the default plan)


@pytest.mark.gpu
def test_gpu_one_workgroup_of_64_in_a_fresh_process(lib, refine_sens_harness, tmp_path):  # noqa: F811
    """SEQIK_REFSENS_BLOCK=64 SEQIK_REFSENS_GRID=1, set in a fresh child process: one wavefront walks the whole range in
    the grid-stride loop -- with the staged store path whole-wavefront trips first and a ragged per-lane trip last --; every
    size, every output subset, per lane and staged."""
    cases = {N: gpu_case(refine_sens_harness, N) for N in GPU_FRAMES}
    path = str(tmp_path / "cases.npz")
    np.savez(path, cases=np.array(cases, dtype=object))
    env = dict(os.environ, SEQIK_REFSENS_BLOCK="64", SEQIK_REFSENS_GRID="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "refine_sens_support.py"), path], env=env,
                         capture_output=True, text=True, timeout=300, cwd=os.path.join(ROOT, "tests"))
    assert out.returncode == 0 and "CHILD OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


@pytest.mark.gpu
def test_gpu_host_entry_point_equals_the_device_entry_point(lib, refine_sens_harness):  # noqa: F811
    import torch
    c = gpu_case(refine_sens_harness, 65)
    S, L, N = c["ang"].shape[:3]
    params = [lib.leg_params_from_arrays(s, b, np.zeros(27)) for s, b in zip(c["segs"], c["bounds"])]
    ref = c["with_std"]
    host = lib.refine_sensitivity(c["ang"], c["pose"], params, kp_weight=c["weight"], kp_sigma=c["sigma"])
    assert all(same_bits(host[k], ref[k]) for k in ("sens", "std", "grad"))
    assert host["flags"].dtype == np.int32 and np.array_equal(host["flags"], ref["flags"])
    plain = lib.refine_sensitivity(c["ang"], c["pose"], params, kp_weight=c["weight"], want_flags=False, want_grad=False)
    assert plain["std"] is None and plain["flags"] is None and plain["grad"] is None
    assert same_bits(plain["sens"], c["no_std"]["sens"])
    off = lib.refine_sensitivity(c["ang"], c["pose"], params, kp_weight=c["weight"], want_sens=False, bound_tol=0.0)
    assert not (off["flags"] & 0x7F).any() and (ref["flags"] & 0x7F).any()
    d_ang, d_pose, d_w, d_sig = (torch.from_numpy(c[k]).cuda() for k in ("ang", "pose", "weight", "sigma"))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_sens = torch.full((S, L, N, 7, 4, 3), 7.0, dtype=torch.float64, device="cuda")
        d_std = torch.full((S, L, N, 7), 7.0, dtype=torch.float64, device="cuda")
        d_grad = torch.full((S, L, N), 7.0, dtype=torch.float64, device="cuda")
        d_flags = torch.full((S, L, N), 7, dtype=torch.int32, device="cuda")
        lib.refine_sensitivity_device(d_ang, d_pose, S, L, N, params, d_kp_weight=d_w, d_kp_sigma=d_sig, d_sens=d_sens,
                                      d_std=d_std, d_grad=d_grad, d_flags=d_flags, stream=s)
    s.synchronize()
    assert same_bits(d_sens.cpu().numpy(), host["sens"]) and same_bits(d_std.cpu().numpy(), host["std"])
    assert same_bits(d_grad.cpu().numpy(), host["grad"]) and np.array_equal(d_flags.cpu().numpy(), host["flags"])
    with pytest.raises(ValueError, match="expected a int32 tensor"):
        lib.refine_sensitivity_device(d_ang, d_pose, S, L, N, params, d_flags=d_std)
    # empty input: no launch, the output is not touched
    keep = d_sens.clone()
    lib.refine_sensitivity_device(d_ang.data_ptr(), d_pose.data_ptr(), 0, L, N, params, d_sens=d_sens.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(keep.view(torch.int64), d_sens.view(torch.int64))


@pytest.mark.gpu
def test_gpu_run_refine_with_sigma_equals_the_two_host_calls(lib):
    """``run_refine(key_point_sigma=0.01)`` on RF 0:600 of the shipped recording -- the refined angles stay on the device
    between the two kernels -- equals ``refine_legs`` then ``refine_sensitivity`` through host buffers, bit for bit."""
    from seqikpy_amd.data import BOUNDS, INITIAL_ANGLES
    from seqikpy_amd.kinematic_chain import KinematicChainSeq
    from seqikpy_amd.leg_inverse_kinematics import LegInvKinSeq
    z = load_golden("anipose_shipped")
    pose = z["RF_pose"][:600]
    ik = LegInvKinSeq({"RF_leg": pose}, KinematicChainSeq(BOUNDS, ["RF"]), INITIAL_ANGLES, log_level="ERROR")
    ja = {f"Angle_RF_{d}": z["RF_angles"][:600, i] for i, d in enumerate(DOFS)}
    refined, fk = ik.run_refine(ja, key_point_sigma=0.01)
    report = ik.refine_report["RF"]
    assert sorted(report) == ["cost", "info", "sens_flags", "std"] and report["std"].shape == (600, 7)
    params = [ik._leg_params("RF")]
    ang = z["RF_angles"][:600][None, None]
    kp = ik._fk_key_points("RF", pose)[None, None]
    first = lib.refine_legs(ang, kp, params)
    second = lib.refine_sensitivity(first["angles"], kp, params, kp_sigma=0.01, want_sens=False, want_grad=False)
    assert same_bits(np.stack([refined[f"Angle_RF_{d}"] for d in DOFS], 1), first["angles"][0, 0])
    assert same_bits(report["cost"], first["cost"][0, 0]) and np.array_equal(report["info"], first["info"][0, 0])
    assert same_bits(report["std"], second["std"][0, 0]) and np.array_equal(report["sens_flags"], second["flags"][0, 0])
    assert np.isfinite(report["std"]).all() and (report["std"][report["sens_flags"] == 0] > 0).all()
    # without the argument nothing changes, and angle_uncertainty(fit="refine") is the same quantity
    plain, fk_plain = ik.run_refine(ja)
    assert sorted(ik.refine_report["RF"]) == ["cost", "info"]
    assert all(same_bits(plain[k], refined[k]) for k in refined) and same_bits(fk_plain["RF_leg"], fk["RF_leg"])
    unc = ik.angle_uncertainty(0.01, refined, fit="refine")
    assert same_bits(np.stack([unc[f"Angle_RF_{d}"] for d in DOFS], 1), report["std"])
