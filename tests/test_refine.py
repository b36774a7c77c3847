"""Whole-leg refinement of the sequential fit (include/seqik_refine.h, csrc/seqik_refine.hpp / seqik_refine.hip).

CPU tier: the header, the signature table and the exports; every SEQIK_ERR_BAD_ARG case through the C ABI without a GPU;
the properties the rule has by construction on 40 made-up legs, run on the host (tests/harness/refine_harness.hip); the
bad-input kinds; the Python surface -- ``_lib.refine_legs``, ``LegInvKinSeq.run_refine`` -- on the df3d fixture with the
library calls answered by the host-run rules.  GPU tier (``-m gpu``): the kernel against the host-run rule bit for bit over
sizes around the wavefront, block sizes, a grid of one workgroup, one wavefront with a mix of short, long, bad and capped
lanes, weights / cost / info given and null, in place, with guard records; both entry points; ``run_refine`` chained on
``run_ik_and_fk``.

Against scipy and the 200-bit gradient: tests/test_refine_accuracy.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from angle_map_support import gpu_lib, same_bits, switches
from conftest import DOFS, ROOT, load_golden, random_leg_case
from refine_support import (BAD_INPUT, FTOL, GTOL, MAX_ITER, SEED_OF_DOF, harness_call, held_bits, host_batch, iterations,  # noqa: F401
                            made_up_legs, numpy_refine, reason, refine_harness, shipped_frames)
from test_capi_symbols import assert_same_class, header_prototypes

REFINE_SYMBOLS = ["seqik_refine_legs", "seqik_refine_legs_device"]


# ---------------------------------------------------------------------------------------------------------------------
# CPU tier
# ---------------------------------------------------------------------------------------------------------------------

def test_refine_header_declares_exactly_the_new_entry_points(hiplib):
    raw = open(os.path.join(ROOT, "include", "seqik_refine.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(seqik_[a-z_]+)\s*\(", text)))
    assert declared == sorted(REFINE_SYMBOLS)
    assert sorted(hiplib.REFINE_SIGNATURES) == ["seqik_refine.h"]
    assert hiplib.REFINE_EXPORTED_SYMBOLS == [s[0] for s in hiplib.REFINE_SIGNATURES["seqik_refine.h"]]
    assert sorted(hiplib.REFINE_EXPORTED_SYMBOLS) == declared
    # disjoint from every other table and list
    tables = (hiplib.SIGNATURES, hiplib.EXTENSION_SIGNATURES, hiplib.STREAM_GAPS_SIGNATURES, hiplib.JACOBIAN_SIGNATURES,
              hiplib.SENSITIVITY_SIGNATURES)
    assert not set(declared) & {s[0] for table in tables for sigs in table.values() for s in sigs}
    for name in ("EXPORTED_SYMBOLS", "FK_EXPORTED_SYMBOLS", "FRAMES_EXPORTED_SYMBOLS", "JACOBIAN_EXPORTED_SYMBOLS",
                 "GAPS_EXPORTED_SYMBOLS", "SENSITIVITY_EXPORTED_SYMBOLS"):
        assert not set(declared) & set(getattr(hiplib, name)), name
    for table in tables:
        assert "seqik_refine.h" not in table
    lib = hiplib.load()
    assert lib.seqik_abi_version() == 7 == hiplib.ABI_VERSION
    assert "seqik_refine.hip" in hiplib.COMPILE_UNITS and "seqik_refine.hpp" in hiplib.CSRC_HEADERS
    assert "seqik_refine" not in " ".join(hiplib.KERNEL_SOURCES + hiplib.LATENCY_SOURCES)
    assert '"seqik_refine.h"' in open(os.path.join(ROOT, "setup.py")).read()
    for macro, value, const in (("SEQIK_REFINE_MAX_ITER", "200", hiplib.REFINE_MAX_ITER), ("SEQIK_REFINE_GTOL", "1e-10", hiplib.REFINE_GTOL),
                                ("SEQIK_REFINE_FTOL", "1e-14", hiplib.REFINE_FTOL)):
        assert f"#define {macro} {value}\n" in raw and const == float(value), macro
    assert (hiplib.REFINE_MAX_ITER, hiplib.REFINE_GTOL, hiplib.REFINE_FTOL) == (MAX_ITER, GTOL, FTOL)
    assert "#define SEQIK_REFINE_BAD_INPUT (1 << 24)\n" in raw and hiplib.REFINE_BAD_INPUT == BAD_INPUT
    # the options struct: int32, double, double with C's padding
    assert ctypes.sizeof(hiplib.SeqikRefineOptions) == 24 and hiplib.SeqikRefineOptions.gtol.offset == 8
    # the table against the prototypes: count and class, and what the loaded library is bound with
    protos = header_prototypes("seqik_refine.h")
    table = {sig[0]: sig[1:] for sig in hiplib.REFINE_SIGNATURES["seqik_refine.h"]}
    assert sorted(table) == sorted(protos) == declared
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name][0], list(table[name][1:])
        assert len(argtypes) == len(params) == 13, (name, params)
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
    ang, pose, wgt = np.zeros((1, 2, 3, 7)), np.zeros((1, 2, 3, 5, 3)), np.ones((1, 2, 3, 4))
    out, cst, inf = np.zeros((1, 2, 3, 7)), np.zeros((1, 2, 3, 2)), np.zeros((1, 2, 3), np.int32)
    a, p, w, o, c, f = (ang.ctypes.data_as(dp), pose.ctypes.data_as(dp), wgt.ctypes.data_as(dp), out.ctypes.data_as(dp),
                        cst.ctypes.data_as(dp), inf.ctypes.data_as(ip))
    good = (hiplib.SeqikLegParams * 2)()
    for l in range(2):
        for i in range(4):
            good[l].seg[i] = 0.5
    bad_seg = (hiplib.SeqikLegParams * 2)()
    bad_seg[1].seg[2] = np.inf
    huge = 2 ** 63 // (8 * 15) + 1
    opt = lambda *v: ctypes.byref(hiplib.SeqikRefineOptions(*v))  # noqa: E731
    #        angles pose n_seq n_legs n_frames legs kind kp_weight opt angles_out cost info
    cases = [("n_legs", (a, p, 1, 0, 3, good, 0, None, None, o, c, f)), ("n_legs", (a, p, 1, 9, 3, good, 0, w, None, o, None, None)),
             ("negative", (a, p, -1, 2, 3, good, 0, None, None, o, c, f)), ("negative", (a, p, 1, 2, -3, good, 0, None, None, o, c, f)),
             ("angles must", (None, p, 1, 2, 3, good, 0, None, None, o, c, f)), ("pose must", (a, None, 1, 2, 3, good, 0, None, None, o, c, f)),
             ("angles_out must", (a, p, 1, 2, 3, good, 0, None, None, None, c, f)), ("legs", (a, p, 1, 2, 3, None, 0, None, None, o, c, f)),
             ("not built", (a, p, 1, 2, 3, good, 1, None, None, o, c, f)), ("not built", (a, p, 1, 2, 3, good, 1, w, opt(5, 0.0, 0.0), o, None, None)),
             ("kind", (a, p, 1, 2, 3, good, 2, None, None, o, c, f)), ("kind", (a, p, 1, 2, 3, good, -1, None, None, o, c, f)),
             ("segment", (a, p, 1, 2, 3, bad_seg, 0, None, None, o, c, f)),
             ("max_iter", (a, p, 1, 2, 3, good, 0, None, opt(0, 1e-10, 1e-14), o, c, f)),
             ("max_iter", (a, p, 1, 2, 3, good, 0, None, opt(256, 1e-10, 1e-14), o, c, f)),
             ("max_iter", (a, p, 1, 2, 3, good, 0, None, opt(-1, 1e-10, 1e-14), o, c, f)),
             ("gtol", (a, p, 1, 2, 3, good, 0, None, opt(10, -1e-10, 1e-14), o, c, f)), ("gtol", (a, p, 1, 2, 3, good, 0, None, opt(10, np.nan, 1e-14), o, c, f)),
             ("gtol", (a, p, 1, 2, 3, good, 0, None, opt(10, np.inf, 1e-14), o, c, f)),
             ("ftol", (a, p, 1, 2, 3, good, 0, None, opt(10, 1e-10, -1e-14), o, c, f)), ("ftol", (a, p, 1, 2, 3, good, 0, None, opt(10, 1e-10, np.nan), o, c, f)),
             ("ftol", (a, p, 1, 2, 3, good, 0, None, opt(10, 1e-10, np.inf), o, c, f)),
             ("too many", (a, p, huge, 1, 1, good, 0, None, None, o, c, f)), ("too many", (a, p, 1, 1, huge, good, 0, None, None, o, None, None)),
             ("too many", (a, p, 2 ** 40, 2, 2 ** 40, good, 0, None, None, o, c, f))]
    for what, args in cases:
        for fn, last in ((lib.seqik_refine_legs, -1), (lib.seqik_refine_legs_device, None)):
            assert fn(*args, last) == hiplib.ERR_ARG, (what, fn.__name__)
            msg = lib.seqik_last_error().decode()
            assert msg.startswith("seqik_refine_legs: ") and what in msg, (what, msg)
    for args in ((a, p, 0, 2, 3, good, 0, None, None, o, c, f), (a, p, 1, 2, 0, good, 0, w, opt(1, 0.0, 0.0), o, c, f)):
        assert lib.seqik_refine_legs(*args, -1) == 0 and lib.seqik_refine_legs_device(*args, None) == 0
    assert not out.any() and not cst.any() and not inf.any()
    # the Python wrappers: shapes and arguments
    params = [hiplib.leg_params_from_arrays(np.full(4, 0.5), np.zeros((7, 2)), np.zeros(27))] * 2
    with pytest.raises(ValueError, match="pose must have shape"):
        hiplib.refine_legs(ang, pose[..., :4, :], params)
    with pytest.raises(ValueError, match="kp_weight must broadcast"):
        hiplib.refine_legs(ang, pose, params, kp_weight=np.ones(3))
    with pytest.raises(ValueError, match=r"shape \(S, L, N, 7\)"):
        hiplib.refine_legs(ang[0], pose, params)
    with pytest.raises(ValueError, match="max_iter must lie in 1..255"):
        hiplib.refine_legs(ang, pose, params, max_iter=0)


def test_structure_on_the_made_up_legs(refine_harness):  # noqa: F811
    """40 made-up legs x 24 frames, started from their seeds: what the rule promises by construction, by <= and ==."""
    seen = np.zeros(8, dtype=int)
    on_limit = moved_a_lot = n_capped = 0
    for ang, pose, seg, bounds in made_up_legs():
        out, cost, info = refine_harness.run(ang, pose, seg, bounds)
        lb, ub = bounds[:, 0], bounds[:, 1]
        assert not (info & BAD_INPUT).any() and np.isfinite(out).all() and np.isfinite(cost).all()
        assert (cost[:, 1] <= cost[:, 0]).all()
        assert (out >= lb).all() and (out <= ub).all()
        held = held_bits(info)
        assert ((out == lb) | (out == ub))[held].all()          # a held DOF sits on a limit exactly
        assert (iterations(info) <= MAX_ITER).all() and not (info & ~0xFF077F).any()
        assert np.isin(reason(info), (0, 1, 2, 4)).all()
        assert (cost[iterations(info) == 0, 1] == cost[iterations(info) == 0, 0]).all()
        seen += np.bincount(reason(info), minlength=8)
        on_limit += held.sum()
        moved_a_lot += (cost[:, 1] < 0.5 * cost[:, 0]).sum()
        # a cap of three: a lane that reports the cap reports three iterations; the others are the uncapped lanes
        out3, cost3, info3 = refine_harness.run(ang, pose, seg, bounds, max_iter=3)
        capped = reason(info3) == 4
        n_capped += capped.sum()
        assert (iterations(info3)[capped] == 3).all() and (iterations(info3) <= 3).all()
        assert (cost3[:, 1] <= cost3[:, 0]).all() and (cost[:, 1] <= cost3[:, 1]).all()    # the capped run is a prefix
        assert same_bits(out3[~capped], out[~capped]) and np.array_equal(info3[~capped], info[~capped])
        # a result that met the gradient test is a start that meets it: its clamped bits, no iteration
        done = reason(info) == 0
        again, cost_again, info_again = refine_harness.run(out[done], pose[done], seg, bounds)
        assert same_bits(again, out[done]) and not iterations(info_again).any() and not reason(info_again).any()
        assert same_bits(cost_again[:, 0], cost[done, 1]) and same_bits(cost_again[:, 1], cost[done, 1])
        assert np.array_equal(info_again & 0x7F, info[done] & 0x7F)
    assert seen[0] > 100 and on_limit > 100 and moved_a_lot > 100 and n_capped > 100     # the cases are not trivial


def test_the_host_rule_agrees_with_the_numpy_restatement(refine_harness):  # noqa: F811
    """The harness and the float64 restatement (np.cross, np.linalg.cholesky on the free DOFs) walk the same rule.  After
    ONE accepted step they agree to rounding: with lambda >= 1e-3 the scaled matrix of the step has a condition number
    <= 7 (1 + lambda) / lambda ~ 7e3, so a step of size <= 2 pi differs by ~7e3 x 2 pi x a few eps ~ 1e-11 rad; the
    bar is 1e-9 rad and 1e-9 of the cost.  Whole runs are held to the 200-bit gradient (test_refine_accuracy.py), not to
    numpy's bits: a made-up target can sit where two descents part."""
    n_compared = 0
    for ang, pose, seg, bounds in made_up_legs()[:10]:
        out, cost, info = refine_harness.run(ang, pose, seg, bounds, max_iter=1)
        for i in range(len(ang)):
            q, c, f = numpy_refine(ang[i], pose[i], seg, bounds, max_iter=1)
            assert np.isclose(c[0], cost[i, 0], rtol=1e-13, atol=0)
            if f != info[i]:            # a held verdict or an acceptance decided by the last bit: not comparable
                continue
            n_compared += 1
            assert np.abs(q - out[i]).max() <= 1e-9 and np.isclose(c[1], cost[i, 1], rtol=1e-9, atol=0), (i, q, out[i])
    assert n_compared >= 200
    # whole runs on every tenth shipped frame: the same minimum, so the same cost to the bar the scipy test uses (a stop
    # on ftol leaves a relative slack the size of the last decrease); both stop on the gradient or on the decrease
    for leg, fr, ang, pose, seg, bounds in shipped_frames():
        out, cost, info = refine_harness.run(ang[::10], pose[::10], seg, bounds)
        for i in range(len(out)):
            q, c, f = numpy_refine(ang[10 * i], pose[10 * i], seg, bounds)
            assert c[0] == cost[i, 0] or np.isclose(c[0], cost[i, 0], rtol=1e-13, atol=0)
            assert np.isclose(c[1], cost[i, 1], rtol=1e-9, atol=0) and (f >> 8) & 7 in (0, 1), (leg, fr[10 * i])


def _bad_input_case():
    leg, fr, ang, pose, seg, bounds = shipped_frames()[0]
    return ang[:24].copy(), pose[:24].copy(), np.ones((24, 4)), seg, bounds


def test_bad_input_gives_nan_rows_and_leaves_the_neighbours_alone(refine_harness):  # noqa: F811
    ang, pose, wgt, seg, bounds = _bad_input_case()
    ref, ref_cost, ref_info = refine_harness.run(ang, pose, seg, bounds, weight=wgt)
    assert same_bits(ref, refine_harness.run(ang, pose, seg, bounds)[0])          # weights of 1 are no weights
    kinds = {"nan angle": ("a", (2, 3), np.nan), "inf angle": ("a", (4, 0), -np.inf), "angle beyond 2^30": ("a", (6, 6), 1.1e9),
             "nan weight": ("w", (8, 1), np.nan), "inf weight": ("w", (10, 0), np.inf), "negative weight": ("w", (12, 3), -1.0),
             "nan origin": ("p", (14, 0, 1), np.nan), "inf key point": ("p", (16, 3, 2), np.inf),
             "nan key point": ("p", (18, 4, 0), np.nan)}
    a, p, w = ang.copy(), pose.copy(), wgt.copy()
    for name, (which, idx, value) in kinds.items():
        dict(a=a, p=p, w=w)[which][idx] = value
    out, cost, info = refine_harness.run(a, p, seg, bounds, weight=w)
    bad = np.zeros(24, dtype=bool)
    bad[[idx[0] for _, idx, _ in kinds.values()]] = True
    assert (info[bad] == BAD_INPUT).all() and np.isnan(out[bad]).all() and np.isnan(cost[bad]).all()
    assert same_bits(out[~bad], ref[~bad]) and same_bits(cost[~bad], ref_cost[~bad]) and np.array_equal(info[~bad], ref_info[~bad])
    # a non-finite segment length reaches the rule only here (the C ABI refuses it): every lane of that leg is bad
    seg_bad = np.array(seg, dtype=float)
    seg_bad[1] = np.nan
    o2, c2, i2 = refine_harness.run(ang, pose, seg_bad, bounds)
    assert (i2 == BAD_INPUT).all() and np.isnan(o2).all() and np.isnan(c2).all()
    # weight exactly 0: the key point is not read -- NaN there gives the bits of a finite value there
    w0 = wgt.copy()
    w0[5, 2], w0[7, 3], w0[9, :] = 0.0, 0.0, 0.0
    p_nan, p_fin = pose.copy(), pose.copy()
    p_nan[5, 3], p_nan[7, 4, 1], p_nan[9, 1:] = np.nan, np.inf, np.nan
    p_fin[5, 3], p_fin[7, 4, 1], p_fin[9, 1:] = 123.0, -4.0, 0.5
    got, want = refine_harness.run(ang, p_nan, seg, bounds, weight=w0), refine_harness.run(ang, p_fin, seg, bounds, weight=w0)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert not (got[2] & BAD_INPUT).any() and not got[1][9].any()         # no weight at all: cost 0, nothing to do
    assert not same_bits(got[0][5], ref[5])                               # and the weight does count
    # in place: angles_out is angles
    inplace = refine_harness.run(a, p, seg, bounds, weight=w, in_place=True)
    assert same_bits(inplace[0], out) and same_bits(inplace[1], cost) and np.array_equal(inplace[2], info)
    # cost and info are optional
    only = refine_harness.run(a, p, seg, bounds, weight=w, want_cost=False, want_info=False)
    assert only[1] is None and only[2] is None and same_bits(only[0], out)


def test_python_surface_on_the_df3d_fixture(hiplib, refine_harness, monkeypatch):  # noqa: F811
    from seqikpy_amd.data import BOUNDS, INITIAL_ANGLES, SEGMENTS
    from seqikpy_amd.kinematic_chain import KinematicChainGeneric, KinematicChainSeq
    from seqikpy_amd.leg_inverse_kinematics import LegInvKinGeneric, LegInvKinSeq
    monkeypatch.setattr(hiplib, "_call", harness_call(refine_harness, hiplib._call))
    z = load_golden("df3d_100")
    legs, N = ["RF", "LF"], 100
    ik = LegInvKinSeq({f"{l}_leg": z[f"{l}_pose"] for l in legs}, KinematicChainSeq(BOUNDS, legs), INITIAL_ANGLES,
                      log_level="ERROR")
    ja = {f"Angle_{l}_{d}": z[f"{l}_angles"][:, i].copy() for l in legs for i, d in enumerate(DOFS)}
    ik.joint_angles_dict = {k: v.copy() for k, v in ja.items()}
    stored = ik.joint_angles_dict
    angles, fk = ik.run_refine()
    # keys and shapes as run_ik_and_fk returns them (the fixture holds its outputs)
    assert list(angles) == list(ja) and all(v.shape == (N,) for v in angles.values())
    assert list(fk) == ["RF_leg", "LF_leg"] and all(v.shape == z["RF_fk"].shape == (N, 9, 3) for v in fk.values())
    assert ik.joint_angles_dict is stored and all(same_bits(stored[k], ja[k]) for k in ja)
    assert list(ik.refine_report) == legs
    before, after = ik.fit_error(ja), ik.fit_error(angles)
    for l in legs:
        rep = ik.refine_report[l]
        assert rep["cost"].shape == (N, 2) and rep["info"].shape == (N,) and rep["info"].dtype == np.int32
        seg = [ik.kinematic_chain_class.body_size[f"{l}_{s}"] for s in SEGMENTS]
        bounds = np.array([ik.kinematic_chain_class.bounds_dof[f"{l}_{d}"] for d in DOFS])
        ref, ref_cost, ref_info = refine_harness.run(z[f"{l}_angles"], z[f"{l}_pose"][:, :5], seg, bounds)
        got = np.stack([angles[f"Angle_{l}_{d}"] for d in DOFS], 1)
        assert same_bits(got, ref) and same_bits(rep["cost"], ref_cost) and np.array_equal(rep["info"], ref_info)
        assert (got >= bounds[:, 0]).all() and (got <= bounds[:, 1]).all()
        # the refined angles fit no worse: the summed squared distances per leg, and they are what cost reports
        assert (after[f"{l}_leg"] ** 2).sum() <= (before[f"{l}_leg"] ** 2).sum()
        assert (after[f"{l}_leg"] ** 2).sum() < 0.9 * (before[f"{l}_leg"] ** 2).sum()
        # (f + o) - pose[k] against f - (pose[k] - o): ~1e-16 of a coordinate on a distance d >= 1e-4, so ~1e-11 of d^2
        assert np.allclose((after[f"{l}_leg"] ** 2).sum(1), rep["cost"][:, 1], rtol=1e-9, atol=0)
        assert same_bits(fk[f"{l}_leg"][:, 0], z[f"{l}_pose"][:, 0])            # FK of the refined angles, at the leg's origin
        assert np.allclose(np.linalg.norm(fk[f"{l}_leg"][:, [4, 6, 7, 8]] - z[f"{l}_pose"][:, 1:5], axis=2), after[f"{l}_leg"],
                           rtol=0, atol=1e-14)
    # explicit angles equal the stored default; the weights broadcast: a scalar, (4,), (N, 4), a per-leg dictionary
    assert all(same_bits(v, angles[k]) for k, v in ik.run_refine(ja)[0].items())
    w4, wn4 = np.array([1.0, 2.0, 0.5, 3.0]), np.random.default_rng(5).uniform(0.2, 2.0, (N, 4))
    for weight in (2.0, w4, wn4, {"RF": w4, "LF": wn4}):
        got = ik.run_refine(key_point_weight=weight, max_iter=20)[0]
        for l in legs:
            w = weight[l] if isinstance(weight, dict) else weight
            seg = [ik.kinematic_chain_class.body_size[f"{l}_{s}"] for s in SEGMENTS]
            bounds = np.array([ik.kinematic_chain_class.bounds_dof[f"{l}_{d}"] for d in DOFS])
            ref = refine_harness.run(z[f"{l}_angles"], z[f"{l}_pose"][:, :5], seg, bounds, weight=np.broadcast_to(w, (N, 4)),
                                     max_iter=20)[0]
            assert same_bits(np.stack([got[f"Angle_{l}_{d}"] for d in DOFS], 1), ref)
    with pytest.raises(ValueError, match="key_point_weight must be a scalar"):
        ik.run_refine(key_point_weight=np.ones((N, 3)))
    with pytest.raises(ValueError, match="unknown refinement options"):
        ik.run_refine(xtol=1e-3)
    doc = " ".join(LegInvKinSeq.run_refine.__doc__.split())
    assert "REFINED INDEPENDENTLY" in doc and "more than a radian" in doc
    # _lib.refine_legs: what is asked for, and nothing else
    params = [ik._leg_params(l) for l in legs]
    ang = np.stack([z[f"{l}_angles"] for l in legs])[None]
    pose = np.stack([z[f"{l}_pose"][:, :5] for l in legs])[None]
    only = hiplib.refine_legs(ang, pose, params, want_cost=False, want_info=False)
    assert only["cost"] is None and only["info"] is None and only["angles"].shape == (1, 2, N, 7)
    # the generic chain is not built
    zg = load_golden("generic_rf_100")
    gen = LegInvKinGeneric({"RF_leg": zg["RF_pose"]}, KinematicChainGeneric(BOUNDS, ["RF"]), INITIAL_ANGLES, log_level="ERROR")
    with pytest.raises(NotImplementedError, match="sequential chain only"):
        gen.run_refine()


# ---------------------------------------------------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(hiplib):
    return gpu_lib(hiplib)


SENTINEL, SENTINEL_I = -12345.678, -1234567
WIDTH = dict(angles_out=7, cost=2, info=1)


def _params_of(lib, segs, bounds):
    return [lib.leg_params_from_arrays(s, b, np.zeros(27)) for s, b in zip(segs, bounds)]


def made_up_batch(seed, S, L, N):
    """S x L x N leg-frames of L made-up legs (different segments and limits), started from the legs' seeds, with weights
    and -- from 15 leg-frames on -- one lane of every bad-input kind and a weightless key point that holds NaN.
    -> ang (S, L, N, 7), pose (S, L, N, 5, 3), weight (S, L, N, 4), segs, bounds"""
    rng = np.random.default_rng(seed)
    ang, pose, segs, bounds = np.empty((S, L, N, 7)), np.empty((S, L, N, 5, 3)), [], []
    for l in range(L):
        p, seg, b, seeds = random_leg_case(rng, S * N)
        pose[:, l], ang[:, l] = p.reshape(S, N, 5, 3), seeds[SEED_OF_DOF]
        segs.append(seg)
        bounds.append(b)
    weight = rng.uniform(0.25, 2.0, (S, L, N, 4))
    fa, fp, fw = ang.reshape(-1, 7), pose.reshape(-1, 5, 3), weight.reshape(-1, 4)
    n = len(fa)
    if n >= 15:
        fa[n // 3, 4], fa[n - 1, 0] = np.nan, 1e300
        fp[n // 2, 2, 1], fp[3, 0, 0] = np.inf, np.nan
        fw[5, 2], fw[7, 1] = np.nan, -0.5
        fw[9, 3], fp[9, 4] = 0.0, np.nan
    return ang, pose, weight, np.array(segs), np.array(bounds)


_CASES = {}


def case(rh, S, L, N, seed, **opts):
    """Inputs and the host-run rule's answers for them -- with the weights and without -- computed once per size."""
    key = (S, L, N, seed, tuple(sorted(opts.items())))
    if key not in _CASES:
        ang, pose, weight, segs, bounds = made_up_batch(seed, S, L, N)
        _CASES[key] = (ang, pose, weight, segs, bounds, host_batch(rh, ang, pose, segs, bounds, weight, **opts),
                       host_batch(rh, ang, pose, segs, bounds, None, **opts))
    return _CASES[key]


def device_run(lib, ang, pose, weight, segs, bounds, want=("cost", "info"), in_place=False, env=None, **opts):
    """The device entry point on torch tensors with one guard record on each side of every buffer it writes, all filled
    with a sentinel -> {name: array}; asserts that the guards and the outputs not asked for are untouched."""
    import torch
    S, L, N = ang.shape[:3]
    n = S * L * N
    d_pose = torch.from_numpy(np.ascontiguousarray(pose)).cuda()
    d_w = None if weight is None else torch.from_numpy(np.ascontiguousarray(weight)).cuda()
    bufs = {k: torch.full(((n + 2) * w,), SENTINEL_I if k == "info" else SENTINEL,
                          dtype=torch.int32 if k == "info" else torch.float64, device="cuda") for k, w in WIDTH.items()}
    ptr = {k: bufs[k].data_ptr() + bufs[k].element_size() * WIDTH[k] for k in WIDTH}
    if in_place:      # the start sits inside the guarded output buffer
        bufs["angles_out"][7:-7] = torch.from_numpy(np.ascontiguousarray(ang).reshape(-1)).cuda()
        d_ang = ptr["angles_out"]
    else:
        d_ang = torch.from_numpy(np.ascontiguousarray(ang)).cuda()
    with switches(**(env or {})):
        lib.refine_legs_device(d_ang if in_place else d_ang.data_ptr(), d_pose.data_ptr(), S, L, N, _params_of(lib, segs, bounds),
                               ptr["angles_out"], d_kp_weight=0 if d_w is None else d_w.data_ptr(),
                               d_cost=ptr["cost"] if "cost" in want else 0, d_info=ptr["info"] if "info" in want else 0,
                               stream=torch.cuda.current_stream().cuda_stream, **opts)
        torch.cuda.synchronize()
    out = {}
    for k, w in WIDTH.items():
        got, sent = bufs[k].cpu().numpy(), SENTINEL_I if k == "info" else SENTINEL
        assert (got[:w] == sent).all() and (got[-w:] == sent).all(), (k, "guard", want, env)
        if k == "angles_out" or k in want:
            out[k] = got[w:-w].reshape((S, L, N, w) if w > 1 else (S, L, N))
        else:
            assert (got == sent).all(), (k, "not requested", want, env)
    return out


def assert_equals_host(got, ref, where):
    assert same_bits(got["angles_out"], ref[0]), where
    if "cost" in got:
        assert same_bits(got["cost"], ref[1]), where
    if "info" in got:
        assert np.array_equal(got["info"], ref[2]), where


FRAMES = (1, 63, 64, 65, 257)


@pytest.mark.gpu
def test_gpu_kernel_equals_the_host_rule_bit_for_bit(lib, refine_harness):  # noqa: F811
    """2 sequences x 3 legs (three different segment sets and limits: wavefronts straddle leg and sequence seams) x 1 ..
    257 frames; weights given and null, cost and info null, in place; guards around every buffer."""
    for i, N in enumerate(FRAMES):
        ang, pose, weight, segs, bounds, ref_w, ref_1 = case(refine_harness, 2, 3, N, 300 + i)
        assert_equals_host(device_run(lib, ang, pose, weight, segs, bounds), ref_w, (N, "weights"))
        assert_equals_host(device_run(lib, ang, pose, None, segs, bounds), ref_1, (N, "no weights"))
        assert_equals_host(device_run(lib, ang, pose, weight, segs, bounds, want=()), ref_w, (N, "angles only"))
        assert_equals_host(device_run(lib, ang, pose, weight, segs, bounds, want=("info",)), ref_w, (N, "no cost"))
        assert_equals_host(device_run(lib, ang, pose, weight, segs, bounds, in_place=True), ref_w, (N, "in place"))
    assert (ref_w[2] == BAD_INPUT).sum() >= 6 and np.isnan(ref_w[0][ref_w[2] == BAD_INPUT]).all()


@pytest.mark.gpu
def test_gpu_block_sizes_and_a_grid_of_one_workgroup(lib, refine_harness):  # noqa: F811
    """SEQIK_REFINE_BLOCK 64 and 256 at sizes around the workgroup; SEQIK_REFINE_GRID = 1 at 2 x 3 x 257 leg-frames, so that
    the one workgroup makes several trips of the grid-stride loop and the last trip is ragged."""
    for block in ("64", "128", "256"):
        for i, N in enumerate(FRAMES):
            if N in (65, 257):
                ang, pose, weight, segs, bounds, ref_w, _ = case(refine_harness, 2, 3, N, 300 + i)
                got = device_run(lib, ang, pose, weight, segs, bounds, env=dict(SEQIK_REFINE_BLOCK=block))
                assert_equals_host(got, ref_w, (N, block))
        ang, pose, weight, segs, bounds, ref_w, _ = case(refine_harness, 2, 3, 257, 304)
        for in_place in (False, True):
            got = device_run(lib, ang, pose, weight, segs, bounds, in_place=in_place,
                             env=dict(SEQIK_REFINE_GRID="1", SEQIK_REFINE_BLOCK=block))
            assert_equals_host(got, ref_w, ("grid 1", block, in_place))


def mixed_wavefront(rh):
    """1 x 2 x 32 leg-frames of the shipped recording, one wavefront: per leg the 12 frames that take the most iterations
    (19 .. 44 for RF, 26 .. 77 for LF), 12 starts that are already the answer (0 iterations), 4 bad-input lanes, 4 ordinary ones."""
    ang, pose, segs, bounds = [], [], [], []
    for leg, fr, a, p, seg, b in shipped_frames():
        out, _, info = rh.run(a, p, seg, b)
        slow = np.argsort(iterations(info))[-12:]
        done = np.where(reason(info) == 0)[0][:12]
        rest = np.setdiff1d(np.arange(len(a)), np.concatenate([slow, done]))[:8]
        aa, pp = np.concatenate([a[slow], out[done], a[rest]]), np.concatenate([p[slow], p[done], p[rest]])
        aa[24, 1], aa[25, 6], pp[26, 0, 2], pp[27, 2, 0] = np.nan, 2e9, np.inf, np.nan
        order = np.random.default_rng(len(ang)).permutation(32)
        ang.append(aa[order])
        pose.append(pp[order])
        segs.append(seg)
        bounds.append(b)
    return np.stack(ang)[None], np.stack(pose)[None], np.array(segs), np.array(bounds)


@pytest.mark.gpu
def test_gpu_one_wavefront_with_short_long_bad_and_capped_lanes(lib, refine_harness):  # noqa: F811
    ang, pose, segs, bounds = mixed_wavefront(refine_harness)
    assert ang.shape == (1, 2, 32, 7)
    ref = host_batch(refine_harness, ang, pose, segs, bounds)
    its, bad = iterations(ref[2]), ref[2] == BAD_INPUT
    assert bad.sum() == 8 and (its[~bad] == 0).sum() >= 24 and (its >= 19).sum() >= 24 and (its >= 35).sum() >= 6 and its.max() >= 70
    assert_equals_host(device_run(lib, ang, pose, None, segs, bounds), ref, "mixed")
    ref3 = host_batch(refine_harness, ang, pose, segs, bounds, max_iter=3)
    capped = reason(ref3[2]) == 4
    assert capped.sum() >= 24 and (iterations(ref3[2])[capped] == 3).all() and (iterations(ref3[2])[~bad & ~capped] == 0).sum() >= 24
    assert_equals_host(device_run(lib, ang, pose, None, segs, bounds, max_iter=3), ref3, "mixed, max_iter=3")
    assert_equals_host(device_run(lib, ang, pose, None, segs, bounds, in_place=True, max_iter=3), ref3, "mixed, in place")


@pytest.mark.gpu
def test_gpu_host_entry_point_and_the_device_entry_point_on_a_torch_stream(lib, refine_harness):  # noqa: F811
    import torch
    S, L, N = 2, 3, 65
    ang, pose, weight, segs, bounds, ref_w, ref_1 = case(refine_harness, S, L, N, 303)
    params = _params_of(lib, segs, bounds)
    host = lib.refine_legs(ang, pose, params, kp_weight=weight)
    assert same_bits(host["angles"], ref_w[0]) and same_bits(host["cost"], ref_w[1])
    assert host["info"].dtype == np.int32 and np.array_equal(host["info"], ref_w[2])
    plain = lib.refine_legs(ang, pose, params, want_cost=False, want_info=False)
    assert plain["cost"] is None and plain["info"] is None and same_bits(plain["angles"], ref_1[0])
    capped = lib.refine_legs(ang, pose, params, kp_weight=weight, max_iter=3, gtol=1e-6, ftol=1e-9)
    ref_c = host_batch(refine_harness, ang, pose, segs, bounds, weight, max_iter=3, gtol=1e-6, ftol=1e-9)
    assert same_bits(capped["angles"], ref_c[0]) and np.array_equal(capped["info"], ref_c[2])
    d_ang, d_pose, d_w = (torch.from_numpy(x).cuda() for x in (ang, pose, weight))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_out = torch.full((S, L, N, 7), 7.0, dtype=torch.float64, device="cuda")
        d_cost = torch.full((S, L, N, 2), 7.0, dtype=torch.float64, device="cuda")
        d_info = torch.full((S, L, N), 7, dtype=torch.int32, device="cuda")
        lib.refine_legs_device(d_ang, d_pose, S, L, N, params, d_out, d_kp_weight=d_w, d_cost=d_cost, d_info=d_info, stream=s)
    s.synchronize()     # that stream alone
    assert same_bits(d_out.cpu().numpy(), ref_w[0]) and same_bits(d_cost.cpu().numpy(), ref_w[1])
    assert np.array_equal(d_info.cpu().numpy(), ref_w[2])
    with pytest.raises(ValueError, match="expected a int32 tensor"):
        lib.refine_legs_device(d_ang, d_pose, S, L, N, params, d_out, d_info=d_cost)
    # empty input: no launch, the output is not touched
    keep = d_out.clone()
    lib.refine_legs_device(d_ang.data_ptr(), d_pose.data_ptr(), 0, L, N, params, d_out.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(keep.view(torch.int64), d_out.view(torch.int64))


@pytest.mark.gpu
def test_gpu_run_refine_chained_on_run_ik_and_fk(lib, refine_harness):  # noqa: F811
    from seqikpy_amd.data import BOUNDS, INITIAL_ANGLES, SEGMENTS
    from seqikpy_amd.kinematic_chain import KinematicChainSeq
    from seqikpy_amd.leg_inverse_kinematics import LegInvKinSeq
    z = load_golden("df3d_100")
    legs = ["RF", "LF"]
    ik = LegInvKinSeq({f"{l}_leg": z[f"{l}_pose"] for l in legs}, KinematicChainSeq(BOUNDS, legs), INITIAL_ANGLES,
                      log_level="ERROR")
    ja, fk_seq = ik.run_ik_and_fk()
    ja = {k: v.copy() for k, v in ja.items()}
    angles, fk = ik.run_refine()
    assert list(angles) == list(ja) and list(fk) == list(fk_seq)
    assert all(fk[k].shape == fk_seq[k].shape for k in fk) and all(same_bits(ik.joint_angles_dict[k], ja[k]) for k in ja)
    before, after = ik.fit_error(ja), ik.fit_error(angles)
    for l in legs:
        seg = [ik.kinematic_chain_class.body_size[f"{l}_{s}"] for s in SEGMENTS]
        bounds = np.array([ik.kinematic_chain_class.bounds_dof[f"{l}_{d}"] for d in DOFS])
        start = np.stack([ja[f"Angle_{l}_{d}"] for d in DOFS], 1)
        ref, ref_cost, ref_info = refine_harness.run(start, z[f"{l}_pose"][:, :5], seg, bounds)
        assert same_bits(np.stack([angles[f"Angle_{l}_{d}"] for d in DOFS], 1), ref)
        assert same_bits(ik.refine_report[l]["cost"], ref_cost) and np.array_equal(ik.refine_report[l]["info"], ref_info)
        assert (after[f"{l}_leg"] ** 2).sum() <= (before[f"{l}_leg"] ** 2).sum()
        assert (after[f"{l}_leg"] ** 2).sum() < 0.9 * (before[f"{l}_leg"] ** 2).sum()
        assert same_bits(ik.run_fk(angles)[f"{l}_leg"], fk[f"{l}_leg"])
