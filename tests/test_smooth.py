"""Trajectory refinement: the whole-leg fit with smoothness across frames (include/seqik_smooth.h, csrc/seqik_smooth.hpp /
seqik_smooth.hip).

CPU tier: the header, the signature table and the exports; every SEQIK_ERR_BAD_ARG case through the C ABI without a GPU;
the linear solve alone against numpy's dense solve; the properties the rule has by construction on 40 made-up trajectories
and on the shipped recording, run on the host (tests/harness/smooth_harness.hip); bad frames; the Python surface --
``_lib.smooth_legs``, ``LegInvKinSeq.run_smooth`` -- with the library call answered by the host-run rule.  GPU tier
(``-m gpu``): every output of the kernels against the host-run rule bit for bit, with guard records around every buffer
and the workspace, over frame counts whose strides cross wavefront and workgroup seams, with the default plan and with one
workgroup of 64 lanes; both entry points; 600 frames of the shipped recording; the decision batch -- rejected trials,
reasons 0, 1, 2 and 4, trajectories stopping in different rounds, asserted on the host-run rule first -- run to its natural
end; a converged batch fed back; 1025 and 2049 frames (eleven and twelve strides); 2 x 3 x 513 frames on one wavefront.

Against scipy on the stacked problem: tests/test_smooth_accuracy.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from angle_map_support import gpu_lib, same_bits, switches
from conftest import DOFS, ROOT, load_golden, random_leg_case
from refine_support import SEED_OF_DOF
from smooth_support import (BAD_INPUT, EPS, FTOL, GTOL, MAX_ITER, SMOOTH, block_rows, dense_system, harness_call,  # noqa: F401
                            largest_change, made_up_trajectories, numpy_bad, numpy_parts, numpy_pcr, record, shipped_window,
                            smooth_harness, stiffness)
from test_capi_symbols import assert_same_class, header_prototypes

SMOOTH_SYMBOLS = ["seqik_smooth_legs", "seqik_smooth_legs_device", "seqik_smooth_workspace_bytes"]


def equal_runs(a, b):
    return (same_bits(a["angles"], b["angles"]) and np.array_equal(a["frame_info"], b["frame_info"])
            and same_bits(a["cost"], b["cost"]) and np.array_equal(a["info"], b["info"]))


# ---------------------------------------------------------------------------------------------------------------------
# CPU tier
# ---------------------------------------------------------------------------------------------------------------------

def test_smooth_header_declares_exactly_the_new_entry_points(hiplib):
    raw = open(os.path.join(ROOT, "include", "seqik_smooth.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(seqik_[a-z_]+)\s*\(", text)))
    assert declared == sorted(SMOOTH_SYMBOLS)
    assert sorted(hiplib.SMOOTH_SIGNATURES) == ["seqik_smooth.h"]
    assert hiplib.SMOOTH_EXPORTED_SYMBOLS == [s[0] for s in hiplib.SMOOTH_SIGNATURES["seqik_smooth.h"]]
    assert sorted(hiplib.SMOOTH_EXPORTED_SYMBOLS) == declared
    tables = (hiplib.SIGNATURES, hiplib.EXTENSION_SIGNATURES, hiplib.STREAM_GAPS_SIGNATURES, hiplib.JACOBIAN_SIGNATURES,
              hiplib.SENSITIVITY_SIGNATURES, hiplib.REFINE_SIGNATURES)
    assert not set(declared) & {s[0] for table in tables for sigs in table.values() for s in sigs}
    for table in tables:
        assert "seqik_smooth.h" not in table
    lib = hiplib.load()
    assert lib.seqik_abi_version() == 7 == hiplib.ABI_VERSION
    assert "seqik_smooth.hip" in hiplib.COMPILE_UNITS and "seqik_smooth.hpp" in hiplib.CSRC_HEADERS
    assert "seqik_smooth" not in " ".join(hiplib.KERNEL_SOURCES + hiplib.LATENCY_SOURCES)
    assert '"seqik_smooth.h"' in open(os.path.join(ROOT, "setup.py")).read()
    assert "#define SEQIK_SMOOTH_DEFAULT 0.1\n" in raw and hiplib.SMOOTH_DEFAULT == 0.1 == SMOOTH
    assert "#define SEQIK_SMOOTH_MAX_ITER 300\n" in raw and hiplib.SMOOTH_MAX_ITER == 300 == MAX_ITER
    assert (hiplib.REFINE_GTOL, hiplib.REFINE_FTOL) == (GTOL, FTOL)
    # the header says what is unlike the other units
    flat = " ".join(raw.split())
    assert "SYNCHRONISES THE STREAM" in flat and "NOT seqik_refine_legs" in flat
    # the options struct: double[7], int32, double, double with C's padding
    opt = hiplib.SeqikSmoothOptions
    assert ctypes.sizeof(opt) == 80 and (opt.max_iter.offset, opt.gtol.offset, opt.ftol.offset) == (56, 64, 72)
    protos = header_prototypes("seqik_smooth.h")
    table = {sig[0]: sig[1:] for sig in hiplib.SMOOTH_SIGNATURES["seqik_smooth.h"]}
    assert sorted(table) == sorted(protos) == declared
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name][0], list(table[name][1:])
        assert len(argtypes) == len(params) == {"seqik_smooth_workspace_bytes": 3, "seqik_smooth_legs": 14,
                                                "seqik_smooth_legs_device": 16}[name], (name, params)
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
    out, fin, cst, inf = np.zeros((1, 2, 3, 7)), np.zeros((1, 2, 3), np.int32), np.zeros((1, 2, 2)), np.zeros((1, 2, 3), np.int32)
    a, p, w, o, c = (x.ctypes.data_as(dp) for x in (ang, pose, wgt, out, cst))
    fi, f = fin.ctypes.data_as(ip), inf.ctypes.data_as(ip)
    good = (hiplib.SeqikLegParams * 2)()
    for l in range(2):
        for i in range(4):
            good[l].seg[i] = 0.5
    bad_seg = (hiplib.SeqikLegParams * 2)()
    bad_seg[1].seg[2] = np.inf
    need = lib.seqik_smooth_workspace_bytes(1, 2, 3)
    assert 0 < need <= 6 * 3940 + 2 * 48 + 3072
    ws = ctypes.create_string_buffer(need + 8)
    ws_ptr = ctypes.c_void_p(ctypes.addressof(ws) + (8 - ctypes.addressof(ws) % 8) % 8)
    huge = 2 ** 63 // (8 * 500) + 1

    def opt(smooth=0.1, max_iter=10, gtol=1e-10, ftol=1e-14):
        return ctypes.byref(hiplib.SeqikSmoothOptions((ctypes.c_double * 7)(*np.broadcast_to(smooth, (7,))), max_iter, gtol, ftol))

    one_bad = lambda v: [0.1, 0.1, 0.1, v, 0.1, 0.1, 0.1]  # noqa: E731
    #        angles pose n_seq n_legs n_frames legs kind kp_weight opt angles_out frame_info cost info
    cases = [("n_legs", (a, p, 1, 0, 3, good, 0, None, None, o, fi, c, f)), ("n_legs", (a, p, 1, 9, 3, good, 0, w, None, o, None, None, None)),
             ("negative", (a, p, -1, 2, 3, good, 0, None, None, o, fi, c, f)), ("negative", (a, p, 1, 2, -3, good, 0, None, None, o, fi, c, f)),
             ("angles must", (None, p, 1, 2, 3, good, 0, None, None, o, fi, c, f)), ("pose must", (a, None, 1, 2, 3, good, 0, None, None, o, fi, c, f)),
             ("angles_out must", (a, p, 1, 2, 3, good, 0, None, None, None, fi, c, f)), ("legs", (a, p, 1, 2, 3, None, 0, None, None, o, fi, c, f)),
             ("not built", (a, p, 1, 2, 3, good, 1, None, None, o, fi, c, f)), ("kind", (a, p, 1, 2, 3, good, 2, None, None, o, fi, c, f)),
             ("kind", (a, p, 1, 2, 3, good, -1, None, None, o, fi, c, f)), ("segment", (a, p, 1, 2, 3, bad_seg, 0, None, None, o, fi, c, f)),
             ("max_iter", (a, p, 1, 2, 3, good, 0, None, opt(max_iter=0), o, fi, c, f)),
             ("max_iter", (a, p, 1, 2, 3, good, 0, None, opt(max_iter=1001), o, fi, c, f)),
             ("max_iter", (a, p, 1, 2, 3, good, 0, None, opt(max_iter=-1), o, fi, c, f)),
             ("smooth", (a, p, 1, 2, 3, good, 0, None, opt(smooth=one_bad(-1e-3)), o, fi, c, f)),
             ("smooth", (a, p, 1, 2, 3, good, 0, None, opt(smooth=one_bad(np.nan)), o, fi, c, f)),
             ("smooth", (a, p, 1, 2, 3, good, 0, None, opt(smooth=one_bad(np.inf)), o, fi, c, f)),
             ("gtol", (a, p, 1, 2, 3, good, 0, None, opt(gtol=-1e-10), o, fi, c, f)), ("gtol", (a, p, 1, 2, 3, good, 0, None, opt(gtol=np.nan), o, fi, c, f)),
             ("gtol", (a, p, 1, 2, 3, good, 0, None, opt(gtol=np.inf), o, fi, c, f)),
             ("ftol", (a, p, 1, 2, 3, good, 0, None, opt(ftol=-1e-14), o, fi, c, f)), ("ftol", (a, p, 1, 2, 3, good, 0, None, opt(ftol=np.nan), o, fi, c, f)),
             ("ftol", (a, p, 1, 2, 3, good, 0, None, opt(ftol=np.inf), o, fi, c, f)),
             ("too many", (a, p, huge, 1, 1, good, 0, None, None, o, fi, c, f)), ("too many", (a, p, 1, 1, huge, good, 0, None, None, o, None, None, None)),
             ("too many", (a, p, 2 ** 40, 2, 2 ** 40, good, 0, None, None, o, fi, c, f))]
    for what, args in cases:
        for fn, last in ((lib.seqik_smooth_legs, (-1,)), (lib.seqik_smooth_legs_device, (ws_ptr, need, None))):
            assert fn(*args, *last) == hiplib.ERR_ARG, (what, fn.__name__)
            msg = lib.seqik_last_error().decode()
            assert msg.startswith("seqik_smooth_legs: ") and what in msg, (what, msg)
    ok = (a, p, 1, 2, 3, good, 0, None, None, o, fi, c, f)
    for last in ((None, need, None), (ws_ptr, need - 1, None), (ws_ptr, 0, None), (ws_ptr, -1, None),
                 (ctypes.c_void_p(ws_ptr.value + 4), need, None)):
        assert lib.seqik_smooth_legs_device(*ok, *last) == hiplib.ERR_ARG
        assert "workspace" in lib.seqik_last_error().decode()
    # the workspace: sizes that are not valid, nothing to do, and the bound the documents give
    assert lib.seqik_smooth_workspace_bytes(1, 0, 3) == -1 and "n_legs" in lib.seqik_last_error().decode()
    assert lib.seqik_smooth_workspace_bytes(-1, 2, 3) == -1 and lib.seqik_smooth_workspace_bytes(huge, 1, 1) == -1
    assert lib.seqik_smooth_workspace_bytes(0, 2, 3) == 0 == lib.seqik_smooth_workspace_bytes(4, 2, 0)
    for S, L, N in ((1, 1, 1), (3, 2, 5), (2, 6, 1000), (64, 2, 1000), (1, 2, 6000), (1, 1, 2 ** 20 + 1)):
        assert 0 < lib.seqik_smooth_workspace_bytes(S, L, N) <= S * L * (N * 3940 + 48) + 3072
    # no leg-frames: OK, nothing is touched, a workspace is not asked for
    for args in ((a, p, 0, 2, 3, good, 0, None, None, o, fi, c, f), (a, p, 1, 2, 0, good, 0, w, opt(max_iter=1, gtol=0.0, ftol=0.0), o, fi, c, f)):
        assert lib.seqik_smooth_legs(*args, -1) == 0 and lib.seqik_smooth_legs_device(*args, None, 0, None) == 0
    assert not out.any() and not cst.any() and not inf.any() and not fin.any()
    # the Python wrappers: shapes and arguments
    params = [hiplib.leg_params_from_arrays(np.full(4, 0.5), np.zeros((7, 2)), np.zeros(27))] * 2
    with pytest.raises(ValueError, match="pose must have shape"):
        hiplib.smooth_legs(ang, pose[..., :4, :], params)
    with pytest.raises(ValueError, match="kp_weight must broadcast"):
        hiplib.smooth_legs(ang, pose, params, kp_weight=np.ones(3))
    with pytest.raises(ValueError, match="smooth must be a scalar or"):
        hiplib.smooth_legs(ang, pose, params, smooth=np.ones(4))
    with pytest.raises(ValueError, match="max_iter must lie in 1..1000"):
        hiplib.smooth_legs(ang, pose, params, max_iter=0)
    with pytest.raises(ValueError, match="n_legs"):
        hiplib.smooth_workspace_bytes(1, 9, 3)
    assert hiplib.smooth_workspace_bytes(1, 2, 3) == need


SOLVE_SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 65)


def test_linear_solve_against_the_dense_solve(smooth_harness):  # noqa: F811
    """The parallel cyclic reduction alone, on block rows made from real normal equations with held masks, broken pairs
    and identity rows, against numpy.linalg.solve of the assembled dense matrix.  The bar: 100 times the forward error
    of the float64 numpy restatement of the same reduction against that dense solve, relative to max |x| (and never
    below 100 eps: at N = 1 the restatement IS a direct solve and its error can be 0).  Measured (profiles/
    smooth_vs_scipy.json, "linear_solve"): restatement <= 5.7e-14, harness <= 4.9e-14, harness against restatement
    <= 4.7e-14."""
    worst = dict(restatement=0.0, harness=0.0, harness_vs_restatement=0.0)
    n_held = n_identity = n_broken = 0
    for N in SOLVE_SIZES:
        for seed in range(3):
            D, L, U, b = block_rows(N, 100 * N + seed)
            M, rhs = dense_system(D, L, U, b)
            assert np.array_equal(M, M.T)
            x = np.linalg.solve(M, rhs).reshape(N, 7)
            scale = np.abs(x).max()
            ref = numpy_pcr(D, L, U, b)
            got, rejected = smooth_harness.solve(D, L, U, b)
            assert not rejected
            err_ref, err, diff = (np.abs(v).max() / scale for v in (ref - x, got - x, got - ref))
            print(f"N={N} seed={seed} cond={np.linalg.cond(M):.3g} restatement {err_ref:.3g} harness {err:.3g} apart {diff:.3g}")
            bar = 100 * max(err_ref, EPS)
            assert err <= bar and diff <= bar, (N, seed, err_ref, err, diff)
            identity = np.array([np.array_equal(d, np.eye(7)) for d in D])
            assert (got[identity] == 0).all()                                   # a bad frame does not move
            held = (np.stack([np.diag(d) for d in D]) == 1.0) & (b == 0) & ~identity[:, None]
            assert (got[held] == 0).all()                                       # nor does a held DOF
            n_held, n_identity = n_held + held.sum(), n_identity + identity.sum()
            n_broken += sum(1 for t in range(1, N) if not identity[t] and not identity[t - 1] and not L[t].any())
            for k, v in (("restatement", err_ref), ("harness", err), ("harness_vs_restatement", diff)):
                worst[k] = max(worst[k], float(v))
    assert n_held > 100 and n_identity > 20 and n_broken > 10
    record("linear_solve", worst)
    # the upper triangle of D is never read
    D, L, U, b = block_rows(9, 5)
    junk = D + np.triu(np.full((7, 7), np.nan), 1)
    assert same_bits(smooth_harness.solve(junk, L, U, b)[0], smooth_harness.solve(D, L, U, b)[0])
    # a pivot that is not positive, in the first row, in the last, and one that appears only after a reduction
    for N, t in ((1, 0), (9, 0), (9, 8), (33, 17)):
        D, L, U, b = block_rows(N, 7 + N, lam=1e-3)
        D[t][3, 3] = -1.0
        assert smooth_harness.solve(D, L, U, b)[1], (N, t)
    D, L, U, b = block_rows(8, 3)
    good = ~np.array([np.array_equal(d, np.eye(7)) for d in D])
    t = next(t for t in range(1, 8) if L[t].any())
    L[t], U[t - 1] = 50.0 * L[t], 50.0 * U[t - 1]                  # D_t - L_t D_{t-1}^-1 U_{t-1} is no longer positive
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(dense_system(D, L, U, b)[0])
    for d in D[good]:
        np.linalg.cholesky(np.tril(d) + np.tril(d, -1).T)          # (every block by itself still is)
    assert smooth_harness.solve(D, L, U, b)[1]


def check_properties(res, ang, pose, seg, bounds, smooth, weight=None, max_iter=MAX_ITER):
    """What the rule promises by construction, for one trajectory."""
    lb, ub = bounds[:, 0], bounds[:, 1]
    bad = numpy_bad(ang, pose, weight)
    out, finfo, cost, (why, steps, rejected) = res["angles"], res["frame_info"], res["cost"], res["info"]
    assert np.array_equal(finfo == BAD_INPUT, bad) and np.isnan(out[bad]).all() and np.isfinite(out[~bad]).all()
    assert not (finfo[~bad] & ~0x7F).any()
    assert np.isfinite(cost).all() and cost[1] <= cost[0]
    assert (out[~bad] >= lb).all() and (out[~bad] <= ub).all()
    assert why in (0, 1, 2, 4) and 0 <= steps <= max_iter and rejected >= 0 and (why != 4 or steps == max_iter)
    assert steps > 0 or cost[1] == cost[0]
    # the cost at the start and at the result, recomputed
    q0 = np.clip(np.where(bad[:, None], 0.0, ang), lb, ub)
    C0 = numpy_parts(q0, pose, seg, bounds, smooth, weight, bad)[0]
    C1, g, held = numpy_parts(np.where(bad[:, None], 0.0, out), pose, seg, bounds, smooth, weight, bad)
    assert abs(C0 - cost[0]) <= 1e-12 * C0 and abs(C1 - cost[1]) <= 1e-12 * C1, (C0, C1, cost)
    # the held bits: the rule on the full gradient at the result (a gradient entry within rounding of 0 may fall either way)
    got = (finfo[:, None] >> np.arange(7)) & 1 == 1
    got[bad] = False
    sure = np.abs(g) > 1e-9 * max(1.0, np.abs(g).max())
    assert np.array_equal(got[sure], held[sure])
    assert ((out == lb) | (out == ub))[got].all()
    return why, steps, got.sum()


def test_properties_on_the_made_up_trajectories(smooth_harness):  # noqa: F811
    """40 made-up legs of 24 frames as 40 trajectories, started from their seeds."""
    reasons, n_held, n_steps, n_gradient = np.zeros(8, dtype=int), 0, 0, 0
    trajs = made_up_trajectories()
    for i, (ang, pose, seg, bounds) in enumerate(trajs):
        smooth = (SMOOTH, 1.0, np.array([0.0, 0.3, 0.1, 0.1, 0.02, 0.1, 1.0]), 0.0)[i % 4]
        res = smooth_harness.run_one(ang, pose, seg, bounds, smooth=smooth)
        why, steps, held = check_properties(res, ang, pose, seg, bounds, smooth)
        reasons[why] += 1
        n_held, n_steps = n_held + held, n_steps + steps
        # in place equals out of place
        assert equal_runs(smooth_harness.run_one(ang, pose, seg, bounds, smooth=smooth, in_place=True), res)
        # a cap: a prefix of the uncapped run
        capped = smooth_harness.run_one(ang, pose, seg, bounds, smooth=smooth, max_iter=3)
        check_properties(capped, ang, pose, seg, bounds, smooth, max_iter=3)
        assert capped["cost"][1] >= res["cost"][1] and (capped["info"][0] == 4) == (steps > 3 or (steps == 3 and why == 4))
        # a result that met the gradient test is a start that meets it: its clamped bits, no step.  (These targets are
        # nasty and the default gradient bar is rarely met before the cost stalls; a bar of 1e-5 is met.)
        loose = smooth_harness.run_one(ang, pose, seg, bounds, smooth=smooth, gtol=1e-5)
        check_properties(loose, ang, pose, seg, bounds, smooth)
        for first, gtol in ((res, GTOL), (loose, 1e-5)):
            if first["info"][0] == 0:
                n_gradient += 1
                again = smooth_harness.run_one(first["angles"], pose, seg, bounds, smooth=smooth, gtol=gtol)
                assert same_bits(again["angles"], first["angles"]) and tuple(again["info"]) == (0, 0, 0)
                assert same_bits(again["cost"], first["cost"][[1, 1]]) and np.array_equal(again["frame_info"], first["frame_info"])
        # N = 1 and N = 2
        for n in (1, 2):
            short = smooth_harness.run_one(ang[:n], pose[:n], seg, bounds, smooth=smooth)
            check_properties(short, ang[:n], pose[:n], seg, bounds, smooth)
    assert reasons[1] >= 5 and reasons[4] >= 5 and n_gradient >= 5 and n_held > 200 and n_steps > 400, (reasons, n_gradient, n_held)
    # trajectories solved together equal each solved alone: 2 sequences x 3 legs of different segments and limits
    segs, bounds = [t[2] for t in trajs[:3]], [t[3] for t in trajs[:3]]
    ang = np.stack([np.stack([trajs[l + 3 * s][0] for l in range(3)]) for s in range(2)])
    pose = np.stack([np.stack([trajs[l + 3 * s][1] for l in range(3)]) for s in range(2)])
    both = smooth_harness.run(ang, pose, segs, bounds)
    for s in range(2):
        for l in range(3):
            alone = smooth_harness.run_one(ang[s, l], pose[s, l], segs[l], bounds[l])
            assert equal_runs({k: both[k][s, l] for k in alone if k != "rounds"}, alone), (s, l)
    assert both["rounds"] >= max(both["info"][..., 1:].sum(-1).max(), 1)


def test_properties_on_the_shipped_recording(smooth_harness):  # noqa: F811
    """RF and LF 0:64 of the shipped recording from the sequential fit, alone and together."""
    legs = [shipped_window(leg, 0, 64) for leg in ("RF", "LF")]
    alone = []
    for ang, pose, seg, bounds in legs:
        res = smooth_harness.run_one(ang, pose, seg, bounds)
        why, steps, _ = check_properties(res, ang, pose, seg, bounds, SMOOTH)
        assert why in (0, 1) and steps > 0 and res["cost"][1] < res["cost"][0]
        assert largest_change(res["angles"]) <= largest_change(np.clip(ang, bounds[:, 0], bounds[:, 1]))
        assert equal_runs(smooth_harness.run_one(ang, pose, seg, bounds, in_place=True), res)
        alone.append(res)
    both = smooth_harness.run(np.stack([l[0] for l in legs])[None], np.stack([l[1] for l in legs])[None], [l[2] for l in legs],
                              [l[3] for l in legs])
    for l in range(2):
        assert equal_runs({k: both[k][0, l] for k in alone[l] if k != "rounds"}, alone[l])


def test_bad_frames_take_no_part_and_cut_the_coupling(smooth_harness):  # noqa: F811
    ang, pose, seg, bounds = shipped_window("RF", 0, 24)
    wgt = np.ones((24, 4))
    ref = smooth_harness.run_one(ang, pose, seg, bounds, weight=wgt)
    assert equal_runs(ref, smooth_harness.run_one(ang, pose, seg, bounds))              # weights of 1 are no weights
    # every kind of rule 1 of seqik_refine.h, each on a frame of its own
    kinds = {"nan angle": ("a", (2, 3), np.nan), "inf angle": ("a", (4, 0), -np.inf), "angle beyond 2^30": ("a", (6, 6), 1.1e9),
             "nan weight": ("w", (8, 1), np.nan), "inf weight": ("w", (10, 0), np.inf), "negative weight": ("w", (12, 3), -1.0),
             "nan origin": ("p", (14, 0, 1), np.nan), "inf key point": ("p", (16, 3, 2), np.inf),
             "nan key point": ("p", (18, 4, 0), np.nan)}
    for name, (which, idx, value) in kinds.items():
        a, p, w = ang.copy(), pose.copy(), wgt.copy()
        dict(a=a, p=p, w=w)[which][idx] = value
        res = smooth_harness.run_one(a, p, seg, bounds, weight=w, max_iter=5)
        bad = np.arange(24) == idx[0]
        assert np.array_equal(numpy_bad(a, p, w), bad), name
        check_properties(res, a, p, seg, bounds, SMOOTH, w, max_iter=5)
        assert res["frame_info"][idx[0]] == BAD_INPUT and np.isnan(res["angles"][idx[0]]).all(), name
    # a NaN frame in the middle: the two halves as trajectories of their own.  One lambda and one decision serve the whole
    # trajectory, so the bits are those of the halves as long as all three runs take the same decisions -- here, on the
    # window RF 272:296 where the start jumps by 2.6 rad, six accepted steps without a rejection, which the cap makes the
    # whole of every run; the linear solve, the trial points and every e_t of a half do not depend on what lies behind
    # the cut.  The costs add in another tree order.
    jump_ang, jump_pose = shipped_window("RF", 272, 296)[:2]
    for m in range(1, 23):
        a = jump_ang.copy()
        a[m, 2] = np.nan
        whole = smooth_harness.run_one(a, jump_pose, seg, bounds, max_iter=6)
        first, second = (smooth_harness.run_one(a[s], jump_pose[s], seg, bounds, max_iter=6) for s in (slice(0, m), slice(m + 1, 24)))
        for r in (whole, first, second):
            assert tuple(r["info"]) == (4, 6, 0)
        assert same_bits(whole["angles"][:m], first["angles"]) and same_bits(whole["angles"][m + 1:], second["angles"])
        assert np.array_equal(whole["frame_info"], np.concatenate([first["frame_info"], [BAD_INPUT], second["frame_info"]]))
        assert np.allclose(whole["cost"], first["cost"] + second["cost"], rtol=1e-14, atol=0)
        assert np.isnan(whole["angles"][m]).all()
    # ... and run to the end the coupling is still cut: the result's cost is that of the halves' results
    a = ang.copy()
    a[11, 2] = np.nan
    whole = smooth_harness.run_one(a, pose, seg, bounds)
    first, second = (smooth_harness.run_one(a[s], pose[s], seg, bounds) for s in (slice(0, 11), slice(12, 24)))
    assert all(r["info"][0] in (0, 1) for r in (whole, first, second))
    assert np.isclose(whole["cost"][1], first["cost"][1] + second["cost"][1], rtol=1e-9, atol=0)
    # no good frame at all: reason 0, no step, cost 0
    none = smooth_harness.run_one(np.full((5, 7), np.nan), pose[:5], seg, bounds)
    assert tuple(none["info"]) == (0, 0, 0) and not none["cost"].any() and (none["frame_info"] == BAD_INPUT).all()
    assert np.isnan(none["angles"]).all() and none["rounds"] == 0
    # weight exactly 0: the key point is not read -- NaN there gives the bits of a finite value there
    w0 = wgt.copy()
    w0[5, 2], w0[7, 3], w0[9, :] = 0.0, 0.0, 0.0
    p_nan, p_fin = pose.copy(), pose.copy()
    p_nan[5, 3], p_nan[7, 4, 1], p_nan[9, 1:] = np.nan, np.inf, np.nan
    p_fin[5, 3], p_fin[7, 4, 1], p_fin[9, 1:] = 123.0, -4.0, 0.5
    got, want = smooth_harness.run_one(ang, p_nan, seg, bounds, weight=w0), smooth_harness.run_one(ang, p_fin, seg, bounds, weight=w0)
    assert equal_runs(got, want) and not (got["frame_info"] & BAD_INPUT).any()
    check_properties(got, ang, p_nan, seg, bounds, SMOOTH, w0)
    assert not same_bits(got["angles"][5], ref["angles"][5])                            # and the weight does count


def test_python_surface_on_the_df3d_fixture(hiplib, smooth_harness, monkeypatch):  # noqa: F811
    from seqikpy_amd.data import BOUNDS, INITIAL_ANGLES, SEGMENTS
    from seqikpy_amd.kinematic_chain import KinematicChainGeneric, KinematicChainSeq
    from seqikpy_amd.leg_inverse_kinematics import LegInvKinGeneric, LegInvKinSeq
    monkeypatch.setattr(hiplib, "_call", harness_call(smooth_harness, hiplib._call))
    z = load_golden("df3d_100")
    legs, N = ["RF", "LF"], 100
    ik = LegInvKinSeq({f"{l}_leg": z[f"{l}_pose"] for l in legs}, KinematicChainSeq(BOUNDS, legs), INITIAL_ANGLES,
                      log_level="ERROR")
    assert ik.smooth_report == {}
    ja = {f"Angle_{l}_{d}": z[f"{l}_angles"][:, i].copy() for l in legs for i, d in enumerate(DOFS)}
    ik.joint_angles_dict = {k: v.copy() for k, v in ja.items()}
    stored = ik.joint_angles_dict
    angles = ik.run_smooth(max_iter=40)
    assert list(angles) == list(ja) and all(v.shape == (N,) for v in angles.values())
    assert ik.joint_angles_dict is stored and all(same_bits(stored[k], ja[k]) for k in ja)      # the stored angles are untouched
    assert list(ik.smooth_report) == legs
    for l in legs:
        rep = ik.smooth_report[l]
        seg = [ik.kinematic_chain_class.body_size[f"{l}_{s}"] for s in SEGMENTS]
        bounds = np.array([ik.kinematic_chain_class.bounds_dof[f"{l}_{d}"] for d in DOFS])
        ref = smooth_harness.run_one(z[f"{l}_angles"], z[f"{l}_pose"][:, :5], seg, bounds, max_iter=40)
        got = np.stack([angles[f"Angle_{l}_{d}"] for d in DOFS], 1)
        assert same_bits(got, ref["angles"]) and same_bits(rep["cost"], ref["cost"])
        assert (rep["reason"], rep["steps"], rep["rejected"]) == tuple(ref["info"]) and rep["steps"] > 0
        assert np.array_equal(rep["frame_info"], ref["frame_info"]) and rep["frame_info"].dtype == np.int32
        assert rep["largest_change"].shape == (2,)
        assert rep["largest_change"][0] == largest_change(z[f"{l}_angles"]) and rep["largest_change"][1] == largest_change(got)
        assert rep["cost"][1] < rep["cost"][0]
    # explicit angles equal the stored default; smooth as a scalar or (7,); weights as run_refine takes them
    assert all(same_bits(v, angles[k]) for k, v in ik.run_smooth(ja, max_iter=40).items())
    s7, w4 = np.array([0.0, 0.3, 0.1, 0.1, 0.02, 0.1, 1.0]), np.array([1.0, 2.0, 0.5, 3.0])
    got = ik.run_smooth(smooth=s7, key_point_weight={"RF": w4, "LF": 2.0}, max_iter=10, gtol=1e-8, ftol=1e-12)
    for l, w in (("RF", w4), ("LF", 2.0)):
        seg = [ik.kinematic_chain_class.body_size[f"{l}_{s}"] for s in SEGMENTS]
        bounds = np.array([ik.kinematic_chain_class.bounds_dof[f"{l}_{d}"] for d in DOFS])
        ref = smooth_harness.run_one(z[f"{l}_angles"], z[f"{l}_pose"][:, :5], seg, bounds, smooth=s7, weight=np.broadcast_to(w, (N, 4)),
                                     max_iter=10, gtol=1e-8, ftol=1e-12)
        assert same_bits(np.stack([got[f"Angle_{l}_{d}"] for d in DOFS], 1), ref["angles"])
    with pytest.raises(ValueError, match="key_point_weight must be a scalar"):
        ik.run_smooth(key_point_weight=np.ones((N, 3)))
    with pytest.raises(ValueError, match="unknown smoothing options"):
        ik.run_smooth(xtol=1e-3)
    with pytest.raises(ValueError, match="smooth must be a scalar or"):
        ik.run_smooth(smooth=np.ones(3))
    doc = " ".join(LegInvKinSeq.run_smooth.__doc__.split())
    assert "NOT overwritten" in doc and "LOCAL method" in doc
    # the generic chain is not built
    zg = load_golden("generic_rf_100")
    gen = LegInvKinGeneric({"RF_leg": zg["RF_pose"]}, KinematicChainGeneric(BOUNDS, ["RF"]), INITIAL_ANGLES, log_level="ERROR")
    with pytest.raises(NotImplementedError, match="sequential chain only"):
        gen.run_smooth()


# ---------------------------------------------------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(hiplib):
    return gpu_lib(hiplib)


SENTINEL, SENTINEL_I, GUARD = -12345.678, -1234567, 256


def _params_of(lib, segs, bounds):
    return [lib.leg_params_from_arrays(s, b, np.zeros(27)) for s, b in zip(segs, bounds)]


def made_up_batch(seed, S, L, N):
    """S x L trajectories of N frames of L made-up legs (different segments and limits), started from the legs' seeds,
    with a plane of weights, one bad frame (from 5 frames on, in the middle of a trajectory) and a weightless key point
    that holds NaN -> ang (S, L, N, 7), pose (S, L, N, 5, 3), weight (S, L, N, 4), segs, bounds"""
    rng = np.random.default_rng(seed)
    ang, pose, segs, bounds = np.empty((S, L, N, 7)), np.empty((S, L, N, 5, 3)), [], []
    for l in range(L):
        p, seg, b, seeds = random_leg_case(rng, S * N)
        pose[:, l], ang[:, l] = p.reshape(S, N, 5, 3), seeds[SEED_OF_DOF]
        segs.append(seg)
        bounds.append(b)
    weight = np.ones((S, L, N, 4))
    weight[S - 1, 1] = rng.uniform(0.25, 2.0, (N, 4))
    if N >= 5:
        ang[0, L - 1, N // 2, 4] = np.nan
        weight[S - 1, 1, 1, 3], pose[S - 1, 1, 1, 4] = 0.0, np.nan
    return ang, pose, weight, np.array(segs), np.array(bounds)


WIDE_LIMIT, GLITCH = 1e10, 1e30


def decision_batch(seed, S=3, L=3, N=24):
    """made_up_batch with two changes that open the rule's rarest path: the last leg has no limits to speak of (+-1e10,
    beyond the angle domain of 2^30) and one key point of one frame of its middle trajectory is a tracking glitch at 1e30.
    From there every step leaves the angle domain whatever the damping, so every trial is unusable and the trajectory
    ends on reason 2 after 25 rejections, at a finite cost."""
    ang, pose, weight, segs, bounds = made_up_batch(seed, S, L, N)
    bounds[L - 1] = np.stack([np.full(7, -WIDE_LIMIT), np.full(7, WIDE_LIMIT)], 1)
    pose[S // 2, L - 1, N // 2 - 1, 4, 0] = GLITCH
    return ang, pose, weight, segs, bounds


# the batch whose trajectories take every decision path the rule has between them (found by a search over seeds on the
# host-run rule; tests/test_smooth_accuracy.py::test_decision_paths_are_taken asserts that they do), and its options
DECISION_SEED, DECISION_OPTS = 8, dict(smooth=1.0, gtol=1e-5)

_CASES = {}


def decision_case(sh):
    """The decision batch, the host-run rule's answer with the paths it took (the harness's watched loop) and the answer of
    smooth_run_host itself, computed once."""
    if "decision" not in _CASES:
        ang, pose, weight, segs, bounds = decision_batch(DECISION_SEED)
        watched = sh.run(ang, pose, segs, bounds, weight=weight, paths=True, **DECISION_OPTS)
        ref = sh.run(ang, pose, segs, bounds, weight=weight, **DECISION_OPTS)
        _CASES["decision"] = (ang, pose, weight, segs, bounds, watched, ref)
    return _CASES["decision"]


def assert_decision_paths(watched):
    """The paths the decision batch is there for, on the host-run rule's record of it."""
    info, paths = watched["info"].reshape(-1, 3), watched["paths"].reshape(-1, 3)
    why, steps, rejected = info.T
    assert sorted(set(why.tolist())) == [0, 1, 2, 4]
    # (a) rejected trials -- `lambda * 4`, no copy of qn, the next ASSEMBLE skips the trajectory -- in trajectories that
    # went on to accept steps afterwards
    assert ((rejected > 50) & (steps > 50)).sum() >= 4
    # (b) a pivot that is not positive does not occur in the whole rule (see test_smooth_accuracy.test_decision_paths_are_taken)
    assert not paths[:, 0].any()
    # (c) reason 2: damping exhausted by 25 unusable trials in a row, each lost to an angle outside the domain
    assert np.array_equal(info[why == 2], [[2, 0, 25]]) and np.array_equal(paths[why == 2], [[0, 25, 25]])
    assert not paths[why != 2, 1].any()
    # (d) trajectories of one batch stop in different rounds: reason 0 and reason 1 at least 5 rounds apart, and others
    # go on long after the first has stopped
    assert min(abs(int(a) - int(b)) for a in paths[why == 0, 2] for b in paths[why == 1, 2]) >= 5
    assert len(set(paths[:, 2].tolist())) >= 6 and paths[:, 2].min() == 25 and watched["rounds"] == paths[:, 2].max() > 500
    assert (steps[why == 0] > 50).all()                              # the gradient test was met by work, not at the start
    # (e) reason 4 on the default cap
    assert (why == 4).sum() >= 2 and (steps[why == 4] == MAX_ITER).all()
    assert (paths[:, 2] == steps + rejected).all()                   # a trial per round until it stops


def case(sh, S, L, N, seed, **opts):
    """Inputs and the host-run rule's answers for them, computed once per size."""
    key = (S, L, N, seed, tuple(sorted(opts.items())))
    if key not in _CASES:
        ang, pose, weight, segs, bounds = made_up_batch(seed, S, L, N)
        _CASES[key] = (ang, pose, weight, segs, bounds, sh.run(ang, pose, segs, bounds, weight=weight, **opts))
    return _CASES[key]


def device_run(lib, ang, pose, weight, segs, bounds, in_place=False, env=None, **opts):
    """The device entry point on torch tensors with guard records on each side of every buffer it reads or writes and of
    the workspace, all filled with a sentinel -> the outputs; asserts that the guards and the inputs are untouched."""
    import torch
    S, L, N = ang.shape[:3]
    shapes = dict(angles=((S, L, N, 7), torch.float64), frame_info=((S, L, N), torch.int32), cost=((S, L, 2), torch.float64),
                  info=((S, L, 3), torch.int32))
    need = lib.smooth_workspace_bytes(S, L, N)
    inputs = dict(pose=pose) if weight is None else dict(pose=pose, weight=weight)
    if not in_place:
        inputs["start"] = ang
    bufs, ptr = {}, {}
    for k, a in inputs.items():      # the inputs between guards too: they come back as they went in, guards included
        bufs[k] = torch.full((a.size + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
        bufs[k][GUARD:-GUARD] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
        ptr[k] = bufs[k].data_ptr() + 8 * GUARD
    sent_in = {k: bufs[k].clone() for k in inputs}
    for k, (shape, dtype) in shapes.items():
        n = int(np.prod(shape))
        bufs[k] = torch.full((n + 2 * GUARD,), SENTINEL_I if dtype == torch.int32 else SENTINEL, dtype=dtype, device="cuda")
        ptr[k] = bufs[k].data_ptr() + bufs[k].element_size() * GUARD
    ws = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    if in_place:      # the start sits inside the guarded output buffer
        bufs["angles"][GUARD:-GUARD] = torch.from_numpy(np.ascontiguousarray(ang).reshape(-1)).cuda()
    with switches(**(env or {})):
        lib.smooth_legs_device(ptr["angles" if in_place else "start"], ptr["pose"], S, L, N, _params_of(lib, segs, bounds),
                               ptr["angles"], ws.data_ptr() + GUARD, need, d_kp_weight=ptr.get("weight", 0),
                               d_frame_info=ptr["frame_info"], d_cost=ptr["cost"], d_info=ptr["info"],
                               stream=torch.cuda.current_stream().cuda_stream, **opts)
        torch.cuda.synchronize()
    out = {}
    for k, (shape, dtype) in shapes.items():
        got, sent = bufs[k].cpu().numpy(), SENTINEL_I if dtype == torch.int32 else SENTINEL
        assert (got[:GUARD] == sent).all() and (got[-GUARD:] == sent).all(), (k, "guard", env)
        out[k] = got[GUARD:-GUARD].reshape(shape)
    for k in inputs:
        assert torch.equal(bufs[k].view(torch.int64), sent_in[k].view(torch.int64)), (k, "input changed", env)
    got = ws.cpu().numpy()
    assert (got[:GUARD] == 0xA5).all() and (got[-GUARD:] == 0xA5).all(), ("workspace guard", env)
    return out


def assert_equals_host(got, ref, where):
    assert same_bits(got["angles"], ref["angles"]), where
    assert np.array_equal(got["frame_info"], ref["frame_info"]), where
    assert same_bits(got["cost"], ref["cost"]), where
    assert np.array_equal(got["info"], ref["info"]), where


FRAMES = (1, 2, 5, 33, 64, 65, 130, 300)
ONE_SMALL_WORKGROUP = dict(SEQIK_SMOOTH_GRID="1", SEQIK_SMOOTH_BLOCK="64")


@pytest.mark.gpu
@pytest.mark.parametrize("N", FRAMES)
def test_gpu_kernels_equal_the_host_rule_bit_for_bit(lib, smooth_harness, N):  # noqa: F811
    """2 sequences x 3 legs (three segment sets and limits) x 1 .. 300 frames -- eight lanes per row, so a stride reaches
    across a wavefront from 9 frames and across a 256-lane workgroup from 33 -- with a bad frame, a plane of weights and a
    weightless NaN key point, at most 30 accepted steps; the default plan, and one workgroup of 64 lanes walking
    everything in its grid-stride loop; guards around every buffer and the workspace."""
    ang, pose, weight, segs, bounds, ref = case(smooth_harness, 2, 3, N, 700 + N, max_iter=30)
    assert ref["rounds"] >= 10 and (ref["info"][..., 1] > 0).any()
    assert ((ref["frame_info"] == BAD_INPUT).sum() == 1) == (N >= 5)
    assert_equals_host(device_run(lib, ang, pose, weight, segs, bounds, max_iter=30), ref, (N, "default plan"))
    assert_equals_host(device_run(lib, ang, pose, weight, segs, bounds, max_iter=30, env=ONE_SMALL_WORKGROUP), ref,
                       (N, "one workgroup of 64"))
    if N == 65:
        assert_equals_host(device_run(lib, ang, pose, weight, segs, bounds, max_iter=30, in_place=True), ref, (N, "in place"))


@pytest.mark.gpu
def test_gpu_decision_paths_equal_the_host_rule(lib, smooth_harness):  # noqa: F811
    """The decision batch of tests/test_smooth_accuracy.py::test_decision_paths_are_taken on the kernels, run to its natural end (543 rounds of 16
    launches): rejected trials, damping exhausted, the cap, and trajectories that stop in nine different rounds, so the
    decide kernel's "not accepted" branch and the early return of a stopped trajectory's rows run in every phase.  That
    the paths are taken is asserted on the host-run reference first."""
    ang, pose, weight, segs, bounds, watched, ref = decision_case(smooth_harness)
    assert_decision_paths(watched)
    assert equal_runs(watched, ref)
    assert_equals_host(device_run(lib, ang, pose, weight, segs, bounds, **DECISION_OPTS), ref, "decision batch, default plan")
    assert_equals_host(device_run(lib, ang, pose, weight, segs, bounds, env=ONE_SMALL_WORKGROUP, **DECISION_OPTS), ref,
                       "decision batch, one workgroup of 64")


@pytest.mark.gpu
def test_gpu_a_converged_batch_comes_back_as_its_bits(lib, smooth_harness):  # noqa: F811
    """The decision batch's result fed back in.  Its two trajectories of the last sequence that stopped on the gradient
    (two legs; one with the plane of weights and the weightless NaN key point), as a batch of their own: every trajectory
    stops in the first STOP phase, no trial round launches, the output is the input's bits and info is (0, 0, 0).  (The
    whole result is no converged batch: a trajectory that ended on the cap goes on, the one on reason 2 spends its 25
    trials again, one that stalled tries once more.  It is run too, against the host rule.)"""
    ang, pose, weight, segs, bounds, _, first = decision_case(smooth_harness)
    S = ang.shape[0]
    assert (first["info"][S - 1, :2, 0] == 0).all()
    sub = (first["angles"][S - 1:, :2], pose[S - 1:, :2], weight[S - 1:, :2], segs[:2], bounds[:2])
    ref = smooth_harness.run(sub[0], sub[1], sub[3], sub[4], weight=sub[2], **DECISION_OPTS)
    assert ref["rounds"] == 0 and (ref["info"] == 0).all()
    for env in (None, ONE_SMALL_WORKGROUP):
        got = device_run(lib, *sub, env=env, **DECISION_OPTS)
        assert_equals_host(got, ref, ("converged", env))
        assert same_bits(got["angles"], sub[0]) and (got["info"] == 0).all()
        assert same_bits(got["cost"], first["cost"][S - 1:, :2, [1, 1]])
        assert np.array_equal(got["frame_info"], first["frame_info"][S - 1:, :2])
    again = smooth_harness.run(first["angles"], pose, segs, bounds, weight=weight, **DECISION_OPTS)
    stopped_at_once = (again["info"][..., 1:] == 0).all(-1)
    assert stopped_at_once.sum() >= 3 and (again["info"][stopped_at_once, 0] <= 1).all() and not stopped_at_once.all()
    got = device_run(lib, first["angles"], pose, weight, segs, bounds, **DECISION_OPTS)
    assert_equals_host(got, again, "the whole result fed back")
    assert same_bits(got["angles"][stopped_at_once], first["angles"][stopped_at_once])


LONG = ((1025, 60), (2049, 40))


@pytest.mark.gpu
@pytest.mark.parametrize("N,max_iter", LONG)
def test_gpu_eleven_and_twelve_strides(lib, smooth_harness, N, max_iter):  # noqa: F811
    """RF 0:1025 and 0:2049 of the shipped recording against the host rule bit for bit, with guards: one frame past a
    power of two, so n_pad is 2048 and 4096 and the last of the eleven and twelve strides reduces a single pair.

    The cap on the accepted steps (LONG: 60 and 40).  A trial round is 6 + 2 ceil(log2 N) launches, 28 and
    30 here, at the measured 15 us each 0.42 and 0.45 ms: 60 and 40 rounds are 25 and 18 ms of kernels, and by launches
    alone a cap in the thousands would fit a second.  What a round costs in this test is the host-run reference, about 25
    and 50 ms per round at these sizes; 60 and 40 rounds keep it to 1.5 and 2 s, and that is what sets the caps."""
    ang, pose, seg, bounds = shipped_window("RF", 0, N)
    ref = smooth_harness.run_one(ang, pose, seg, bounds, max_iter=max_iter)
    assert tuple(ref["info"][:2]) == (4, max_iter) and ref["cost"][1] < ref["cost"][0] and ref["rounds"] >= max_iter
    got = device_run(lib, ang[None, None], pose[None, None], None, [seg], [bounds], max_iter=max_iter)
    assert_equals_host({k: v[0, 0] for k, v in got.items()}, ref, f"RF 0:{N}")


@pytest.mark.gpu
def test_gpu_many_trips_of_the_grid_stride_loop_at_stride_512(lib, smooth_harness):  # noqa: F811
    """2 x 3 trajectories of 513 frames (ten strides, the last of 512 frames reduces one pair per trajectory) on one
    workgroup of 64 lanes: the eight-lanes-per-row phases walk 24 624 items in 385 trips of the grid-stride loop.  Six
    accepted steps at the most, which with the rejections between them are 16 rounds: one wavefront does all the work."""
    ang, pose, weight, segs, bounds, ref = case(smooth_harness, 2, 3, 513, 700 + 513, max_iter=6)
    assert (ref["info"][..., 1] > 0).all() and ref["rounds"] >= 6 and (ref["frame_info"] == BAD_INPUT).sum() == 1
    assert_equals_host(device_run(lib, ang, pose, weight, segs, bounds, max_iter=6, env=ONE_SMALL_WORKGROUP), ref,
                       "513 frames, one workgroup of 64")


@pytest.mark.gpu
def test_gpu_host_entry_point_equals_the_device_entry_point(lib, smooth_harness):  # noqa: F811
    import torch
    S, L, N = 2, 3, 33
    ang, pose, weight, segs, bounds, ref = case(smooth_harness, S, L, N, 700 + N, max_iter=30)
    params = _params_of(lib, segs, bounds)
    host = lib.smooth_legs(ang, pose, params, kp_weight=weight, max_iter=30)
    assert_equals_host(host, ref, "host entry")
    assert host["frame_info"].dtype == np.int32 and host["info"].dtype == np.int32
    # other options, no weights, only the angles asked for, on a stream of torch's
    s7 = np.array([0.0, 0.3, 0.1, 0.1, 0.02, 0.1, 1.0])
    ref2 = smooth_harness.run(ang, pose, segs, bounds, smooth=s7, max_iter=7, gtol=1e-6, ftol=1e-9)
    assert_equals_host(lib.smooth_legs(ang, pose, params, smooth=s7, max_iter=7, gtol=1e-6, ftol=1e-9), ref2, "host entry, options")
    d_ang, d_pose = (torch.from_numpy(x).cuda() for x in (ang, pose))
    need = lib.smooth_workspace_bytes(S, L, N)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_out = torch.full((S, L, N, 7), 7.0, dtype=torch.float64, device="cuda")
        d_ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        lib.smooth_legs_device(d_ang, d_pose, S, L, N, params, d_out, d_ws, need, smooth=s7, max_iter=7, gtol=1e-6, ftol=1e-9, stream=s)
    s.synchronize()
    assert same_bits(d_out.cpu().numpy(), ref2["angles"])
    with pytest.raises(ValueError, match="expected a int32 tensor"):
        lib.smooth_legs_device(d_ang, d_pose, S, L, N, params, d_out, d_ws, need, d_frame_info=d_out)
    # empty input: no launch, the output is not touched
    keep = d_out.clone()
    lib.smooth_legs_device(d_ang.data_ptr(), d_pose.data_ptr(), 0, L, N, params, d_out.data_ptr(), 0, 0)
    torch.cuda.synchronize()
    assert torch.equal(keep.view(torch.int64), d_out.view(torch.int64))


@pytest.mark.gpu
def test_gpu_600_frames_of_the_shipped_recording(lib, smooth_harness):  # noqa: F811
    """RF 0:600 at smooth = 0.1, run to the end: the properties, and the host rule's bits."""
    ang, pose, seg, bounds = shipped_window("RF", 0, 600)
    ref = smooth_harness.run_one(ang, pose, seg, bounds)
    got = device_run(lib, ang[None, None], pose[None, None], None, [seg], [bounds])
    assert_equals_host({k: v[0, 0] for k, v in got.items()}, ref, "RF 0:600")
    why, steps, _ = check_properties({k: v[0, 0] for k, v in got.items()}, ang, pose, seg, bounds, SMOOTH)
    assert why in (0, 1) and steps > 0
    start = np.clip(ang, bounds[:, 0], bounds[:, 1])
    print(f"RF 0:600: {steps} steps, {ref['rounds']} rounds, reason {why}, cost {got['cost'][0, 0]}, largest change "
          f"{largest_change(start):.3f} -> {largest_change(got['angles'][0, 0]):.3f}")
    assert largest_change(got["angles"][0, 0]) < largest_change(start)
