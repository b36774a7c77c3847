"""TEST INFRASTRUCTURE -- what the bit-for-bit tests of the per-pass cuts of csrc/seqik_core.hpp share
(tests/test_pass_path_cuts.py, tests/test_frame_constants.py, tests/test_trans_cuts.py): comparison as integers, the
LegParamsC fill, the narrowed limits, the C oracle's reference over a batch, the launch paths with the one assertion that
a path equals that reference, and the first-pass operands recorded from host runs of run_stage
(tests/harness/first_pass_harness.hip)."""
import ctypes
import functools
import os

import numpy as np

from conftest import ROOT, SEED_LINK_DOF, LegParamsC, load_golden
from harness_build import build_harness

dp = ctypes.POINTER(ctypes.c_double)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """bit for bit, a NaN on both sides counting as equal (NaN stays NaN)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def leg_struct(seg, bounds, seeds):
    lp = LegParamsC()
    for i in range(4):
        lp.seg[i] = seg[i]
    for i in range(7):
        lp.bounds[i][0], lp.bounds[i][1] = bounds[i][0], bounds[i][1]
    for i in range(27):
        lp.seeds[i] = seeds[i]
    return lp


def shipped_legs(oracle):
    from seqikpy_amd import data, utils
    body = utils.calculate_body_size(data.TEMPLATE_NMF_LOCOMOTION, data.LEGS)
    return [oracle.leg_params(l, data.BOUNDS_LOCOMOTION, body, data.INITIAL_ANGLES_LOCOMOTION) for l in data.LEGS]


def pin_seed(seeds, dof, value):
    for i, d in enumerate(SEED_LINK_DOF):
        if d == dof:
            seeds[i] = value


def narrow_limits(bounds, seeds):
    """In place: limits 1e-8 apart on one joint of every stage, around the joint's seed, which every chain is pinned to
    (steps around the xtol threshold; clears StageConst::fd_wide)."""
    for dof in (1, 2, 5, 6):   # ThC_pitch (stage 1), ThC_roll (2), FTi_pitch (3), TiTa_pitch (4)
        c = float(seeds[SEED_LINK_DOF.index(dof)])
        if dof == 6:
            c = -0.6           # (the shipped seed 0 sits on the shipped upper limit)
        bounds[dof] = (c - 0.5e-8, c + 0.5e-8)
        pin_seed(seeds, dof, c)


def oracle_reference(pose, cases):
    """The C oracle's angles, fk, status and nfev over pose [S, L, N, 5, 3] with cases[l] = (seg, bounds, seeds), read-only"""
    from oracle import c_oracle
    c_oracle.build()
    S, L, N = pose.shape[:3]
    ref = dict(angles=np.zeros((S, L, N, 7)), fk=np.zeros((S, L, N, 9, 3)),
               status=np.zeros((S, L, N, 4), np.int32), nfev=np.zeros((S, L, N, 4), np.int32))
    for li, (seg, b, seeds) in enumerate(cases):
        for s in range(S):
            r = c_oracle.seq_leg(pose[s, li], seg, b, seeds)
            for k in ref:
                ref[k][s, li] = r[k]
    for v in ref.values():
        v.setflags(write=False)
    return ref


LAUNCH_PATHS = dict(fused=dict(pipeline=1, lanes_per_wave=64), queue128=dict(pipeline=1, lanes_per_wave=128),
                    staged=dict(staged=1, lanes_per_wave=64), staged_diag=dict(want_diag=True), pipeline=dict(pipeline=2),
                    chunked=dict(frame_chunk=3, frame_halo=2, chunk_tol=-1.0, chunk_rounds=2),   # exact mode: == the serial walk
                    subset=None)


def solve_on_path(hiplib, pose, cases, ref, path):
    """The outputs of the launches that make up `path`"""
    params = [hiplib.leg_params_from_arrays(*c) for c in cases]
    if path == "subset":
        # stages k .. 4 from the stored angles of the earlier stages: the FROM_ANGLES instantiations, which rebuild the
        # prefix (and read its translation for the FK rows of the stages that are not run)
        outs = []
        for first in (2, 3, 4):
            prior = ref["angles"].copy()
            prior[..., 2 * (first - 1):] = 0.0
            outs.append(hiplib.solve_seq(pose, params, first_stage=first, last_stage=4, angles=prior, want_fk=True))
    else:
        outs = [hiplib.solve_seq(pose, params, want_fk=True, **LAUNCH_PATHS[path])]
    hiplib.check_faults()
    return outs


def assert_equal_reference(outs, ref, path, n_chains=None):
    for out in outs:
        assert np.array_equal(bits(out["angles"]), bits(ref["angles"]))
        assert np.array_equal(bits(out["fk"]), bits(ref["fk"]))
    if path == "staged_diag":
        assert np.array_equal(outs[0]["status"], ref["status"])
        assert np.array_equal(outs[0]["nfev"], ref["nfev"])
    if path == "chunked":
        assert outs[0]["chunk_stats"]["chunks"] == 2 * n_chains   # every chain was cut into two chunks


ROW = 28   # doubles per recorded row; column 27 = stage (first_pass_harness.hip)


@functools.lru_cache(maxsize=None)
def first_pass_rows():
    """First-pass operands of every solve of host runs of run_stage over the shipped recording, all six legs: rows
    [2400][ROW] in the order leg, frame, stage; read-only."""
    lib = ctypes.CDLL(build_harness(os.path.join(ROOT, "tests", "harness", "first_pass_harness.hip")))
    lib.fp_record.restype = ctypes.c_int64
    lib.fp_record.argtypes = [dp, ctypes.c_int64, ctypes.POINTER(LegParamsC), dp, ctypes.c_int64]
    z = load_golden("df3d_100")
    rows = []
    for leg in [str(l) for l in z["legs"]]:
        pose = np.ascontiguousarray(z[f"{leg}_pose"], dtype=np.float64)
        r = np.zeros((4 * len(pose), ROW))
        n = lib.fp_record(pose.ctypes.data_as(dp), len(pose), ctypes.byref(leg_struct(z[f"{leg}_seg"], z[f"{leg}_bounds"],
                                                                                      z[f"{leg}_seeds"])),
                          r.ctypes.data_as(dp), len(r))
        assert n == len(r)
        rows.append(r)
    rows = np.concatenate(rows)
    assert rows.shape == (2400, ROW) and np.all(np.isfinite(rows))
    rows.setflags(write=False)
    return rows
