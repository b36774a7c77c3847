#!/usr/bin/env python3
"""Writes tests/golden/leg_records_pin.npz: fixed inputs and the raw outputs of the host harnesses of link frames, leg
Jacobians, fit sensitivity and refinement (tests/harness/*.hip), built from the harness directory given -- that of the
commit the pin is taken from (a `git worktree` of it).  tests/test_leg_records_pin.py holds this tree's harnesses to
those outputs bit for bit.  Needs hipcc, no GPU.

    python tests/tools/leg_records_pin.py <tree>/tests/harness <build dir> [out.npz]

Entries that must agree bit for bit in any tree (a staged entry with its plain one, the reduce-only Jacobian entry with
the full one) are checked here and stored once (SAME_AS)."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "sequential-inverse-kinematics_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from conftest import DOFS, LegParamsC, load_golden  # noqa: E402
from harness_build import build_harness  # noqa: E402

N = 32                       # leg-frames per chain kind: a multiple of 16, so that the staged entries run
ANGLE_MAX = 1073741824.0     # SEQIK_ANGLE_MAX
# the rows set by hand
ROW_NAN, ROW_INF, ROW_BEYOND, ROW_POSE, ROW_UB, ROW_LB, ROW_ZERO, ROW_WEIGHT = 3, 7, 11, 13, 17, 19, 23, 21
BAD_ANGLE_ROWS = (ROW_NAN, ROW_INF, ROW_BEYOND)              # NaN records in every unit
BAD_INPUT_ROWS = BAD_ANGLE_ROWS + (ROW_POSE,)                # ... and in the units that read the pose
SAME_AS = {"frames_staged": "frames", "frames_origin_staged": "frames_origin", "jac_staged": "jac",
           "sigma_reduce": "sigma", "vel_reduce": "vel", "sens_staged": "sens"}
INPUTS = ("seg", "bounds", "angles_seq", "angles_gen", "pose", "qdot", "kp_sigma", "kp_weight")


def pin_inputs():
    """The inputs: RF of the shipped recording's segments with the shipped locomotion limits, angles from a fixed seed
    inside them, key points = the chain's own (float64 restatement) plus noise, and the hand-set rows."""
    from seqikpy_amd.data import BOUNDS_LOCOMOTION
    from sensitivity_support import KEY_LINKS, numpy_frames
    rng = np.random.default_rng(20261021)
    seg = np.asarray(load_golden("anipose_shipped")["RF_seg"], dtype=np.float64)
    bounds = np.array([[float(v) for v in BOUNDS_LOCOMOTION[f"RF_{d}"]] for d in DOFS])
    inp = {"seg": seg, "bounds": bounds}
    for kind in ("seq", "gen"):
        ang = rng.uniform(bounds[:, 0], bounds[:, 1], (N, 7))
        ang[ROW_NAN, 2], ang[ROW_INF, 5], ang[ROW_BEYOND, 0] = np.nan, -np.inf, 2.0 * ANGLE_MAX
        ang[ROW_UB, 6], ang[ROW_LB, 1] = bounds[6, 1], bounds[1, 0]
        ang[ROW_ZERO] = 0.0
        inp[f"angles_{kind}"] = ang
    pose = np.empty((N, 5, 3))
    pose[:, 0] = rng.normal(0.0, 1.0, (N, 3))
    for i in range(N):
        q = inp["angles_seq"][i]
        fr = numpy_frames(q if np.all(np.abs(q) <= ANGLE_MAX) else np.zeros(7), seg)
        pose[i, 1:] = pose[i, 0] + fr[list(KEY_LINKS), :, 3] + rng.normal(0.0, 0.02, (4, 3))
    pose[ROW_POSE, 2, 0] = np.inf
    inp["pose"] = pose
    inp["qdot"] = rng.normal(0.0, 3.0, (N, 7))
    inp["kp_sigma"] = rng.uniform(0.005, 0.05, (N, 4))
    inp["kp_weight"] = rng.uniform(0.5, 2.0, (N, 4))
    inp["kp_weight"][ROW_WEIGHT, 1] = 0.0
    return inp


def run_harnesses(harness_dir, build_dir, inp):
    """Every output of the pin from the harnesses of `harness_dir` (built into `build_dir`) -> {name: array}; the names of
    frames and Jacobians carry the chain kind (`_seq` / `_gen`)."""
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    lib = {u: ctypes.CDLL(build_harness(os.path.join(harness_dir, f"{u}_harness.hip"), build_dir))
           for u in ("frames", "jacobian", "sensitivity", "refine")}
    lp = LegParamsC()
    for i in range(4):
        lp.seg[i] = float(inp["seg"][i])
    for d in range(7):
        lp.bounds[d][0], lp.bounds[d][1] = float(inp["bounds"][d][0]), float(inp["bounds"][d][1])
    leg = ctypes.byref(lp)
    c = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    ptr = lambda a: a.ctypes.data_as(dp)  # noqa: E731
    new = lambda *shape: np.full(shape, 7.0)  # noqa: E731
    n, n64 = N, ctypes.c_int64(N)
    pose, origin = c(inp["pose"]), c(inp["pose"][:, 0])
    qdot, sig, w = c(inp["qdot"]), c(inp["kp_sigma"]), c(inp["kp_weight"])
    out = {}

    def call(fn, *args):
        fn.restype = ctypes.c_int
        assert fn(*args) == 0, fn.__name__

    for kind, tag in ((0, "seq"), (1, "gen")):
        ang = c(inp[f"angles_{tag}"])
        for name, o in (("frames", None), ("frames_origin", ptr(origin))):
            for fn, suffix in ((lib["frames"].harness_link_frames, ""), (lib["frames"].harness_link_frames_staged, "_staged")):
                res = new(n, 9, 3, 4)
                call(fn, ptr(ang), n64, leg, ctypes.c_int32(kind), o, ptr(res))
                out[f"{name}{suffix}_{tag}"] = res
        jac, sigma, vel = new(n, 4, 3, 7), new(n, 8), new(n, 4, 3)
        call(lib["jacobian"].harness_leg_jacobians, ptr(ang), n64, leg, ctypes.c_int32(kind), ptr(qdot), ptr(jac), ptr(sigma),
             ptr(vel))
        sigma_r, vel_r, jac_s = new(n, 8), new(n, 4, 3), new(n, 4, 3, 7)
        call(lib["jacobian"].harness_leg_jacobians_reduce_only, ptr(ang), n64, leg, ctypes.c_int32(kind), ptr(qdot),
             ptr(sigma_r), ptr(vel_r))
        call(lib["jacobian"].harness_leg_jacobians_staged, ptr(ang), n64, leg, ctypes.c_int32(kind), ptr(jac_s))
        for name, res in (("jac", jac), ("sigma", sigma), ("vel", vel), ("sigma_reduce", sigma_r), ("vel_reduce", vel_r),
                          ("jac_staged", jac_s)):
            out[f"{name}_{tag}"] = res
    ang = c(inp["angles_seq"])
    tol = ctypes.c_double(1e-6)   # SEQIK_SENS_BOUND_TOL
    sens, std, flags, sens_s = new(n, 7, 4, 3), new(n, 7), np.full(n, -1, dtype=np.int32), new(n, 7, 4, 3)
    call(lib["sensitivity"].harness_fit_sensitivity, ptr(ang), ptr(pose), n64, leg, ptr(sig), tol, ptr(sens), ptr(std),
         flags.ctypes.data_as(ip))
    call(lib["sensitivity"].harness_fit_sensitivity_staged, ptr(ang), ptr(pose), n64, leg, tol, ptr(sens_s))
    out.update(sens=sens, std=std, flags=flags, sens_staged=sens_s)
    r_ang, r_cost, r_info = new(n, 7), new(n, 2), np.full(n, -1, dtype=np.int32)
    call(lib["refine"].harness_refine_legs, ptr(ang), ptr(pose), n64, leg, ptr(w), ctypes.c_int32(200), ctypes.c_double(1e-10),
         ctypes.c_double(1e-14), ptr(r_ang), ptr(r_cost), r_info.ctypes.data_as(ip))   # the defaults of seqik_refine.h
    out.update(refine_angles=r_ang, refine_cost=r_cost, refine_info=r_info)
    return out


def stored_name(name):
    """The fixture's key for output `name`: entries that must agree bit for bit are stored once."""
    for dup, base in SAME_AS.items():
        if name.startswith(dup + "_") or name == dup:
            return base + name[len(dup):]
    return name


def same_bits(a, b):
    view = np.int32 if a.dtype == np.int32 else np.uint64
    return a.shape == b.shape and np.array_equal(a.view(view), b.view(view))


def main():
    harness_dir, build_dir = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "tests", "golden", "leg_records_pin.npz")
    inp = pin_inputs()
    out = run_harnesses(harness_dir, build_dir, inp)
    keep = dict(inp)
    for name, res in out.items():
        if stored_name(name) != name:
            assert same_bits(res, out[stored_name(name)]), name
        else:
            keep[name] = res
    np.savez_compressed(path, **keep)
    print(f"{path}: {len(keep)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
