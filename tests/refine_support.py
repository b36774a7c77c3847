"""TEST INFRASTRUCTURE -- what the tests of the whole-leg refinement (include/seqik_refine.h) share: the host harness
(csrc/seqik_refine.hpp compiled for the host), a float64 numpy restatement of the rule, the inputs (the 575 frames of the
shipped recording the issue names, 40 made-up legs of 24 frames), real scipy from the same start, and the gradient at
200 bits on ``mp_chain`` of tests/test_fk_accuracy.py.  Nothing here is taken from csrc."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT, LegParamsC, load_golden, random_leg_case
from harness_build import build_harness
from sensitivity_support import DOF_LINK, KEY_LINKS, _mp_cross, _mp_dot, leg_params, numpy_frames
from test_fk_accuracy import _MP, mp_chain

MAX_ITER, GTOL, FTOL = 200, 1e-10, 1e-14
BAD_INPUT = 1 << 24
NONZERO = np.array([[d < 2 * (k + 1) or k == 3 for d in range(7)] for k in range(4)])   # (key point, DOF)
SEED_OF_DOF = [1, 2, 7, 8, 15, 16, 25]      # the start value of every DOF among a leg's 27 seeds


def reason(info):
    return (np.asarray(info) >> 8) & 7


def iterations(info):
    return (np.asarray(info) >> 16) & 255


def held_bits(info):
    return (np.asarray(info)[..., None] >> np.arange(7)) & 1 == 1


class RefineHarness:
    def __init__(self, so, fk_so):
        dp, ip, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(LegParamsC)
        self.lib = ctypes.CDLL(so)
        self.lib.harness_refine_legs.restype = ctypes.c_int
        self.lib.harness_refine_legs.argtypes = [dp, dp, ctypes.c_int64, lp, dp, ctypes.c_int32, ctypes.c_double,
                                                 ctypes.c_double, dp, dp, ip]
        self.fk = ctypes.CDLL(fk_so)
        self.fk.harness_fk.restype = ctypes.c_int
        self.fk.harness_fk.argtypes = [dp, ctypes.c_int64, lp, ctypes.c_int32, dp, ctypes.c_int64, dp, dp]

    def run(self, angles, pose, seg, bounds, weight=None, max_iter=MAX_ITER, gtol=GTOL, ftol=FTOL, want_cost=True,
            want_info=True, in_place=False):
        """(n, 7), (n, 5, 3) [, anything that broadcasts to (n, 4)] -> angles (n, 7), cost (n, 2) or None, info (n,) or None"""
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        angles = np.array(angles, dtype=np.float64, order="C")      # a copy: in_place writes into it
        pose = np.ascontiguousarray(pose, dtype=np.float64)
        n = angles.shape[0]
        assert angles.shape == (n, 7) and pose.shape == (n, 5, 3)
        w = None if weight is None else np.ascontiguousarray(np.broadcast_to(weight, (n, 4)), dtype=np.float64)
        out = angles if in_place else np.full((n, 7), 7.0)
        cost = np.full((n, 2), 7.0) if want_cost else None
        info = np.full(n, -1, dtype=np.int32) if want_info else None
        lp = leg_params(seg, bounds)
        ptr = lambda a: a.ctypes.data_as(dp) if a is not None else None  # noqa: E731
        rc = self.lib.harness_refine_legs(ptr(angles), ptr(pose), n, ctypes.byref(lp), ptr(w), max_iter, gtol, ftol, ptr(out),
                                          ptr(cost), info.ctypes.data_as(ip) if info is not None else None)
        assert rc == 0
        return out, cost, info


@pytest.fixture(scope="module")
def refine_harness():
    # The harness libraries link the HIP runtime hipcc ships with; torch bundles its own.  Whichever is loaded first owns
    # the GPU (seqikpy_amd/_lib.py, load()), so in a process that will use torch, torch goes first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    return RefineHarness(build_harness(os.path.join(ROOT, "tests", "harness", "refine_harness.hip")),
                         build_harness(os.path.join(ROOT, "tests", "harness", "fk_harness.hip")))


def host_batch(rh, ang, pose, segs, bounds, weight=None, **kw):
    """The host-run rule over a (S, L, N, ...) batch, leg by leg -> angles (S, L, N, 7), cost (S, L, N, 2), info (S, L, N)."""
    S, L, N = ang.shape[:3]
    out, cost, info = np.empty((S, L, N, 7)), np.empty((S, L, N, 2)), np.empty((S, L, N), dtype=np.int32)
    for li in range(L):
        w = None if weight is None else np.ascontiguousarray(weight[:, li]).reshape(-1, 4)
        a, c, f = rh.run(np.ascontiguousarray(ang[:, li]).reshape(-1, 7), np.ascontiguousarray(pose[:, li]).reshape(-1, 5, 3),
                         segs[li], bounds[li], w, **kw)
        out[:, li], cost[:, li], info[:, li] = a.reshape(S, N, 7), c.reshape(S, N, 2), f.reshape(S, N)
    return out, cost, info


# ------------------------------------------------------- inputs -------------------------------------------------------

def shipped_frames():
    """The issue's 575 frames of tests/golden/anipose_shipped.npz: RF 0, 20, ... (300), LF 0, 24, ... plus 280..304 (275)
    -> [(leg, frames, angles (n, 7), pose (n, 5, 3), seg, bounds)]"""
    z = load_golden("anipose_shipped")
    rf = np.arange(0, 6000, 20)
    lf = np.concatenate([np.arange(0, 6000, 24), np.arange(280, 305)])   # (frame 288 is in both: 275 entries, 274 frames)
    assert len(rf) == 300 and len(lf) == 275
    return [(leg, fr, z[f"{leg}_angles"][fr], z[f"{leg}_pose"][fr], z[f"{leg}_seg"], z[f"{leg}_bounds"])
            for leg, fr in (("RF", rf), ("LF", lf))]


_MADE_UP = []


def made_up_legs():
    """40 made-up legs of 24 frames (conftest.random_leg_case: targets far out of reach, on the origin, repeated), every
    frame started from the leg's seeds (some of which sit on a limit) -> [(angles (24, 7), pose, seg, bounds)]"""
    if not _MADE_UP:
        rng = np.random.default_rng(20261020)
        for _ in range(40):
            pose, seg, bounds, seeds = random_leg_case(rng, 24)
            _MADE_UP.append((np.tile(seeds[SEED_OF_DOF], (24, 1)), pose, seg, bounds))
    return _MADE_UP


# ------------------------------------------------ float64 restatement ------------------------------------------------

def numpy_model(q, t, w, seg):
    """r (12,), J (12, 7) of one leg-frame at the angles q: t (4, 3) targets, w (4,) weights."""
    fr = numpy_frames(q, seg)
    axis = [fr[l, :, c] for l, c in DOF_LINK]
    org = [fr[l, :, 3] for l, _ in DOF_LINK]
    r, J = np.zeros((4, 3)), np.zeros((4, 3, 7))
    for k in range(4):
        f = fr[KEY_LINKS[k], :, 3]
        r[k] = w[k] * (f - t[k])
        for d in range(7):
            if NONZERO[k, d]:
                J[k, :, d] = w[k] * np.cross(axis[d], f - org[d])
    return r.ravel(), J.reshape(12, 7)


def targets_of(pose, w):
    """t (4, 3): pose[k] - pose[0], 0 for a key point without weight (it is not read)."""
    t = np.zeros((4, 3))
    for k in range(4):
        if w[k] != 0:
            t[k] = pose[k + 1] - pose[0]
    return t


def numpy_refine(ang, pose, seg, bounds, weight=None, max_iter=MAX_ITER, gtol=GTOL, ftol=FTOL):
    """The rule of include/seqik_refine.h for one leg-frame in float64 numpy (np.linalg.cholesky on the free DOFs)
    -> angles (7,), (cost at the clamped start, cost at the result), info."""
    w = np.ones(4) if weight is None else np.asarray(weight, dtype=np.float64)
    lb, ub = np.asarray(bounds)[:, 0], np.asarray(bounds)[:, 1]
    t = targets_of(pose, w)
    q = np.clip(ang, lb, ub)
    r, J = numpy_model(q, t, w, seg)
    c = c0 = r @ r
    lam, iters, last = 1e-3, 0, False
    bar = gtol * np.sum(seg) ** 2
    while True:
        g = J.T @ r
        held = ((q <= lb) & (g > 0)) | ((q >= ub) & (g < 0))
        F = np.where(~held)[0]
        if last:
            why = 1
            break
        if iters >= max_iter:
            why = 4
            break
        if len(F) == 0 or np.abs(g[F]).max() <= bar:
            why = 0
            break
        A = J[:, F].T @ J[:, F]
        d = np.where(np.diag(A) <= 0, np.finfo(float).tiny, np.diag(A))
        accepted = stalled = False
        while not accepted and not stalled and lam <= 1e12:
            try:
                Lc = np.linalg.cholesky(A + lam * np.diag(d))
                delta = np.linalg.solve(Lc.T, np.linalg.solve(Lc, -g[F]))
            except np.linalg.LinAlgError:
                lam *= 4
                continue
            qn = q.copy()
            qn[F] = np.clip(q[F] + delta, lb[F], ub[F])
            rn, Jn = numpy_model(qn, t, w, seg)
            cn = rn @ rn
            if cn < c:
                accepted, last = True, c - cn <= ftol * c
                q, r, J, c = qn, rn, Jn, cn
                iters += 1
                lam = max(lam / 3, 1e-12)
            elif np.any(qn != q) and cn - c <= ftol * c:
                stalled = True
            else:
                lam *= 4
        if not accepted:
            why = 1 if stalled else 2
            break
    return q, (c0, c), int(sum(1 << j for j in range(7) if held[j])) | (why << 8) | (iters << 16)


# ---------------------------------------------------- real scipy ----------------------------------------------------

def scipy_refine(ang, pose, seg, bounds):
    """scipy.optimize.least_squares (TRF, bounds, analytic Jacobian, xtol = ftol = 1e-14, gtol = 1e-12) from the clamped
    start -> (angles, the sum of squares there: twice scipy's cost)."""
    from scipy.optimize import least_squares
    w = np.ones(4)
    lb, ub = np.asarray(bounds)[:, 0], np.asarray(bounds)[:, 1]
    t = targets_of(pose, w)
    res = least_squares(lambda q: numpy_model(q, t, w, seg)[0], np.clip(ang, lb, ub), jac=lambda q: numpy_model(q, t, w, seg)[1],
                        bounds=(lb, ub), method="trf", xtol=1e-14, ftol=1e-14, gtol=1e-12, max_nfev=2000)
    return res.x, 2.0 * res.cost


# ------------------------------------------------- 200-bit yardstick -------------------------------------------------

def mp_gradient(q, pose, seg, weight=None):
    """g = J^T r of one leg-frame at the angles q, at 200 bits -> (7,) float64 of the exact values."""
    mpf = _MP.mpf
    w = [mpf(1)] * 4 if weight is None else [mpf(float(v)) for v in weight]
    fr = mp_chain(0, q, seg, np.zeros((5, 3)))[0]
    F = [[[mpf(float(fr[0, i, r, c])) + mpf(float(fr[1, i, r, c])) for c in range(4)] for r in range(3)] for i in range(9)]
    axis = [[F[l][r][c] for r in range(3)] for l, c in DOF_LINK]
    org = [[F[l][r][3] for r in range(3)] for l, _ in DOF_LINK]
    P = [[mpf(float(v)) for v in row] for row in pose]
    g = [mpf(0)] * 7
    for k in range(4):
        if w[k] == 0:
            continue
        f = [F[KEY_LINKS[k]][r][3] for r in range(3)]
        res = [w[k] * w[k] * (f[c] - (P[k + 1][c] - P[0][c])) for c in range(3)]
        for d in range(7):
            if NONZERO[k, d]:
                g[d] += _mp_dot(_mp_cross(axis[d], [f[c] - org[d][c] for c in range(3)]), res)
    return np.array([float(v) for v in g])


# ------------------------------------- the library call answered by the host harness -------------------------------------

def harness_call(rh, real_call):
    """A stand-in for ``_lib._call`` that answers ``seqik_refine_legs`` and ``seqik_forward_kinematics`` with the host-run
    rules, leg by leg: what the CPU tier can run of the Python surface (the product itself has no CPU path)."""
    addr = lambda ptr: ctypes.cast(ptr, ctypes.c_void_p).value if ptr is not None else None  # noqa: E731
    dp, ip, lpp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(LegParamsC)
    at = lambda base, width, i: None if base is None else ctypes.cast(base + 8 * width * i, dp)  # noqa: E731

    def call(name, *args):
        if name == "seqik_refine_legs":
            angles, pose, S, L, N, legs, kind, weight, opt, out, cost, info, device = args
            assert kind == 0
            o = opt._obj
            for s in range(S):
                for l in range(L):
                    i = (s * L + l) * N
                    f = None if info is None else ctypes.cast(addr(info) + 4 * i, ip)
                    rc = rh.lib.harness_refine_legs(at(addr(angles), 7, i), at(addr(pose), 15, i), N,
                                                    ctypes.cast(ctypes.byref(legs[l]), lpp), at(addr(weight), 4, i),
                                                    o.max_iter, o.gtol, o.ftol, at(addr(out), 7, i), at(addr(cost), 2, i), f)
                    assert rc == 0
            return None
        if name == "seqik_forward_kinematics":
            angles, S, L, N, legs, kind, pose, origin, fk, dist, device = args
            src, stride = (pose, 15) if pose is not None else (origin, 3)
            for s in range(S):
                for l in range(L):
                    i = (s * L + l) * N
                    rc = rh.fk.harness_fk(at(addr(angles), 7, i), N, ctypes.cast(ctypes.byref(legs[l]), lpp), kind,
                                          at(addr(src), stride, i), stride, at(addr(fk), 27, i), at(addr(dist), 4, i))
                    assert rc == 0
            return None
        return real_call(name, *args)
    return call
