"""TEST INFRASTRUCTURE -- what the tests of the trajectory refinement (include/seqik_smooth.h) share: the host harness
(csrc/seqik_smooth.hpp compiled for the host), float64 numpy restatements of its parts (the cost, the gradient and held
rule, the parallel cyclic reduction), block rows made from real normal equations, the shipped windows the issue names,
and real scipy on the stacked problem.  Nothing here is taken from csrc."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import ROOT, LegParamsC, load_golden
from harness_build import build_harness
from refine_support import made_up_legs, numpy_model, targets_of
from sensitivity_support import leg_params

MAX_ITER, GTOL, FTOL, SMOOTH = 300, 1e-10, 1e-14, 0.1
BAD_INPUT = 1 << 24
PROFILE = os.path.join(ROOT, "profiles", "smooth_vs_scipy.json")
EPS = np.finfo(float).eps


def smooth7(smooth):
    s = np.ascontiguousarray(np.broadcast_to(np.asarray(smooth, dtype=np.float64), (7,)))
    return s


def legs_array(segs, bounds):
    lps = [leg_params(s, b) for s, b in zip(segs, bounds)]
    return (LegParamsC * len(lps))(*lps)


class SmoothHarness:
    def __init__(self, so, fk_so):
        dp, ip, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(LegParamsC)
        self.lib = ctypes.CDLL(so)
        self.lib.harness_smooth_legs.restype = ctypes.c_int
        self.lib.harness_smooth_legs.argtypes = [dp, dp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, lp, dp, dp,
                                                 ctypes.c_int32, ctypes.c_double, ctypes.c_double, dp, ip, dp, ip,
                                                 ctypes.POINTER(ctypes.c_int64)]
        self.lib.harness_smooth_solve.restype = ctypes.c_int
        self.lib.harness_smooth_solve.argtypes = [dp, ctypes.c_int64, dp]
        self.fk = ctypes.CDLL(fk_so)
        self.fk.harness_fk.restype = ctypes.c_int
        self.fk.harness_fk.argtypes = [dp, ctypes.c_int64, lp, ctypes.c_int32, dp, ctypes.c_int64, dp, dp]

    def run(self, angles, pose, segs, bounds, smooth=SMOOTH, weight=None, max_iter=MAX_ITER, gtol=GTOL, ftol=FTOL,
            in_place=False):
        """(S, L, N, 7), (S, L, N, 5, 3), L segment sets and limits [, weights that broadcast to (S, L, N, 4)]
        -> dict(angles (S, L, N, 7), frame_info (S, L, N), cost (S, L, 2), info (S, L, 3), rounds)"""
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        angles = np.array(angles, dtype=np.float64, order="C")      # a copy: in_place writes into it
        pose = np.ascontiguousarray(pose, dtype=np.float64)
        S, L, N = angles.shape[:3]
        assert angles.shape == (S, L, N, 7) and pose.shape == (S, L, N, 5, 3) and len(segs) == len(bounds) == L
        w = None if weight is None else np.ascontiguousarray(np.broadcast_to(weight, (S, L, N, 4)), dtype=np.float64)
        out = angles if in_place else np.full((S, L, N, 7), 7.0)
        finfo, cost, info = np.full((S, L, N), -1, dtype=np.int32), np.full((S, L, 2), 7.0), np.full((S, L, 3), -1, dtype=np.int32)
        rounds = ctypes.c_int64(0)
        ptr = lambda a: a.ctypes.data_as(dp) if a is not None else None  # noqa: E731
        rc = self.lib.harness_smooth_legs(ptr(angles), ptr(pose), S, L, N, legs_array(segs, bounds), ptr(w), ptr(smooth7(smooth)),
                                          max_iter, gtol, ftol, ptr(out), finfo.ctypes.data_as(ip), ptr(cost),
                                          info.ctypes.data_as(ip), ctypes.byref(rounds))
        assert rc == 0
        return dict(angles=out, frame_info=finfo, cost=cost, info=info, rounds=rounds.value)

    def run_one(self, angles, pose, seg, bounds, **kw):
        """One trajectory: (N, 7), (N, 5, 3) -> the same dictionary without the leading (1, 1)."""
        w = kw.pop("weight", None)
        if w is not None:
            w = np.broadcast_to(w, (len(angles), 4))[None, None]
        res = self.run(np.asarray(angles)[None, None], np.asarray(pose)[None, None], [seg], [bounds], weight=w, **kw)
        return {k: (v[0, 0] if isinstance(v, np.ndarray) else v) for k, v in res.items()}

    def solve(self, D, L, U, b):
        """The linear solve alone: blocks (N, 7, 7) x 3 and b (N, 7) -> delta (N, 7), whether a pivot was not positive."""
        dp = ctypes.POINTER(ctypes.c_double)
        N = len(D)
        rows = np.ascontiguousarray(np.concatenate([D.reshape(N, 49), L.reshape(N, 49), U.reshape(N, 49), b.reshape(N, 7)], 1))
        delta = np.full((N, 7), 7.0)
        rc = self.lib.harness_smooth_solve(rows.ctypes.data_as(dp), N, delta.ctypes.data_as(dp))
        assert rc in (0, 1)
        return delta, rc == 1


@pytest.fixture(scope="module")
def smooth_harness():
    # (torch first where there is one: refine_support.refine_harness says why)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    return SmoothHarness(build_harness(os.path.join(ROOT, "tests", "harness", "smooth_harness.hip")),
                         build_harness(os.path.join(ROOT, "tests", "harness", "fk_harness.hip")))


def record(key, value):
    """Keeps a measured value in profiles/smooth_vs_scipy.json when SEQIK_RECORD_PROFILES is set (the committed file is
    the record of one such run; a plain test run writes nothing)."""
    if not os.environ.get("SEQIK_RECORD_PROFILES"):
        return
    data = {}
    if os.path.exists(PROFILE):
        with open(PROFILE) as f:
            data = json.load(f)
    data[key] = value
    with open(PROFILE, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


# ------------------------------------------------------- inputs -------------------------------------------------------

def shipped_window(leg, lo, hi):
    """Frames lo:hi of a leg of tests/golden/anipose_shipped.npz -> the sequential fit's angles (n, 7), pose (n, 5, 3), seg,
    bounds"""
    z = load_golden("anipose_shipped")
    return z[f"{leg}_angles"][lo:hi].copy(), z[f"{leg}_pose"][lo:hi, :5].copy(), z[f"{leg}_seg"], z[f"{leg}_bounds"]


def made_up_trajectories():
    """refine_support.made_up_legs() as 40 trajectories of 24 frames -> [(angles (24, 7), pose (24, 5, 3), seg, bounds)]"""
    return made_up_legs()


def largest_change(angles):
    """The largest frame-to-frame change of any angle over the neighbouring good frames of (N, 7) angles (0 if none)."""
    d = np.abs(np.diff(angles, axis=0))
    d = d[np.isfinite(d)]
    return float(d.max()) if d.size else 0.0


# ------------------------------------------------ float64 restatements ------------------------------------------------

def stiffness(smooth, seg):
    return smooth7(smooth) * np.sum(seg) ** 2


def numpy_bad(angles, pose, weight=None):
    """Rule 1 of include/seqik_refine.h per frame -> (N,) bool"""
    N = len(angles)
    w = np.ones((N, 4)) if weight is None else np.broadcast_to(weight, (N, 4))
    bad = ~(np.abs(angles) <= 2.0 ** 30).all(1)                      # (false for NaN)
    bad |= ~np.isfinite(w).all(1) | (np.nan_to_num(w) < 0).any(1) | ~np.isfinite(pose[:, 0]).all(1)
    for k in range(4):
        bad |= (w[:, k] != 0) & ~np.isfinite(pose[:, k + 1]).all(1)
    return bad


def numpy_parts(q, pose, seg, bounds, smooth, weight=None, bad=None):
    """C, the full gradient (N, 7) (half the derivative, as the rule keeps it) and the held set (N, 7) at the angles q
    (N, 7) of one trajectory; frames in `bad` take no part (their rows are 0 / False)."""
    N = len(q)
    w = np.ones((N, 4)) if weight is None else np.broadcast_to(weight, (N, 4))
    bad = np.zeros(N, dtype=bool) if bad is None else bad
    s = stiffness(smooth, seg)
    lb, ub = np.asarray(bounds)[:, 0], np.asarray(bounds)[:, 1]
    C, g = 0.0, np.zeros((N, 7))
    for t in range(N):
        if bad[t]:
            continue
        r, J = numpy_model(q[t], targets_of(pose[t], w[t]), w[t], seg)
        C += r @ r
        g[t] = J.T @ r
        for u in (t - 1, t + 1):
            if 0 <= u < N and not bad[u]:
                g[t] += s * (q[t] - q[u])
        if t > 0 and not bad[t - 1]:
            C += np.sum(s * (q[t] - q[t - 1]) ** 2)
    held = ((q <= lb) & (g > 0)) | ((q >= ub) & (g < 0))
    held[bad] = False
    return C, g, held


def sym_lower(D):
    """The symmetric matrix whose lower triangle is D's (the rule reads only that)."""
    return np.tril(D) + np.tril(D, -1).T


def dense_system(D, L, U, b):
    """The block-tridiagonal system as one dense matrix (7 N, 7 N) and right-hand side (7 N,)."""
    N = len(D)
    M = np.zeros((7 * N, 7 * N))
    for t in range(N):
        M[7 * t:7 * t + 7, 7 * t:7 * t + 7] = sym_lower(D[t])
        if t > 0:
            M[7 * t:7 * t + 7, 7 * t - 7:7 * t] = L[t]
        if t + 1 < N:
            M[7 * t:7 * t + 7, 7 * t + 7:7 * t + 14] = U[t]
    return M, b.reshape(-1)


def _chol_solve(D, X):
    c = np.linalg.cholesky(sym_lower(D))            # raises LinAlgError where a pivot is not positive
    return np.linalg.solve(c.T, np.linalg.solve(c, X))


def numpy_pcr(D, L, U, b):
    """The parallel cyclic reduction of include/seqik_smooth.h in float64 numpy: strides 1, 2, 4, ... while h < N, every
    row normalised by its Cholesky factor, then every row reduced -> delta (N, 7).  The reference arithmetic of the
    linear-solve test, not the code under test."""
    N = len(D)
    D, L, U, b = D.copy(), L.copy(), U.copy(), b.copy()
    h = 1
    while h < N:
        EL = np.stack([_chol_solve(D[u], L[u]) for u in range(N)])
        EU = np.stack([_chol_solve(D[u], U[u]) for u in range(N)])
        eb = np.stack([_chol_solve(D[u], b[u]) for u in range(N)])
        Dn, Ln, Un, bn = sym_lower_all(D), np.zeros_like(L), np.zeros_like(U), b.copy()
        for t in range(N):
            if t - h >= 0:
                Dn[t] -= L[t] @ EU[t - h]
                Ln[t] = -(L[t] @ EL[t - h])
                bn[t] -= L[t] @ eb[t - h]
            if t + h < N:
                Dn[t] -= U[t] @ EL[t + h]
                Un[t] = -(U[t] @ EU[t + h])
                bn[t] -= U[t] @ eb[t + h]
        D, L, U, b = Dn, Ln, Un, bn
        h *= 2
    return np.stack([_chol_solve(D[t], b[t]) for t in range(N)])


def sym_lower_all(D):
    return np.stack([sym_lower(d) for d in D])


def block_rows(N, seed, smooth=SMOOTH, lam=1e-3):
    """A block-tridiagonal system as step 4 builds it, N rows: D from the real normal equations of made-up leg-frames
    (J^T J of refine_support.numpy_model at their seeds, plus the penalty, plus lambda diag), random held masks, some
    broken pairs and some identity rows (bad frames) -> D, L, U (N, 7, 7), b (N, 7)"""
    rng = np.random.default_rng(seed)
    legs = made_up_legs()
    ang, pose, seg, bounds = legs[seed % len(legs)]
    s = stiffness(smooth, seg)
    bad = rng.random(N) < 0.1
    held = rng.random((N, 7)) < 0.15
    broken = rng.random(N) < 0.1                    # the pair (t - 1, t) does not exist although both frames are good
    pair = np.array([t > 0 and not bad[t] and not bad[t - 1] and not broken[t] for t in range(N)])
    D, L, U, b = np.zeros((N, 7, 7)), np.zeros((N, 7, 7)), np.zeros((N, 7, 7)), np.zeros((N, 7))
    for t in range(N):
        if bad[t]:
            D[t] = np.eye(7)
            continue
        i = rng.integers(len(ang))
        q = np.clip(ang[i] + 0.1 * rng.standard_normal(7), bounds[:, 0], bounds[:, 1])
        r, J = numpy_model(q, targets_of(pose[i], np.ones(4)), np.ones(4), seg)
        A, g = J.T @ J, J.T @ r
        n_pairs = int(pair[t]) + int(t + 1 < N and pair[t + 1])
        A = A + n_pairs * np.diag(s)
        d = np.where(np.diag(A) <= 0, np.finfo(float).tiny, np.diag(A))
        M = A + lam * np.diag(d)
        f = ~held[t]
        D[t] = np.where(np.outer(f, f), M, 0.0) + np.diag(np.where(f, 0.0, 1.0))
        b[t] = np.where(f, -g, 0.0)
        if pair[t]:
            L[t] = -np.diag(np.where(f & ~held[t - 1], s, 0.0))
            U[t - 1] = L[t].T
    return D, L, U, b


# ---------------------------------------------------- real scipy ----------------------------------------------------

def scipy_smooth(angles, pose, seg, bounds, smooth=SMOOTH):
    """scipy.optimize.least_squares (TRF, bounds, analytic Jacobian, xtol = ftol = 1e-14, gtol = 1e-12) on the stacked
    residuals of one trajectory without bad frames -- the 12 data residuals of every frame, then sqrt(s_j) times the
    differences of neighbouring frames -- from the clamped start -> (angles (N, 7), C there: twice scipy's cost)."""
    from scipy.optimize import least_squares
    N = len(angles)
    lb, ub = np.asarray(bounds)[:, 0], np.asarray(bounds)[:, 1]
    rs = np.sqrt(stiffness(smooth, seg))
    w = np.ones(4)
    t = [targets_of(pose[i], w) for i in range(N)]

    def res(x):
        q = x.reshape(N, 7)
        data = [numpy_model(q[i], t[i], w, seg)[0] for i in range(N)]
        return np.concatenate(data + [(rs * np.diff(q, axis=0)).ravel()])

    def jac(x):
        q = x.reshape(N, 7)
        J = np.zeros((12 * N + 7 * (N - 1), 7 * N))
        for i in range(N):
            J[12 * i:12 * i + 12, 7 * i:7 * i + 7] = numpy_model(q[i], t[i], w, seg)[1]
        for i in range(N - 1):
            row = 12 * N + 7 * i
            J[row:row + 7, 7 * i:7 * i + 7] = -np.diag(rs)
            J[row:row + 7, 7 * i + 7:7 * i + 14] = np.diag(rs)
        return J

    sol = least_squares(res, np.clip(angles, lb, ub).ravel(), jac=jac, bounds=(np.tile(lb, N), np.tile(ub, N)), method="trf",
                        xtol=1e-14, ftol=1e-14, gtol=1e-12, max_nfev=5000)
    return sol.x.reshape(N, 7), 2.0 * sol.cost


# ------------------------------------- the library call answered by the host harness -------------------------------------

def harness_call(sh, real_call):
    """A stand-in for ``_lib._call`` that answers ``seqik_smooth_legs`` with the host-run rule: what the CPU tier can run
    of the Python surface (the product itself has no CPU path)."""
    def call(name, *args):
        if name == "seqik_smooth_legs":
            angles, pose, S, L, N, legs, kind, weight, opt, out, finfo, cost, info, device = args
            assert kind == 0
            o = opt._obj
            rc = sh.lib.harness_smooth_legs(angles, pose, S, L, N, ctypes.cast(legs, ctypes.POINTER(LegParamsC)), weight,
                                            o.smooth, o.max_iter, o.gtol, o.ftol, out, finfo, cost, info, None)
            assert rc == 0
            return None
        return real_call(name, *args)
    return call
