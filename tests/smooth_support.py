"""TEST INFRASTRUCTURE -- what the tests of the trajectory refinement (include/seqik_smooth.h) share: the host harness
(csrc/seqik_smooth.hpp compiled for the host), float64 numpy restatements of its parts (the cost, the gradient and held
rule, the parallel cyclic reduction), block rows made from real normal equations, the shipped windows the issue names,
real scipy on the stacked problem (with weights and bad frames), LAPACK's banded solve refined in extended precision and
a block elimination at 200 bits for the linear solve, and C(Q) with its full gradient at 200 bits.  Nothing here is taken
from csrc."""
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
        self.lib.harness_smooth_legs_paths.restype = ctypes.c_int
        self.lib.harness_smooth_legs_paths.argtypes = self.lib.harness_smooth_legs.argtypes + [ctypes.POINTER(ctypes.c_int64)]
        self.lib.harness_smooth_solve.restype = ctypes.c_int
        self.lib.harness_smooth_solve.argtypes = [dp, ctypes.c_int64, dp]
        self.fk = ctypes.CDLL(fk_so)
        self.fk.harness_fk.restype = ctypes.c_int
        self.fk.harness_fk.argtypes = [dp, ctypes.c_int64, lp, ctypes.c_int32, dp, ctypes.c_int64, dp, dp]

    def run(self, angles, pose, segs, bounds, smooth=SMOOTH, weight=None, max_iter=MAX_ITER, gtol=GTOL, ftol=FTOL,
            in_place=False, paths=False):
        """(S, L, N, 7), (S, L, N, 5, 3), L segment sets and limits [, weights that broadcast to (S, L, N, 4)]
        -> dict(angles (S, L, N, 7), frame_info (S, L, N), cost (S, L, 2), info (S, L, 3), rounds); with `paths` the
        harness's own loop over the phases runs instead of smooth_run_host and the dictionary also holds paths (S, L, 3):
        trials lost to a pivot that was not positive, trials lost to an angle outside the domain, and the trial round
        after which the trajectory stopped."""
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
        args = (ptr(angles), ptr(pose), S, L, N, legs_array(segs, bounds), ptr(w), ptr(smooth7(smooth)), max_iter, gtol, ftol,
                ptr(out), finfo.ctypes.data_as(ip), ptr(cost), info.ctypes.data_as(ip), ctypes.byref(rounds))
        if paths:
            taken = np.full((S, L, 3), -1, dtype=np.int64)
            assert self.lib.harness_smooth_legs_paths(*args, taken.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) == 0
            return dict(angles=out, frame_info=finfo, cost=cost, info=info, rounds=rounds.value, paths=taken)
        assert self.lib.harness_smooth_legs(*args) == 0
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


_BLOCK_FRAMES = {}


def _block_frames(N, seed, cut, hold):
    """What block_rows(N, seed, ...) draws and evaluates whatever the penalty and the damping (kept for the last few
    (N, seed): the grids vary those two) -> seg, bad (N,), held (N, 7), pair (N,), [(J^T J, J^T r) or None per frame]"""
    if (N, seed, cut, hold) not in _BLOCK_FRAMES:
        rng = np.random.default_rng(seed)
        legs = made_up_legs()
        ang, pose, seg, bounds = legs[seed % len(legs)]
        bad = rng.random(N) < cut
        held = rng.random((N, 7)) < hold
        broken = rng.random(N) < cut                # the pair (t - 1, t) does not exist although both frames are good
        pair = np.array([t > 0 and not bad[t] and not bad[t - 1] and not broken[t] for t in range(N)])
        normal = [None] * N
        for t in range(N):
            if bad[t]:
                continue
            i = rng.integers(len(ang))
            q = np.clip(ang[i] + 0.1 * rng.standard_normal(7), bounds[:, 0], bounds[:, 1])
            r, J = numpy_model(q, targets_of(pose[i], np.ones(4)), np.ones(4), seg)
            normal[t] = (J.T @ J, J.T @ r)
        while len(_BLOCK_FRAMES) >= 4:
            _BLOCK_FRAMES.pop(next(iter(_BLOCK_FRAMES)))
        _BLOCK_FRAMES[(N, seed, cut, hold)] = (seg, bad, held, pair, normal)
    return _BLOCK_FRAMES[(N, seed, cut, hold)]


def block_rows(N, seed, smooth=SMOOTH, lam=1e-3, cut=0.1, hold=0.15):
    """A block-tridiagonal system as step 4 builds it, N rows: D from the real normal equations of made-up leg-frames
    (J^T J of refine_support.numpy_model at their seeds, plus the penalty, plus lambda diag), random held masks (a DOF
    with probability `hold`), some broken pairs and some identity rows (bad frames; each with probability `cut`)
    -> D, L, U (N, 7, 7), b (N, 7).  With the defaults a run of coupled frames is about five frames long, so the far
    strides of the reduction meet blocks of zeros; cut = hold = 0 couples all N frames."""
    seg, bad, held, pair, normal = _block_frames(N, seed, cut, hold)
    s = stiffness(smooth, seg)
    D, L, U, b = np.zeros((N, 7, 7)), np.zeros((N, 7, 7)), np.zeros((N, 7, 7)), np.zeros((N, 7))
    for t in range(N):
        if bad[t]:
            D[t] = np.eye(7)
            continue
        A, g = normal[t]
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


# ------------------------------------- the linear solve: LAPACK and an extended-precision truth -------------------------------------

def banded_lower(D, L):
    """The block-tridiagonal matrix of D (lower triangles) and L in LAPACK's lower banded storage (14, 7 N): entry (r, c),
    r >= c, at [r - c, c].  The matrix is symmetric (U_{t-1} = L_t^T), so U is not needed."""
    N = len(D)
    Ds, ab = sym_lower_all(D), np.zeros((14, 7 * N))
    for i in range(7):
        for j in range(7):
            if i >= j:
                ab[i - j, j::7] = Ds[:, i, j]
            ab[7 + i - j, j:7 * (N - 1):7] = L[1:, i, j]
    return ab


def block_matvec(D, L, U, x, dtype):
    """The block-tridiagonal matrix times x (N, 7), every product and sum in `dtype`."""
    Ds, x = sym_lower_all(D).astype(dtype), x.astype(dtype)
    y = np.einsum("tij,tj->ti", Ds, x)
    y[1:] += np.einsum("tij,tj->ti", L[1:].astype(dtype), x[:-1])
    y[:-1] += np.einsum("tij,tj->ti", U[:-1].astype(dtype), x[1:])
    return y


def lapack_and_truth(D, L, U, b, sweeps=20):
    """LAPACK's banded Cholesky solve (scipy.linalg.solveh_banded, float64) of the system, and that solution refined --
    residual b - M x in numpy.longdouble (64-bit mantissa), correction by the same float64 solve, x kept in longdouble
    -- until the correction stops shrinking -> (x_lapack (N, 7) float64, truth (N, 7) longdouble, the last correction's
    size relative to max |x|)."""
    from scipy.linalg import solveh_banded
    LD = np.longdouble
    assert np.finfo(LD).eps < 2e-19 and np.array_equal(U[:-1], L[1:].transpose(0, 2, 1))
    ab = banded_lower(D, L)
    x0 = solveh_banded(ab, b.reshape(-1), lower=True).reshape(-1, 7)
    x, last = x0.astype(LD), np.inf
    for _ in range(sweeps):
        r = b.astype(LD) - block_matvec(D, L, U, x, LD)
        dx = solveh_banded(ab, np.asarray(r, dtype=np.float64).reshape(-1), lower=True).reshape(-1, 7)
        size = float(np.abs(dx).max())
        if not size < 0.5 * last:
            break
        x, last = x + dx.astype(LD), size
    scale = float(np.abs(x).max())
    return x0, x, last / scale if scale > 0 else 0.0           # (an all-identity system: x = 0 exactly)


def mp_block_solve(D, L, U, b):
    """The system by block elimination at 200 bits (mpmath): S_0 = D_0, S_t = D_t - L_t S_{t-1}^-1 U_{t-1}, and back
    -> (N, 7) longdouble of the exact values.  For small N: the yardstick of the yardstick."""
    from test_fk_accuracy import _MP as mp
    N = len(D)
    mat = lambda a: mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.atleast_2d(a)])  # noqa: E731
    Ds = sym_lower_all(D)
    S, y = [mat(Ds[0])], [mat(b[0]).T]
    for t in range(1, N):
        Lt, Ut, X = mat(L[t]), mat(U[t - 1]), mp.matrix(7, 7)
        for c in range(7):                          # (lu_solve takes one right-hand side)
            X[:, c] = mp.lu_solve(S[t - 1], Ut[:, c])
        S.append(mat(Ds[t]) - Lt * X)
        y.append(mat(b[t]).T - Lt * mp.lu_solve(S[t - 1], y[t - 1]))
    x = [None] * N
    x[N - 1] = mp.lu_solve(S[N - 1], y[N - 1])
    for t in range(N - 2, -1, -1):
        x[t] = mp.lu_solve(S[t], y[t] - mat(U[t]) * x[t + 1])
    hi = np.array([[float(x[t][i]) for i in range(7)] for t in range(N)])
    lo = np.array([[float(x[t][i] - mp.mpf(hi[t, i])) for i in range(7)] for t in range(N)])
    return hi.astype(np.longdouble) + lo.astype(np.longdouble)


# ------------------------------------------------- 200-bit yardstick -------------------------------------------------

def mp_parts(q, pose, seg, smooth, weight=None, bad=None):
    """C(Q) and its full gradient (half the derivative, as the rule keeps it) of one trajectory at 200 bits: the data term
    on refine_support.mp_gradient and tests/test_fk_accuracy.mp_chain, with weights, plus the penalty over the existing
    pairs with s_j = smooth[j] len^2; bad frames are out of both -> (C float64 of the exact value, g (N, 7) likewise)."""
    from refine_support import mp_gradient
    from sensitivity_support import KEY_LINKS
    from test_fk_accuracy import _MP as mp, mp_chain
    mpf = mp.mpf
    N = len(q)
    w = np.ones((N, 4)) if weight is None else np.broadcast_to(weight, (N, 4))
    bad = np.zeros(N, dtype=bool) if bad is None else bad
    length = sum(mpf(float(v)) for v in seg)
    s = [mpf(float(v)) * length * length for v in smooth7(smooth)]
    Q = [[mpf(float(v)) for v in row] for row in q]
    C, g = mpf(0), np.zeros((N, 7))
    for t in range(N):
        if bad[t]:
            continue
        fr = mp_chain(0, q[t], seg, np.zeros((5, 3)))[0]
        for k in range(4):
            if w[t, k] == 0:
                continue
            for c in range(3):
                f = mpf(float(fr[0, KEY_LINKS[k], c, 3])) + mpf(float(fr[1, KEY_LINKS[k], c, 3]))
                r = mpf(float(w[t, k])) * (f - (mpf(float(pose[t, k + 1, c])) - mpf(float(pose[t, 0, c]))))
                C += r * r
        gt = [mpf(float(v)) for v in mp_gradient(q[t], np.where(np.isfinite(pose[t]), pose[t], 0.0), seg, w[t])]
        for u in (t - 1, t + 1):
            if 0 <= u < N and not bad[u]:
                for j in range(7):
                    gt[j] += s[j] * (Q[t][j] - Q[u][j])
        if t > 0 and not bad[t - 1]:
            for j in range(7):
                C += s[j] * (Q[t][j] - Q[t - 1][j]) ** 2
        g[t] = [float(v) for v in gt]
    return float(C), g


# ---------------------------------------------------- real scipy ----------------------------------------------------

def _scipy_run(angles, pose, seg, bounds, smooth, w):
    """One run of good frames: see scipy_smooth."""
    from scipy.optimize import least_squares
    N = len(angles)
    lb, ub = np.asarray(bounds)[:, 0], np.asarray(bounds)[:, 1]
    rs = np.sqrt(stiffness(smooth, seg))
    t = [targets_of(pose[i], w[i]) for i in range(N)]

    def res(x):
        q = x.reshape(N, 7)
        data = [numpy_model(q[i], t[i], w[i], seg)[0] for i in range(N)]
        return np.concatenate(data + [(rs * np.diff(q, axis=0)).ravel()])

    def jac(x):
        q = x.reshape(N, 7)
        J = np.zeros((12 * N + 7 * (N - 1), 7 * N))
        for i in range(N):
            J[12 * i:12 * i + 12, 7 * i:7 * i + 7] = numpy_model(q[i], t[i], w[i], seg)[1]
        for i in range(N - 1):
            row = 12 * N + 7 * i
            J[row:row + 7, 7 * i:7 * i + 7] = -np.diag(rs)
            J[row:row + 7, 7 * i + 7:7 * i + 14] = np.diag(rs)
        return J

    sol = least_squares(res, np.clip(angles, lb, ub).ravel(), jac=jac, bounds=(np.tile(lb, N), np.tile(ub, N)), method="trf",
                        xtol=1e-14, ftol=1e-14, gtol=1e-12, max_nfev=5000)
    return sol.x.reshape(N, 7), 2.0 * sol.cost


def scipy_smooth(angles, pose, seg, bounds, smooth=SMOOTH, weight=None):
    """scipy.optimize.least_squares (TRF, bounds, analytic Jacobian, xtol = ftol = 1e-14, gtol = 1e-12) on the stacked
    residuals of one trajectory -- the 12 data residuals of every frame, each key point's scaled by its weight as
    refine_support.numpy_model scales them, then sqrt(s_j) times the differences of neighbouring frames -- from the clamped
    start.  Bad frames (numpy_bad) cut the coupling, so the runs of good frames between them are solved one by one and
    their costs added; a bad frame's angles are NaN -> (angles (N, 7), C there: twice scipy's cost)."""
    N = len(angles)
    w = np.ones((N, 4)) if weight is None else np.broadcast_to(weight, (N, 4))
    bad = numpy_bad(angles, pose, weight)
    x, C, t = np.full((N, 7), np.nan), 0.0, 0
    while t < N:
        if bad[t]:
            t += 1
            continue
        end = t
        while end < N and not bad[end]:
            end += 1
        x[t:end], c = _scipy_run(angles[t:end], pose[t:end], seg, bounds, smooth, w[t:end])
        C, t = C + c, end
    return x, C


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
