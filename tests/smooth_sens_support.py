"""TEST INFRASTRUCTURE -- what the tests of the smoothed trajectory's error bars (include/seqik_smooth_sensitivity.h)
share: the host harness (csrc/seqik_smooth_sens.hpp compiled for the host), the dense float64 numpy statement of the linear
part (one 7 N x 7 N matrix, np.linalg.inv), a float64 numpy restatement of the sweeps and the same recursions at 200 bits
(mpmath) that set the bar of the linear test, made-up block systems, and a stand-in for ``_lib._call``.  Nothing here is
taken from csrc."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import ROOT, LegParamsC
from harness_build import build_harness
from smooth_support import legs_array, shipped_window, smooth7

BAD_INPUT, NOT_PD, BAD_SIGMA = 1 << 16, 1 << 8, 1 << 17
IDENTITY_ROW = 1 << 24      # the word bit of the linear harness: an identity row that cuts the coupling
TOL = 1e-6
EPS = np.finfo(float).eps
PROFILE = os.path.join(ROOT, "profiles", "smooth_sensitivity_accuracy.json")


def record(key, value):
    """Keeps a measured value in profiles/smooth_sensitivity_accuracy.json when SEQIK_RECORD_PROFILES is set (the
    committed file is the record of one such run; a plain test run writes nothing)."""
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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class SmoothSensHarness:
    def __init__(self, so):
        dp, ip, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(LegParamsC)
        self.lib = ctypes.CDLL(so)
        self.lib.harness_smooth_sensitivity.restype = ctypes.c_int
        self.lib.harness_smooth_sensitivity.argtypes = [dp, dp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, lp, dp, dp, dp,
                                                        ctypes.c_double, ctypes.c_int32, dp, dp, dp, ip]
        self.lib.harness_smooth_sens_linear.restype = ctypes.c_int
        self.lib.harness_smooth_sens_linear.argtypes = [dp, ip, ctypes.c_int64, dp, dp, dp, ctypes.c_int32, dp, dp, ip]

    def run(self, angles, pose, segs, bounds, smooth=0.1, weight=None, kp_sigma=None, half_width=0, tol=TOL,
            want=("sens", "grad", "flags")):
        """(S, L, N, 7), (S, L, N, 5, 3), L segment sets and limits [, weights and sigmas that broadcast to (S, L, N, 4)]
        -> dict(sens (S, L, N, 2 W + 1, 7, 4, 3), std (S, L, N, 7), grad (S, L, N), flags (S, L, N) int32), None for what
        is not in ``want`` (std is wanted whenever kp_sigma is given)."""
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        angles, pose = np.ascontiguousarray(angles, dtype=np.float64), np.ascontiguousarray(pose, dtype=np.float64)
        S, L, N = angles.shape[:3]
        assert angles.shape == (S, L, N, 7) and pose.shape == (S, L, N, 5, 3) and len(segs) == len(bounds) == L
        bc = lambda v: None if v is None else np.ascontiguousarray(np.broadcast_to(v, (S, L, N, 4)), dtype=np.float64)  # noqa: E731
        w, sig = bc(weight), bc(kp_sigma)
        W = int(half_width)
        out = dict(sens=np.full((S, L, N, 2 * W + 1, 7, 4, 3), 7.0) if "sens" in want else None,
                   std=np.full((S, L, N, 7), 7.0) if sig is not None else None,
                   grad=np.full((S, L, N), 7.0) if "grad" in want else None,
                   flags=np.full((S, L, N), -1, dtype=np.int32) if "flags" in want else None)
        ptr = lambda a: a.ctypes.data_as(dp) if a is not None else None  # noqa: E731
        rc = self.lib.harness_smooth_sensitivity(ptr(angles), ptr(pose), S, L, N, legs_array(segs, bounds), ptr(w), ptr(sig),
                                                 ptr(smooth7(smooth)), tol, W, ptr(out["sens"]), ptr(out["std"]),
                                                 ptr(out["grad"]),
                                                 out["flags"].ctypes.data_as(ip) if out["flags"] is not None else None)
        assert rc == 0
        return out

    def run_one(self, angles, pose, seg, bounds, **kw):
        """One trajectory: (N, 7), (N, 5, 3) -> the same dictionary without the leading (1, 1)."""
        n = len(angles)
        for k in ("weight", "kp_sigma"):
            if kw.get(k) is not None:
                kw[k] = np.broadcast_to(kw[k], (n, 4))[None, None]
        res = self.run(np.asarray(angles)[None, None], np.asarray(pose)[None, None], [seg], [bounds], **kw)
        return {k: (None if v is None else v[0, 0]) for k, v in res.items()}

    def linear(self, H, word, s, B, sigma, half_width):
        """The linear part on caller-given blocks: H (N, 7, 7), word (N,) (bits 0..6 held, IDENTITY_ROW), s (7,), B (N, 7,
        12), sigma (N, 4) -> sens (N, 2 W + 1, 7, 12), std (N, 7), flags (N,)"""
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        N, W = len(H), int(half_width)
        H, B = np.ascontiguousarray(H, dtype=np.float64), np.ascontiguousarray(B, dtype=np.float64)
        sigma, s = np.ascontiguousarray(sigma, dtype=np.float64), np.ascontiguousarray(s, dtype=np.float64)
        word = np.ascontiguousarray(word, dtype=np.int32)
        assert H.shape == (N, 7, 7) and B.shape == (N, 7, 12) and sigma.shape == (N, 4) and s.shape == (7,)
        sens, std, flags = np.full((N, 2 * W + 1, 7, 12), 7.0), np.full((N, 7), 7.0), np.full(N, -1, dtype=np.int32)
        rc = self.lib.harness_smooth_sens_linear(H.ctypes.data_as(dp), word.ctypes.data_as(ip), N, s.ctypes.data_as(dp),
                                                 B.ctypes.data_as(dp), sigma.ctypes.data_as(dp), W, sens.ctypes.data_as(dp),
                                                 std.ctypes.data_as(dp), flags.ctypes.data_as(ip))
        assert rc == 0
        return sens, std, flags


@pytest.fixture(scope="session")
def smooth_sens_harness():
    # (torch first where there is one: refine_support.refine_harness says why)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    return SmoothSensHarness(build_harness(os.path.join(ROOT, "tests", "harness", "smooth_sens_harness.hip")))


# ------------------------------------------------- the linear part -------------------------------------------------

def masked_blocks(H, word, s):
    """The blocks the definition names, from raw ones: H_tt with the rows and columns of held DOFs replaced by the
    identity's (an identity row: the identity), k (N, 7) with k[t] the diagonal of K_t (k[0] = 0) -> Hm (N, 7, 7), k, free
    (N, 7), identity (N,).  Works on float64 and on object (mpmath) arrays."""
    H, s = np.asarray(H), np.asarray(s)
    N = len(H)
    ident = (np.asarray(word) & IDENTITY_ROW) != 0
    held = ((np.asarray(word)[:, None] >> np.arange(7)) & 1).astype(bool)
    free = ~held & ~ident[:, None]
    Hm, k = np.zeros((N, 7, 7), dtype=H.dtype), np.zeros((N, 7), dtype=s.dtype)
    for t in range(N):
        sym = np.tril(H[t]) + np.tril(H[t], -1).T
        Hm[t] = np.where(np.outer(free[t], free[t]), sym, 0) + np.diag(np.where(free[t], 0, 1))
        if t > 0 and not ident[t] and not ident[t - 1]:
            k[t] = np.where(free[t] & free[t - 1], s, 0)
    return Hm, k, free, ident


def dense_matrix(Hm, k):
    N = len(Hm)
    A = np.zeros((7 * N, 7 * N), dtype=Hm.dtype)
    for t in range(N):
        A[7 * t:7 * t + 7, 7 * t:7 * t + 7] = Hm[t]
        if t > 0:
            A[7 * t:7 * t + 7, 7 * t - 7:7 * t] = A[7 * t - 7:7 * t, 7 * t:7 * t + 7] = -np.diag(k[t])
    return A


def _dense_outputs(G, Bm, sig2, N):
    GB = np.zeros((N, N, 7, 12), dtype=G.dtype)
    var = np.zeros((N, 7), dtype=G.dtype)
    for t in range(N):
        for u in range(N):
            GB[t, u] = G[7 * t:7 * t + 7, 7 * u:7 * u + 7] @ Bm[u]
            var[t] += np.sum(GB[t, u] ** 2 * sig2[u], axis=1)
    return GB, var


def dense_linear(H, word, s, B, sigma):
    """The definition as one dense matrix: inv(H) B per block and the diagonal of inv(H) M inv(H), M = B diag(sigma^2) B^T
    -> G B (N, N, 7, 12) [t, source], var (N, 7), positive definite (bool).  The matrix is kept in
    ``dense_linear.last_matrix``."""
    Hm, k, free, ident = masked_blocks(H, word, s)
    A = dense_matrix(Hm, k)
    dense_linear.last_matrix = A
    pd = bool(np.all(np.linalg.eigvalsh(A) > 0))
    GB, var = _dense_outputs(np.linalg.inv(A), np.where(free[:, :, None], B, 0.0),
                             np.repeat(np.asarray(sigma) ** 2, 3, axis=1), len(H))
    return GB, var, pd


def dense_mp(H, word, s, B, sigma, W, bits_=200):
    """The same at 200 bits (mpmath's dense inverse; small N only) -> sens (N, 2 W + 1, 7, 12), var (N, 7) of mpf"""
    import mpmath
    with mpmath.workprec(bits_):
        Hm, k, free, ident = masked_blocks(_MpOps.arr(H), word, _MpOps.arr(s))
        A = dense_matrix(Hm, k)
        G = np.array((mpmath.matrix(A.tolist()) ** -1).tolist(), dtype=object)
        sig2 = _MpOps.arr(np.repeat(np.asarray(sigma, dtype=float), 3, axis=1)) ** 2
        GB, var = _dense_outputs(G, np.where(free[:, :, None], _MpOps.arr(B), 0), sig2, len(H))
        out = np.zeros((len(H), 2 * W + 1, 7, 12), dtype=object)
        for t in range(len(H)):
            for d in range(2 * W + 1):
                if 0 <= t + d - W < len(H):
                    out[t, d] = GB[t, t + d - W]
        return out, var


def sweeps_numpy(H, word, s, B, sigma, half_width):
    """The recursions of the header in plain float64 numpy (np.linalg.solve, @ products): Sf / Sb, Pf / Pb, the combine,
    the off-centre products and Lam / Ups -> sens (N, 2 W + 1, 7, 12), var (N, 7).  The reference arithmetic that sets
    the bar of the accuracy tests, not the code under test."""
    return _sweeps(H, word, s, B, sigma, half_width, _NumpyOps)[:2]


def _to_float(a):
    return np.array([float(x) for x in a.ravel()]).reshape(a.shape)


def sweeps_mp(H, word, s, B, sigma, half_width, bits_=200, as_float=True, verdicts=False):
    """The same recursions at 200 bits -> sens, var (float64 roundings of the 200-bit values, or the mpf themselves)
    [, poisoned (N,) bool, robust: no pivot of any factorisation within 2^-40 of zero relative to the largest]."""
    import mpmath
    with mpmath.workprec(bits_):
        sens, var, poisoned, robust = _sweeps(H, word, s, B, sigma, half_width, _MpOps)
        if as_float:
            sens, var = _to_float(sens), _to_float(var)
        return (sens, var, poisoned, robust) if verdicts else (sens, var)


class _NumpyOps:
    @staticmethod
    def arr(a):
        return np.array(a, dtype=float)

    @staticmethod
    def solve(S, X):
        try:
            return np.linalg.solve(S, X)
        except np.linalg.LinAlgError:      # singular: the 200-bit verdict skips such a trajectory
            return np.full(np.shape(X), np.nan)

    @staticmethod
    def pivots(S):
        return None


class _MpOps:
    @staticmethod
    def arr(a):
        import mpmath
        a = np.asarray(a)
        if a.dtype != object:
            a = a.astype(float)
        return np.vectorize(lambda v: mpmath.mpf(v), otypes=[object])(a)

    @staticmethod
    def solve(S, X):
        import mpmath
        try:
            inv = np.array((mpmath.matrix(S.tolist()) ** -1).tolist(), dtype=object)      # (lu_solve takes one vector)
        except ZeroDivisionError:      # singular: a pivot is 0, which `pivots` reports as not robust
            return np.full(X.shape, mpmath.nan, dtype=object)
        return inv @ X

    @staticmethod
    def pivots(S):
        """The pivots of the LDL^T factorisation in the rule's order: all positive <=> positive definite"""
        import mpmath
        L, piv = [[mpmath.mpf(0)] * 7 for _ in range(7)], []
        for j in range(7):
            d = S[j][j] - sum(L[j][k] ** 2 * piv[k] for k in range(j))
            piv.append(d)
            for i in range(j + 1, 7):
                L[i][j] = (S[i][j] - sum(L[i][k] * L[j][k] * piv[k] for k in range(j))) / d if d != 0 else mpmath.mpf(0)
        return piv


ROBUST = 2.0 ** -40


def _sweeps(H, word, s, B, sigma, W, ops):
    Hm, k, free, ident = masked_blocks(ops.arr(H), word, ops.arr(s))
    N = len(Hm)
    kk = k
    Bm = np.where(free[:, :, None], ops.arr(B), 0)
    sig2 = ops.arr(np.repeat(np.asarray(sigma, dtype=float), 3, axis=1)) ** 2
    zero = ops.arr(np.zeros((7, 7)))
    coupled = [t > 0 and bool(np.any(k[t] != 0)) for t in range(N)] + [False]
    Pf, Pb, Sf, Sb = [zero] * N, [zero] * N, [None] * N, [None] * N
    fail = np.zeros((3, N), dtype=bool)
    robust = True

    def verdict(which, t, S):
        nonlocal robust
        piv = ops.pivots(S)
        if piv is not None and not ident[t]:
            fail[which, t] = any(p <= 0 for p in piv)
            if min(abs(p) for p in piv) <= ROBUST * max(abs(p) for p in piv):
                robust = False

    for t in range(N):
        Sf[t] = Hm[t] - (kk[t][:, None] * Pf[t - 1] if coupled[t] else zero)
        verdict(0, t, Sf[t])
        if coupled[t + 1]:
            Pf[t] = ops.solve(Sf[t], np.diag(kk[t + 1]) + zero)
    for t in range(N - 1, -1, -1):
        Sb[t] = Hm[t] - (kk[t + 1][:, None] * Pb[t + 1] if coupled[t + 1] else zero)
        verdict(1, t, Sb[t])
        if coupled[t]:
            Pb[t] = ops.solve(Sb[t], np.diag(kk[t]) + zero)
    sens0 = []
    for t in range(N):
        T = Sf[t] + Sb[t] - Hm[t]
        verdict(2, t, T)
        sens0.append(ops.solve(T, Bm[t]))
    # poisoning: forward from an Sf failure, backward from an Sb failure, inside the coupled run
    poisoned = fail[2].copy()
    p = False
    for t in range(N):
        p = (p and coupled[t]) or fail[0, t]
        poisoned[t] |= p
    p = False
    for t in range(N - 1, -1, -1):
        p = (p and coupled[t + 1]) or fail[1, t]
        poisoned[t] |= p
    Wt = [(sens0[t] * sig2[t]) @ sens0[t].T for t in range(N)]
    sens = ops.arr(np.zeros((N, 2 * W + 1, 7, 12)))
    for t in range(N):
        sens[t, W] = sens0[t]
        Q = None
        for m in range(1, W + 1):                      # sources t - m
            u = t - m
            if u < 0 or not coupled[u + 1]:
                break
            Q = Pb[u + 1] if Q is None else Q @ Pb[u + 1]
            sens[t, W - m] = Q @ sens0[u]
        Q = None
        for m in range(1, W + 1):                      # sources t + m
            u = t + m
            if u >= N or not coupled[u]:
                break
            Q = Pf[u - 1] if Q is None else Q @ Pf[u - 1]
            sens[t, W + m] = Q @ sens0[u]
    Lam, Ups = [zero] * N, [zero] * N
    for t in range(1, N):
        if coupled[t]:
            Lam[t] = Pb[t] @ (Lam[t - 1] + Wt[t - 1]) @ Pb[t].T
    for t in range(N - 2, -1, -1):
        if coupled[t + 1]:
            Ups[t] = Pf[t] @ (Ups[t + 1] + Wt[t + 1]) @ Pf[t].T
    var = np.stack([np.diag(Wt[t]) + (np.diag(Lam[t]) + np.diag(Ups[t])) for t in range(N)])
    return sens, var, poisoned, robust


def banded(GB, W):
    """(N, N, 7, 12) [t, source] -> the layout of sens: (N, 2 W + 1, 7, 12), blocks outside 0..N-1 zero"""
    N = len(GB)
    out = np.zeros((N, 2 * W + 1, 7, 12))
    for t in range(N):
        for d in range(2 * W + 1):
            u = t + d - W
            if 0 <= u < N:
                out[t, d] = GB[t, u]
    return out


def random_system(N, seed, held_rate=0.15, ident_rate=0.1, zero_s_rate=0.2):
    """A random symmetric positive definite block-tridiagonal system in the form of the definition, with held masks,
    broken pairs (a DOF held on either side breaks its entry; an all-held frame breaks the pair) and identity rows ->
    H (N, 7, 7), word (N,), s (7,), B (N, 7, 12), sigma (N, 4).  H_tt = A A^T + 0.5 I + (the s of both pairs): the whole
    matrix is the sum of positive definite data blocks and the positive semidefinite penalty."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.5, 20.0, 7) * (rng.random(7) >= zero_s_rate)
    ident = rng.random(N) < ident_rate
    held = rng.random((N, 7)) < held_rate
    if N > 4:
        held[rng.integers(N)] = True                 # one frame with no free DOF
    word = (held * (1 << np.arange(7))).sum(1).astype(np.int32) | np.where(ident, IDENTITY_ROW, 0).astype(np.int32)
    H = np.zeros((N, 7, 7))
    for t in range(N):
        A = rng.standard_normal((7, 7))
        H[t] = A @ A.T + 0.5 * np.eye(7)
        for u in (t - 1, t + 1):
            if 0 <= u < N and not ident[u]:
                H[t] += np.diag(s)
    B = rng.standard_normal((N, 7, 12))
    B[:, :, :7] = np.eye(7)                           # the first seven columns of a block of sens are G_ts itself
    sigma = rng.uniform(0.0, 2.0, (N, 4))
    return H, word, s, B, sigma


# ------------------------------------- the library call answered by the host harness -------------------------------------

def harness_call(ssh, real_call):
    """A stand-in for ``_lib._call`` that answers ``seqik_smooth_sensitivity`` with the host-run rule: what the CPU tier can
    run of the Python surface (the product itself has no CPU path)."""
    def call(name, *args):
        if name == "seqik_smooth_sensitivity":
            (angles, pose, S, L, N, legs, kind, weight, sigma, smooth, tol, W, sens, std, grad, flags, device) = args
            assert kind == 0
            rc = ssh.lib.harness_smooth_sensitivity(angles, pose, S, L, N, ctypes.cast(legs, ctypes.POINTER(LegParamsC)),
                                                    weight, sigma, ctypes.cast(smooth, ctypes.POINTER(ctypes.c_double)), tol,
                                                    W, sens, std, grad, flags)
            assert rc == 0
            return None
        return real_call(name, *args)
    return call


# ------------------------------------------------------- inputs -------------------------------------------------------

_SMOOTHED = {}


def smoothed_window(smh, leg, lo, hi, smooth=0.1):
    """Frames lo:hi of a leg of the shipped recording, smoothed once by the host-run rule of seqik_smooth.h at ``smooth``
    -> the smoothed angles (n, 7), pose (n, 5, 3), seg, bounds (copies)"""
    key = (leg, lo, hi, smooth)
    if key not in _SMOOTHED:
        ang, pose, seg, bounds = shipped_window(leg, lo, hi)
        _SMOOTHED[key] = (smh.run_one(ang, pose, seg, bounds, smooth=smooth)["angles"], pose, seg, bounds)
    q, pose, seg, bounds = _SMOOTHED[key]
    return q.copy(), pose.copy(), seg, bounds


# ------------------------------------------- the whole rule at 200 bits -------------------------------------------

def _mp_frame(q, pose, seg, w):
    """One leg-frame at 200 bits on mp_chain: the exact data Hessian H (7 x 7), g, the magnitudes summed into g (gs) and
    B (7, 12) = w_k (w_k J_k)^T, as object arrays of mpf (the frame of test_fk_accuracy.mp_chain, the sums of
    refine_sens_support.mp_rule)."""
    from refine_sens_support import DOF_LINK, KEY_LINKS, NONZERO, _mp_cross, _mp_dot
    from test_fk_accuracy import _MP, mp_chain
    mpf = _MP.mpf
    fr = mp_chain(0, q, seg, np.zeros((5, 3)))[0]
    Fm = [[[mpf(float(fr[0, i, r, c])) + mpf(float(fr[1, i, r, c])) for c in range(4)] for r in range(3)] for i in range(9)]
    axis = [[Fm[l][r][c] for r in range(3)] for l, c in DOF_LINK]
    org = [[Fm[l][r][3] for r in range(3)] for l, _ in DOF_LINK]
    P = [[mpf(float(v)) if np.isfinite(v) else mpf(0) for v in row] for row in pose]
    H = np.full((7, 7), mpf(0), dtype=object)
    g, gs, B = np.full(7, mpf(0), dtype=object), np.full(7, mpf(0), dtype=object), np.full((7, 12), mpf(0), dtype=object)
    norm = lambda v: _MP.sqrt(_mp_dot(v, v))  # noqa: E731
    for k in range(4):
        wk = mpf(float(w[k]))
        if wk == 0:
            continue
        f = [Fm[KEY_LINKS[k]][r][3] for r in range(3)]
        res = [wk * (f[c] - (P[k + 1][c] - P[0][c])) for c in range(3)]
        J = [None] * 7
        for d in range(7):
            if NONZERO[k, d]:
                J[d] = [wk * v for v in _mp_cross(axis[d], [f[c] - org[d][c] for c in range(3)])]
                g[d] += _mp_dot(J[d], res)
                gs[d] += norm(J[d]) * norm(res)
                for c in range(3):
                    B[d, 3 * k + c] = wk * J[d][c]
        for a in range(7):
            for b in range(a, 7):
                if NONZERO[k, a] and NONZERO[k, b]:
                    h = _mp_dot(J[a], J[b]) + _mp_dot(res, _mp_cross(axis[a], J[b]))
                    H[a, b] += h
                    if b != a:
                        H[b, a] += h
    return H, g, gs, B


def mp_trajectory(q, pose, seg, bounds, smooth, weight, W, sigma, tol=TOL):
    """One trajectory at 200 bits: the blocks of the definition from ``_mp_frame`` and the penalty, the held verdicts, the
    sweeps (``_sweeps`` with mpmath) -> dict(bad (N,), flags (N,) int32 (held bits and NOT_PD; 0 for bad frames), grad,
    grad_scale (N,), sens (N, 2 W + 1, 7, 12), var (N, 7): float64 roundings of the 200-bit values, sens_numpy, var_numpy: the
    float64 numpy restatement of the same recursions on float64 blocks (refine_sens_support.numpy_rule), robust: False
    when a held verdict or a pivot could flip under rounding (7p's two criteria, the pivots being those of every Sf, Sb and
    combined block))."""
    import mpmath
    from refine_sens_support import numpy_rule
    from smooth_support import numpy_bad
    from test_fk_accuracy import _MP
    N = len(q)
    w = np.ones((N, 4)) if weight is None else np.broadcast_to(weight, (N, 4))
    bad = numpy_bad(q, pose, w)
    with mpmath.workprec(200):
        mpf = _MP.mpf
        len2 = sum(mpf(float(v)) for v in seg) ** 2
        s = np.array([mpf(float(v)) * len2 for v in smooth7(smooth)], dtype=object)
        eye = np.array([[mpf(int(i == j)) for j in range(7)] for i in range(7)], dtype=object)
        H = np.stack([eye] * N)
        B = np.full((N, 7, 12), mpf(0), dtype=object)
        word = np.where(bad, IDENTITY_ROW, 0).astype(np.int32)
        grad, grad_scale, robust = np.full(N, np.nan), np.full(N, np.nan), True
        Hn, Bn = np.stack([np.eye(7)] * N), np.zeros((N, 7, 12))          # the float64 restatement's blocks
        s64 = smooth7(smooth) * np.sum(seg) ** 2
        for t in np.where(~bad)[0]:
            Ht, g, gs, B[t] = _mp_frame(q[t], pose[t], seg, w[t])
            nr = numpy_rule(q[t], np.where(np.isfinite(pose[t]), pose[t], 0.0), seg, bounds, w[t], tol)
            Hn[t] = nr["H"]
            for u in (t - 1, t + 1):
                if 0 <= u < N and not bad[u]:
                    d = np.array([mpf(float(q[t, j])) - mpf(float(q[u, j])) for j in range(7)], dtype=object)
                    g = g + s * d
                    gs = gs + np.array([abs(v) for v in s * d], dtype=object)
                    Ht = Ht + np.diag(s)
                    Hn[t] = Hn[t] + np.diag(s64)
            H[t] = Ht
            free = []
            for a in range(7):
                at_lb = mpf(float(q[t, a])) - mpf(float(bounds[a][0])) <= mpf(tol)
                at_ub = mpf(float(bounds[a][1])) - mpf(float(q[t, a])) <= mpf(tol)
                if (at_lb or at_ub) and abs(g[a]) <= mpf(ROBUST) * gs[a]:
                    robust = False
                if (at_lb and g[a] > 0) or (at_ub and g[a] < 0):
                    word[t] |= 1 << a
                else:
                    free.append(a)
            grad[t] = float(max([abs(g[a]) for a in free], default=mpf(0)) / len2)
            grad_scale[t] = float(max(gs) / len2)
            Bn[t] = _numpy_B(q[t], np.where(np.isfinite(pose[t]), pose[t], 0.0), seg, w[t])
        sig = np.full((N, 4), float(sigma))
        sens, var, poisoned, rob = _sweeps(H, word, s, B, sig, W, _MpOps)
        robust = robust and rob
        sens, var = _to_float(sens), _to_float(var)
    sens_np, var_np = sweeps_numpy(Hn, word, s64, Bn, sig, W)
    flags = (word & 0x7F) | np.where(poisoned & ~bad, NOT_PD, 0).astype(np.int32)
    return dict(bad=bad, flags=flags.astype(np.int32), grad=grad, grad_scale=grad_scale, sens=sens, var=var, sens_numpy=sens_np,
                var_numpy=var_np, robust=robust)


def _numpy_B(q, pose, seg, w):
    """B (7, 12) = w_k (w_k J_k)^T in float64 numpy (the Jacobian of refine_support.numpy_model carries one w_k)."""
    from refine_support import numpy_model, targets_of
    _, J = numpy_model(q, targets_of(pose, w), w, seg)                # (12, 7), rows 3 k + c
    return (J * np.repeat(w, 3)[:, None]).T


def fd_polish(smh, ssh, ang, pose, seg, bounds, smooth=0.1, cap=25):
    """The host-run trajectory fit, then again and again from its own result with gtol = ftol = 0 until the largest
    reported grad stops falling -> the angles, the grad reached, the polishing calls made."""
    q = smh.run_one(ang, pose, seg, bounds, smooth=smooth)["angles"]
    best = float(ssh.run_one(q, pose, seg, bounds, smooth=smooth, want=("grad",))["grad"].max())
    for n in range(1, cap + 1):
        q2 = smh.run_one(q, pose, seg, bounds, smooth=smooth, max_iter=1000, gtol=0.0, ftol=0.0)["angles"]
        g2 = float(ssh.run_one(q2, pose, seg, bounds, smooth=smooth, want=("grad",))["grad"].max())
        if not g2 < best:
            return q, best, n
        q, best = q2, g2
    return q, best, cap


# ------------------------------------------------------ GPU tier ------------------------------------------------------

SENTINEL, SENTINEL_I = -12345.678, -1234567
SUBSETS = (("sens",), ("std",), ("flags", "grad"), ("sens", "std", "grad", "flags"))
GPU_FRAMES = (1, 2, 3, 63, 64, 65, 300)
GPU_WIDTHS = (0, 2)
GPU_S, GPU_L = 2, 3
GPU_SMOOTH = np.array([0.3, 0.05, 1.0, 0.02, 0.5, 2.0, 0.1])    # per DOF
GUARD = 256                                                      # bytes on each side of the workspace

_GPU_CASES = {}


def gpu_case(ssh, N, W, S=GPU_S):
    """Inputs (refine_sens_support.gpu_batch: angles inside made-up limits, some on one, weights, zero-weight NaN key
    points with NaN sigmas, a few bad leg-frames and a NaN sigma that is read; for N >= 3 a bad frame in the middle of the
    first trajectory) and the
    host-run rule's answers for them, computed once per shape: with std (the sigmas are read) and without."""
    from refine_sens_support import gpu_batch
    key = (N, W, S)
    if key not in _GPU_CASES:
        ang, pose, weight, sigma, segs, bounds = gpu_batch(900 + N, S, GPU_L, N)
        if N >= 3:
            ang[0, 0, N // 2, 2] = np.nan
        sigma[weight == 0.0] = np.nan                 # the sigma of a key point without weight is not read
        all3 = ("sens", "grad", "flags")
        kw = dict(smooth=GPU_SMOOTH, weight=weight, half_width=W, want=all3)
        _GPU_CASES[key] = dict(ang=ang, pose=pose, weight=weight, sigma=sigma, segs=segs, bounds=bounds, smooth=GPU_SMOOTH, W=W,
                               with_std=ssh.run(ang, pose, segs, bounds, kp_sigma=sigma, **kw),
                               no_std=ssh.run(ang, pose, segs, bounds, **kw))
    return _GPU_CASES[key]


def device_run(lib, c, want):
    """The device entry point on torch tensors with one guard record on each side of every output and GUARD bytes on each
    side of the workspace, all filled with a sentinel -> {name: (S, L, N, width)} of the outputs asked for; asserts that
    the guards and the outputs not asked for are untouched."""
    import torch
    S, L, N = c["ang"].shape[:3]
    n, W = S * L * N, c["W"]
    width = dict(sens=84 * (2 * W + 1), std=7, grad=1, flags=1)
    d_in = [torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("ang", "pose", "weight", "sigma")]
    bufs = {k: torch.full(((n + 2) * w,), SENTINEL_I if k == "flags" else SENTINEL,
                          dtype=torch.int32 if k == "flags" else torch.float64, device="cuda") for k, w in width.items()}
    ptr = {k: (bufs[k].data_ptr() + bufs[k].element_size() * width[k] if k in want else 0) for k in width}
    ws_bytes = lib.smooth_sensitivity_workspace_bytes(S, L, N, W)
    d_ws = torch.full((ws_bytes + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    params = [lib.leg_params_from_arrays(s, b, np.zeros(27)) for s, b in zip(c["segs"], c["bounds"])]
    lib.smooth_sensitivity_device(d_in[0].data_ptr(), d_in[1].data_ptr(), S, L, N, params, d_ws.data_ptr() + GUARD, ws_bytes,
                                  d_kp_weight=d_in[2].data_ptr(), d_kp_sigma=d_in[3].data_ptr(), d_sens=ptr["sens"],
                                  d_std=ptr["std"], d_grad=ptr["grad"], d_flags=ptr["flags"], smooth=c["smooth"], half_width=W,
                                  stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ws = d_ws.cpu().numpy()
    assert (ws[:GUARD] == 0x5A).all() and (ws[-GUARD:] == 0x5A).all(), ("workspace guard", want, N)
    out = {}
    for k, w in width.items():
        got, sent = bufs[k].cpu().numpy(), SENTINEL_I if k == "flags" else SENTINEL
        assert (got[:w] == sent).all() and (got[-w:] == sent).all(), (k, "guard", want, N)
        if k in want:
            out[k] = got[w:-w].reshape(S, L, N, w)
        else:
            assert (got == sent).all(), (k, "not requested", want, N)
    return out


def check_device_against_host(lib, c, want):
    S, L, N = c["ang"].shape[:3]
    got = device_run(lib, c, want)
    ref = c["with_std"] if "std" in want else c["no_std"]
    for k in want:
        if k == "flags":
            assert np.array_equal(got[k][..., 0], ref[k]), (k, N, c["W"], want)
        else:
            a, b = got[k].reshape(-1).view(np.uint64), np.ascontiguousarray(ref[k]).reshape(-1).view(np.uint64)
            assert np.array_equal(a, b), (k, N, c["W"], want, int((a != b).sum()))


if __name__ == "__main__":
    # The child process of the GPU tier's test of SEQIK_SMOOTHSENS_BLOCK / SEQIK_SMOOTHSENS_GRID: the environment is the
    # parent's plus the switches; the case (inputs and the host-run rule's answers) comes in an .npz.
    import sys
    from seqikpy_amd import _lib as hiplib
    case = np.load(sys.argv[1], allow_pickle=True)["case"].item()
    assert os.environ["SEQIK_SMOOTHSENS_BLOCK"] == "64" and os.environ["SEQIK_SMOOTHSENS_GRID"] == "1"
    for want in SUBSETS:
        check_device_against_host(hiplib, case, want)
    print("CHILD OK", case["ang"].shape)
