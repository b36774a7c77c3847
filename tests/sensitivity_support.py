"""TEST INFRASTRUCTURE -- what the tests of the key-point sensitivity (include/seqik_sensitivity.h) share: the host
harness (csrc/seqik_sensitivity.hpp compiled for the host), a float64 numpy restatement of the rule (np.cross,
np.linalg.solve; with switches for the two wrong rules the solver test measures) and the 200-bit yardstick on ``mp_chain``
of tests/test_fk_accuracy.py.  Nothing here is taken from csrc."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT, LegParamsC
from harness_build import build_harness
from test_fk_accuracy import _MP, mp_chain

KEY_LINKS = (4, 6, 7, 8)                                      # the links whose origins are key points 1..4
DOF_LINK = [(1, 0), (2, 1), (3, 2), (4, 1), (5, 2), (6, 1), (7, 1)]   # (link, axis column) of every DOF, sequential chain
STAGE_DOFS = [(0, 1), (2, 3), (4, 5), (6,)]
BAD_INPUT = 1 << 16
WIDE = np.array([[-10.0, 10.0]] * 7)                          # limits no test angle comes near


def structural_zero_mask():
    """(7, 4) bool: True where sens[d][k] is a structural zero (key point k + 1 lies after the DOF's stage)."""
    return np.array([[k > d // 2 for k in range(4)] for d in range(7)])


def leg_params(seg, bounds):
    lp = LegParamsC()
    for i in range(4):
        lp.seg[i] = float(seg[i])
    for d in range(7):
        lp.bounds[d][0], lp.bounds[d][1] = float(bounds[d][0]), float(bounds[d][1])
    return lp


class SensHarness:
    def __init__(self, so):
        self.lib = ctypes.CDLL(so)
        dp, ip, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(LegParamsC)
        self.lib.harness_fit_sensitivity.restype = ctypes.c_int
        self.lib.harness_fit_sensitivity.argtypes = [dp, dp, ctypes.c_int64, lp, dp, ctypes.c_double, dp, dp, ip]
        self.lib.harness_fit_sensitivity_staged.restype = ctypes.c_int
        self.lib.harness_fit_sensitivity_staged.argtypes = [dp, dp, ctypes.c_int64, lp, ctypes.c_double, dp]

    def run(self, angles, pose, seg, bounds, kp_sigma=None, tol=1e-6):
        """(n, 7), (n, 5, 3) [, (n, 4)] -> sens (n, 7, 4, 3), std (n, 7) or None, flags (n,) int32"""
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        angles, pose = np.ascontiguousarray(angles, dtype=np.float64), np.ascontiguousarray(pose, dtype=np.float64)
        n = angles.shape[0]
        assert angles.shape == (n, 7) and pose.shape == (n, 5, 3)
        sig = None if kp_sigma is None else np.ascontiguousarray(np.broadcast_to(kp_sigma, (n, 4)), dtype=np.float64)
        sens, flags = np.full((n, 7, 4, 3), 7.0), np.full(n, -1, dtype=np.int32)
        std = None if sig is None else np.full((n, 7), 7.0)
        lp = leg_params(seg, bounds)
        ptr = lambda a: a.ctypes.data_as(dp) if a is not None else None  # noqa: E731
        rc = self.lib.harness_fit_sensitivity(ptr(angles), ptr(pose), n, ctypes.byref(lp), ptr(sig), tol, ptr(sens),
                                              ptr(std), flags.ctypes.data_as(ip))
        assert rc == 0
        return sens, std, flags

    def staged(self, angles, pose, seg, bounds, tol=1e-6):
        dp = ctypes.POINTER(ctypes.c_double)
        angles, pose = np.ascontiguousarray(angles, dtype=np.float64), np.ascontiguousarray(pose, dtype=np.float64)
        sens = np.full((angles.shape[0], 7, 4, 3), 7.0)
        lp = leg_params(seg, bounds)
        assert self.lib.harness_fit_sensitivity_staged(angles.ctypes.data_as(dp), pose.ctypes.data_as(dp), angles.shape[0],
                                                       ctypes.byref(lp), tol, sens.ctypes.data_as(dp)) == 0
        return sens


@pytest.fixture(scope="module")
def sens_harness():
    return SensHarness(build_harness(os.path.join(ROOT, "tests", "harness", "sensitivity_harness.hip")))


def host_batch(sh, ang, pose, segs, bounds, kp_sigma=None, tol=1e-6):
    """The host-run rule over a (S, L, N, ...) batch, leg by leg -> sens (S, L, N, 7, 4, 3), std or None, flags."""
    S, L, N = ang.shape[:3]
    sens, flags = np.empty((S, L, N, 7, 4, 3)), np.empty((S, L, N), dtype=np.int32)
    std = None if kp_sigma is None else np.empty((S, L, N, 7))
    for li in range(L):
        sig = None if kp_sigma is None else np.ascontiguousarray(kp_sigma[:, li]).reshape(-1, 4)
        s, d, f = sh.run(np.ascontiguousarray(ang[:, li]).reshape(-1, 7), np.ascontiguousarray(pose[:, li]).reshape(-1, 5, 3),
                         segs[li], bounds[li], sig, tol)
        sens[:, li], flags[:, li] = s.reshape(S, N, 7, 4, 3), f.reshape(S, N)
        if d is not None:
            std[:, li] = d.reshape(S, N, 7)
    return sens, std, flags


# ------------------------------------------------ float64 restatement ------------------------------------------------

def numpy_frames(ang, seg):
    """Leg-local link frames (9, 3, 4) of the sequential chain, float64: T(0, 0, -seg) . R(axis, angle) link by link."""
    spec = [(None, None, None), (0, 0, None), (1, 1, None), (2, 2, None), (1, 3, 0), (2, 4, None), (1, 5, 1), (1, 6, 2),
            (None, None, 3)]
    R, t, out = np.eye(3), np.zeros(3), np.zeros((9, 3, 4))
    for i, (axis, a, s) in enumerate(spec):
        if s is not None:
            t = t + R @ np.array([0.0, 0.0, -seg[s]])
        if axis is not None:
            c, sn = np.cos(ang[a]), np.sin(ang[a])
            L = [np.array([[1, 0, 0], [0, c, -sn], [0, sn, c]]), np.array([[c, 0, sn], [0, 1, 0], [-sn, 0, c]]),
                 np.array([[c, -sn, 0], [sn, c, 0], [0, 0, 1]])][axis]
            R = R @ L
        out[i, :, :3], out[i, :, 3] = R, t
    return out


def numpy_rule(ang, pose, seg, bounds, tol=1e-6, curvature=True, hold=True):
    """One leg-frame -> sens (7, 4, 3), flags.  ``curvature=False``: Gauss-Newton (G = J^T J); ``hold=False``: no held
    joints -- the two wrong rules."""
    fr = numpy_frames(ang, seg)
    axis = [fr[l, :, c] for l, c in DOF_LINK]
    org = [fr[l, :, 3] for l, _ in DOF_LINK]
    S, flags = np.zeros((7, 4, 3)), 0
    for s, own in enumerate(STAGE_DOFS):
        f = fr[KEY_LINKS[s], :, 3]
        r = f - (pose[s + 1] - pose[0])
        n_col = own[-1] + 1
        J = [np.cross(axis[d], f - org[d]) for d in range(n_col)]

        def G(a, b):
            i, j = min(a, b), max(a, b)
            return J[a] @ J[b] + (r @ np.cross(axis[i], J[j]) if curvature else 0.0)
        free = []
        for a in own:
            g = J[a] @ r
            if hold and tol > 0 and ((ang[a] - bounds[a][0] <= tol and g > 0) or (bounds[a][1] - ang[a] <= tol and g < 0)):
                flags |= 1 << a
            else:
                free.append(a)
        if not free:
            continue
        GFF = np.array([[G(a, b) for b in free] for a in free])
        if GFF[0, 0] <= 0 or np.linalg.det(GFF) <= 0:
            flags |= 1 << (8 + s)
            S[free, :s + 1] = np.nan
            continue
        rhs = np.zeros((len(free), 4, 3))
        for i, a in enumerate(free):
            rhs[i, s] = J[a]
            for e in range(own[0]):
                rhs[i] -= G(a, e) * S[e]
        S[free] = np.linalg.solve(GFF, rhs.reshape(len(free), 12)).reshape(len(free), 4, 3)
        S[free, s + 1:] = 0.0
    return S, flags


def numpy_std(sens, sigma):
    """std (..., 7) from sens (..., 7, 4, 3) and sigma (..., 4) by the header's formula."""
    return np.sqrt(((sens ** 2).sum(-1) * np.asarray(sigma)[..., None, :] ** 2).sum(-1))


# ------------------------------------------------- 200-bit yardstick -------------------------------------------------

def _mp_cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _mp_dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def mp_key_points(ang, seg):
    """Leg-local key points 1..4 at 200 bits -> list of four [x, y, z] of mpf."""
    fr = mp_chain(0, ang, seg, np.zeros((5, 3)))[0]
    return [[_MP.mpf(float(fr[0, l, r, 3])) + _MP.mpf(float(fr[1, l, r, 3])) for r in range(3)] for l in KEY_LINKS]


def mp_rule(ang, pose, seg, bounds, tol=1e-6):
    """One leg-frame at 200 bits -> dict(sens (7, 4, 3) float64 of the exact values (NaN rows where the rule gives NaN),
    flags, kappa (4,): the 2-norm condition number of G_FF per stage (1 where nothing or one DOF is free), margin: the
    smallest relative distance of a held / positive-definite verdict from flipping (|g| / (|J| |r|) of an own DOF that
    sits within tol of a limit, |G_aa| / (|J_a|^2 + |r| |a x J_a|) and |det| / (G_aa G_bb scale) of a solve))."""
    mpf = _MP.mpf
    fr = mp_chain(0, ang, seg, np.zeros((5, 3)))[0]
    F = [[[mpf(float(fr[0, i, r, c])) + mpf(float(fr[1, i, r, c])) for c in range(4)] for r in range(3)] for i in range(9)]
    axis = [[F[l][r][c] for r in range(3)] for l, c in DOF_LINK]
    org = [[F[l][r][3] for r in range(3)] for l, _ in DOF_LINK]
    P = [[mpf(float(v)) for v in row] for row in pose]
    S = [[[mpf(0)] * 3 for _ in range(4)] for _ in range(7)]
    bad = [[False] * 4 for _ in range(7)]     # NaN entries of S, per (DOF, key point)
    flags, kappa, margin = 0, np.ones(4), np.inf
    norm = lambda v: _MP.sqrt(_mp_dot(v, v))  # noqa: E731
    for s, own in enumerate(STAGE_DOFS):
        f = [F[KEY_LINKS[s]][r][3] for r in range(3)]
        r = [f[c] - (P[s + 1][c] - P[0][c]) for c in range(3)]
        J = [_mp_cross(axis[d], [f[c] - org[d][c] for c in range(3)]) for d in range(own[-1] + 1)]

        def G(a, b):
            i, j = min(a, b), max(a, b)
            return _mp_dot(J[a], J[b]) + _mp_dot(r, _mp_cross(axis[i], J[j]))

        def G_scale(a, b):
            i, j = min(a, b), max(a, b)
            return norm(J[a]) * norm(J[b]) + norm(r) * norm(_mp_cross(axis[i], J[j]))
        free = []
        for a in own:
            g = _mp_dot(J[a], r)
            at_lb = mpf(float(ang[a])) - mpf(float(bounds[a][0])) <= mpf(tol)
            at_ub = mpf(float(bounds[a][1])) - mpf(float(ang[a])) <= mpf(tol)
            if tol > 0 and (at_lb or at_ub):
                scale = norm(J[a]) * norm(r)
                margin = min(margin, float(abs(g) / scale) if scale > 0 else 0.0)
            if tol > 0 and ((at_lb and g > 0) or (at_ub and g < 0)):
                flags |= 1 << a
            else:
                free.append(a)
        if not free:
            continue
        a = free[0]
        Gaa = G(a, a)
        margin = min(margin, float(abs(Gaa) / G_scale(a, a)))
        if len(free) == 2:
            b = free[1]
            Gab, Gbb = G(a, b), G(b, b)
            det = Gaa * Gbb - Gab * Gab
            margin = min(margin, float(abs(det) / (G_scale(a, a) * G_scale(b, b))))
            pd = Gaa > 0 and det > 0
        else:
            pd = Gaa > 0
        if not pd:
            flags |= 1 << (8 + s)
            for d in free:
                for k in range(s + 1):
                    bad[d][k] = True
            continue
        if len(free) == 2:
            ev = _MP.eigsy(_MP.matrix([[Gaa, Gab], [Gab, Gbb]]), eigvals_only=True)
            kappa[s] = float(max(ev) / min(ev))
        for k in range(s + 1):
            nan_k = any(bad[e][k] for e in range(own[0]))
            for d in free:
                bad[d][k] = nan_k and k < s
            if nan_k and k < s:
                continue
            for c in range(3):
                y = []
                for d in free:
                    v = J[d][c] if k == s else mpf(0)
                    for e in range(own[0]):
                        v -= G(d, e) * S[e][k][c]
                    y.append(v)
                if len(free) == 2:
                    S[a][k][c] = (Gbb * y[0] - Gab * y[1]) / det
                    S[b][k][c] = (Gaa * y[1] - Gab * y[0]) / det
                else:
                    S[a][k][c] = y[0] / Gaa
    out = np.array([[[float(S[d][k][c]) for c in range(3)] for k in range(4)] for d in range(7)])
    out[np.array(bad)] = np.nan
    return dict(sens=out, flags=flags, kappa=kappa, margin=margin)
