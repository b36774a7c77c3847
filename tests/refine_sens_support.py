"""TEST INFRASTRUCTURE -- what the tests of the refinement's sensitivity (include/seqik_refine_sensitivity.h) share: the
host harness (csrc/seqik_refine_sens.hpp compiled for the host), a float64 numpy restatement of the rule (np.cross,
np.linalg.cholesky / solve; with a switch for the Gauss-Newton rule the solver test measures), the 200-bit yardstick on
``mp_chain`` of tests/test_fk_accuracy.py with an mpmath linear solve, and a stand-in for ``_lib._call``.  Nothing here is
taken from csrc."""
import ctypes
import json
import os

import numpy as np
import pytest

from angle_map_support import switches
from conftest import ROOT, LegParamsC
from harness_build import build_harness
from refine_support import NONZERO, RefineHarness, made_up_legs, shipped_frames, targets_of
from refine_support import harness_call as refine_harness_call
from sensitivity_support import DOF_LINK, KEY_LINKS, _mp_cross, _mp_dot, leg_params, numpy_frames, numpy_std  # noqa: F401
from test_fk_accuracy import _MP, mp_chain

BAD_INPUT, NOT_PD = 1 << 16, 1 << 8
TOL = 1e-6
WIDTH = dict(sens=84, std=7, grad=1, flags=1)
ROBUST = 2.0 ** -40
EPS = np.finfo(float).eps
PROFILE = os.path.join(ROOT, "profiles", "refine_sensitivity_accuracy.json")


def record(key, value):
    """Keeps a measured value in profiles/refine_sensitivity_accuracy.json when SEQIK_RECORD_PROFILES is set (the
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


class RefSensHarness:
    def __init__(self, so):
        self.lib = ctypes.CDLL(so)
        dp, ip, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(LegParamsC)
        self.lib.harness_refine_sensitivity.restype = ctypes.c_int
        self.lib.harness_refine_sensitivity.argtypes = [dp, dp, ctypes.c_int64, lp, dp, dp, ctypes.c_double, dp, dp, dp, ip]
        self.lib.harness_refine_sensitivity_staged.restype = ctypes.c_int
        self.lib.harness_refine_sensitivity_staged.argtypes = [dp, dp, ctypes.c_int64, lp, dp, ctypes.c_double, dp]
        self.lib.harness_refsens_factor.restype = ctypes.c_int
        self.lib.harness_refsens_factor.argtypes = [dp, ctypes.c_int32]

    def run(self, angles, pose, seg, bounds, weight=None, kp_sigma=None, tol=TOL, want=("sens", "grad", "flags")):
        """(n, 7), (n, 5, 3) [, weights and sigmas that broadcast to (n, 4)] -> dict(sens (n, 7, 4, 3), std (n, 7), grad
        (n,), flags (n,) int32), None for what is not in ``want`` (std is wanted whenever kp_sigma is given)."""
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        angles, pose = np.ascontiguousarray(angles, dtype=np.float64), np.ascontiguousarray(pose, dtype=np.float64)
        n = angles.shape[0]
        assert angles.shape == (n, 7) and pose.shape == (n, 5, 3)
        bc = lambda v: None if v is None else np.ascontiguousarray(np.broadcast_to(v, (n, 4)), dtype=np.float64)  # noqa: E731
        w, sig = bc(weight), bc(kp_sigma)
        out = dict(sens=np.full((n, 7, 4, 3), 7.0) if "sens" in want else None,
                   std=np.full((n, 7), 7.0) if sig is not None else None,
                   grad=np.full(n, 7.0) if "grad" in want else None,
                   flags=np.full(n, -1, dtype=np.int32) if "flags" in want else None)
        lp = leg_params(seg, bounds)
        ptr = lambda a: a.ctypes.data_as(dp) if a is not None else None  # noqa: E731
        rc = self.lib.harness_refine_sensitivity(ptr(angles), ptr(pose), n, ctypes.byref(lp), ptr(w), ptr(sig), tol,
                                                 ptr(out["sens"]), ptr(out["std"]), ptr(out["grad"]),
                                                 out["flags"].ctypes.data_as(ip) if out["flags"] is not None else None)
        assert rc == 0
        return out

    def staged(self, angles, pose, seg, bounds, weight=None, tol=TOL):
        dp = ctypes.POINTER(ctypes.c_double)
        angles, pose = np.ascontiguousarray(angles, dtype=np.float64), np.ascontiguousarray(pose, dtype=np.float64)
        n = angles.shape[0]
        w = None if weight is None else np.ascontiguousarray(np.broadcast_to(weight, (n, 4)), dtype=np.float64)
        sens = np.full((n, 7, 4, 3), 7.0)
        lp = leg_params(seg, bounds)
        assert self.lib.harness_refine_sensitivity_staged(angles.ctypes.data_as(dp), pose.ctypes.data_as(dp), n, ctypes.byref(lp),
                                                          w.ctypes.data_as(dp) if w is not None else None, tol,
                                                          sens.ctypes.data_as(dp)) == 0
        return sens

    def factor(self, H, held=0):
        """The masked Cholesky factorisation alone -> (the factor's lower triangle (7, 7), every pivot positive)."""
        M = np.array(H, dtype=np.float64, order="C")
        pd = self.lib.harness_refsens_factor(M.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), held)
        return np.tril(M), bool(pd)


def _preload_torch():
    # The harness libraries link the HIP runtime hipcc ships with; torch bundles its own.  Whichever is loaded first owns
    # the GPU (seqikpy_amd/_lib.py, load()), so in a process that will use torch, torch goes first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


@pytest.fixture(scope="session")
def refine_sens_harness():
    _preload_torch()
    return RefSensHarness(build_harness(os.path.join(ROOT, "tests", "harness", "refine_sens_harness.hip")))


@pytest.fixture(scope="session")
def refine_rule_harness():
    """The host-run 7n rule (tests/harness/refine_harness.hip) and the FK rule: what refines the inputs."""
    _preload_torch()
    return RefineHarness(build_harness(os.path.join(ROOT, "tests", "harness", "refine_harness.hip")),
                         build_harness(os.path.join(ROOT, "tests", "harness", "fk_harness.hip")))


def host_batch(sh, ang, pose, segs, bounds, weight=None, kp_sigma=None, tol=TOL, want=("sens", "grad", "flags")):
    """The host-run rule over a (S, L, N, ...) batch, leg by leg -> dict of (S, L, N, ...) arrays (None: not wanted)."""
    S, L, N = ang.shape[:3]
    parts = []
    for li in range(L):
        flat = lambda a, *tail: None if a is None else np.ascontiguousarray(a[:, li]).reshape((-1,) + tail)  # noqa: E731
        parts.append(sh.run(flat(ang, 7), flat(pose, 5, 3), segs[li], bounds[li], flat(weight, 4), flat(kp_sigma, 4), tol, want))
    out = {}
    for k in ("sens", "std", "grad", "flags"):
        if parts[0][k] is None:
            out[k] = None
        else:
            out[k] = np.stack([p[k].reshape((S, N) + p[k].shape[1:]) for p in parts], axis=1)
    return out


# ------------------------------------------------------- inputs -------------------------------------------------------

_REFINED = {}


def refined_inputs(rh):
    """The inputs of the CPU tier, refined once by the host-run rule of seqik_refine.h from their starts: the 575 shipped
    frames (refine_support.shipped_frames) and the 40 made-up legs of 24 frames (made_up_legs: targets out of reach and
    on the origin, seeds on a limit) -> [(name, refined angles (n, 7), pose (n, 5, 3), seg, bounds, info (n,))]"""
    if not _REFINED:
        cases = [(leg, ang, pose[:, :5], seg, b) for leg, _, ang, pose, seg, b in shipped_frames()]
        cases += [(f"made-up {i}", ang, pose[:, :5], seg, b) for i, (ang, pose, seg, b) in enumerate(made_up_legs())]
        out = []
        for name, ang, pose, seg, b in cases:
            q, _, info = rh.run(ang, pose, seg, b)
            out.append((name, q, np.ascontiguousarray(pose), np.asarray(seg), np.asarray(b), info))
        _REFINED["cases"] = out
    return _REFINED["cases"]


FD_FRAMES = tuple(range(0, 6000, 400))      # of RF and of LF: the 30 frames of the solver test


# ------------------------------------------------ float64 restatement ------------------------------------------------

def numpy_rule(q, pose, seg, bounds, weight=None, tol=TOL, curvature=True):
    """The rule of include/seqik_refine_sensitivity.h for one leg-frame in float64 numpy -> dict(sens (7, 4, 3), flags,
    grad, g (7,), H (7, 7)).  ``curvature=False``: Gauss-Newton (H = J^T J), the wrong rule."""
    w = np.ones(4) if weight is None else np.asarray(weight, dtype=np.float64)
    lb, ub = np.asarray(bounds)[:, 0], np.asarray(bounds)[:, 1]
    t = targets_of(pose, w)
    fr = numpy_frames(q, seg)
    axis = [fr[l, :, c] for l, c in DOF_LINK]
    org = [fr[l, :, 3] for l, _ in DOF_LINK]
    J, r, H = np.zeros((4, 3, 7)), np.zeros((4, 3)), np.zeros((7, 7))
    for k in range(4):
        f = fr[KEY_LINKS[k], :, 3]
        r[k] = w[k] * (f - t[k])
        for d in range(7):
            if NONZERO[k, d]:
                J[k, :, d] = w[k] * np.cross(axis[d], f - org[d])
        H += J[k].T @ J[k]
        if curvature:
            for a in range(7):
                for b in range(a, 7):
                    if NONZERO[k, a] and NONZERO[k, b]:
                        h = r[k] @ np.cross(axis[a], J[k, :, b])
                        H[a, b] += h
                        if b != a:
                            H[b, a] += h
    g = np.einsum("kcd,kc->d", J, r)
    held = (tol > 0) & (((q - lb <= tol) & (g > 0)) | ((ub - q <= tol) & (g < 0)))
    F = np.where(~held)[0]
    flags = int(sum(1 << j for j in range(7) if held[j]))
    sens = np.zeros((7, 4, 3))
    if len(F):
        try:
            np.linalg.cholesky(H[np.ix_(F, F)])
            rhs = np.stack([w[k] * J[k][:, F].T for k in range(4)], axis=1)      # (F, 4, 3)
            sens[F] = np.linalg.solve(H[np.ix_(F, F)], rhs.reshape(len(F), 12)).reshape(len(F), 4, 3)
            sens[:, w == 0] = 0.0
        except np.linalg.LinAlgError:
            flags |= NOT_PD
            sens[F] = np.nan
    grad = (np.abs(g[F]).max() if len(F) else 0.0) / np.sum(seg) ** 2
    return dict(sens=sens, flags=flags, grad=grad, g=g, H=H)


# ------------------------------------------------- 200-bit yardstick -------------------------------------------------

def mp_rule(q, pose, seg, bounds, weight=None, tol=TOL):
    """One leg-frame at 200 bits: H, g, the held verdicts and sens = H_FF^-1 (w_k J_k,F) with an mpmath linear solve
    -> dict(sens (7, 4, 3) float64 of the exact values (NaN rows where the rule gives NaN), flags, grad, robust: False
    when a held verdict (|g_a| <= 2^-40 |J_a| |r| of a DOF within tol of a limit) or the positive-definite verdict
    (smallest pivot of the masked 7 x 7 factorisation <= 2^-40 of the largest, in magnitude) could flip under rounding)."""
    mpf = _MP.mpf
    w = [mpf(1)] * 4 if weight is None else [mpf(float(v)) for v in weight]
    fr = mp_chain(0, q, seg, np.zeros((5, 3)))[0]
    Fm = [[[mpf(float(fr[0, i, r, c])) + mpf(float(fr[1, i, r, c])) for c in range(4)] for r in range(3)] for i in range(9)]
    axis = [[Fm[l][r][c] for r in range(3)] for l, c in DOF_LINK]
    org = [[Fm[l][r][3] for r in range(3)] for l, _ in DOF_LINK]
    P = [[mpf(float(v)) for v in row] for row in pose]
    H = [[mpf(0)] * 7 for _ in range(7)]
    g, gs = [mpf(0)] * 7, [mpf(0)] * 7                   # g_a and the scale sum_k |J_ka| |r_k|
    J = [[None] * 7 for _ in range(4)]
    norm = lambda v: _MP.sqrt(_mp_dot(v, v))  # noqa: E731
    for k in range(4):
        if w[k] == 0:
            continue
        f = [Fm[KEY_LINKS[k]][r][3] for r in range(3)]
        res = [w[k] * (f[c] - (P[k + 1][c] - P[0][c])) for c in range(3)]
        for d in range(7):
            if NONZERO[k, d]:
                J[k][d] = [w[k] * v for v in _mp_cross(axis[d], [f[c] - org[d][c] for c in range(3)])]
                g[d] += _mp_dot(J[k][d], res)
                gs[d] += norm(J[k][d]) * norm(res)
        for a in range(7):
            for b in range(a, 7):
                if NONZERO[k, a] and NONZERO[k, b]:
                    h = _mp_dot(J[k][a], J[k][b]) + _mp_dot(res, _mp_cross(axis[a], J[k][b]))
                    H[a][b] += h
                    if b != a:
                        H[b][a] += h
    flags, robust, free = 0, True, []
    for a in range(7):
        at_lb = mpf(float(q[a])) - mpf(float(bounds[a][0])) <= mpf(tol)
        at_ub = mpf(float(bounds[a][1])) - mpf(float(q[a])) <= mpf(tol)
        if tol > 0 and (at_lb or at_ub) and abs(g[a]) <= mpf(ROBUST) * gs[a]:
            robust = False
        if tol > 0 and ((at_lb and g[a] > 0) or (at_ub and g[a] < 0)):
            flags |= 1 << a
        else:
            free.append(a)
    sens = np.zeros((7, 4, 3))
    leg2 = sum(mpf(float(s)) for s in seg) ** 2
    grad = float(max([abs(g[a]) for a in free], default=mpf(0)) / leg2)
    if free:
        n = len(free)
        A = _MP.matrix(n, n)
        for i, a in enumerate(free):
            for j, b in enumerate(free):
                A[i, j] = H[a][b]
        # the pivots s_j of the factorisation the header defines: the 7 x 7 matrix in DOF order with the rows and columns of
        # held DOFs replaced by the identity's (their pivots are 1); all positive <=> H_FF positive definite
        held = [a not in free for a in range(7)]
        Mk = [[(mpf(1) if a == b else mpf(0)) if held[a] or held[b] else H[a][b] for b in range(7)] for a in range(7)]
        Lm, piv = [[mpf(0)] * 7 for _ in range(7)], []
        for j in range(7):
            d = Mk[j][j] - sum(Lm[j][k] ** 2 * piv[k] for k in range(j))
            piv.append(d)
            for i in range(j + 1, 7):
                Lm[i][j] = (Mk[i][j] - sum(Lm[i][k] * Lm[j][k] * piv[k] for k in range(j))) / d if d != 0 else mpf(0)
        if min(abs(p) for p in piv) <= mpf(ROBUST) * max(abs(p) for p in piv):
            robust = False
        if all(p > 0 for p in piv):
            for k in range(4):
                for c in range(3):
                    rhs = _MP.matrix([w[k] * J[k][a][c] if J[k][a] is not None else mpf(0) for a in free])
                    x = _MP.lu_solve(A, rhs)
                    for i, a in enumerate(free):
                        sens[a, k, c] = float(x[i])
        else:
            flags |= NOT_PD
            sens[free] = np.nan
    return dict(sens=sens, flags=flags, grad=grad, robust=robust)


# ------------------------------------- the library call answered by the host harness -------------------------------------

def harness_call(sh, rh, real_call):
    """A stand-in for ``_lib._call`` that answers ``seqik_refine_sensitivity`` with the host-run rule, leg by leg, and
    hands ``seqik_refine_legs`` / ``seqik_forward_kinematics`` to refine_support's stand-in: what the CPU tier can run of
    the Python surface (the product itself has no CPU path)."""
    inner = refine_harness_call(rh, real_call)
    fn = sh.lib.harness_refine_sensitivity
    addr = lambda ptr: ctypes.cast(ptr, ctypes.c_void_p).value if ptr is not None else None  # noqa: E731
    dp, ip, lpp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(LegParamsC)
    at = lambda base, width, i: None if base is None else ctypes.cast(base + 8 * width * i, dp)  # noqa: E731

    def call(name, *args):
        if name != "seqik_refine_sensitivity":
            return inner(name, *args)
        angles, pose, S, L, N, legs, kind, weight, sigma, tol, sens, std, grad, flags, device = args
        assert kind == 0
        for s in range(S):
            for l in range(L):
                i = (s * L + l) * N
                f = None if flags is None else ctypes.cast(addr(flags) + 4 * i, ip)
                rc = fn(at(addr(angles), 7, i), at(addr(pose), 15, i), N, ctypes.cast(ctypes.byref(legs[l]), lpp),
                        at(addr(weight), 4, i), at(addr(sigma), 4, i), tol, at(addr(sens), 84, i), at(addr(std), 7, i),
                        at(addr(grad), 1, i), f)
                assert rc == 0
        return None
    return call


# ------------------------------------------------------ GPU tier ------------------------------------------------------

SENTINEL, SENTINEL_I = -12345.678, -1234567
SUBSETS = (("sens",), ("std",), ("flags", "grad"), ("sens", "std", "grad", "flags"))
GPU_FRAMES = (1, 3, 4, 5, 63, 64, 65, 300)      # the quarter-record and wavefront seams
GPU_S, GPU_L = 2, 3


def gpu_batch(seed, S, L, N):
    """Angles inside made-up limits, some on one; targets = the chain's key points + noise; weights (some exactly 0, that
    key point NaN), sigmas; leg-frames with a NaN angle, an angle outside the domain, an infinite coordinate, a negative
    weight and a NaN sigma -> ang (S, L, N, 7), pose (S, L, N, 5, 3), weight, sigma (S, L, N, 4), segs (L, 4), bounds"""
    rng = np.random.default_rng(seed)
    segs = np.random.default_rng(3).uniform(0.15, 1.8, (8, 4))[:L]
    lo = np.random.default_rng(4).uniform(-2.5, -1.0, (8, 7))[:L]
    bounds = np.stack([lo, lo + np.random.default_rng(5).uniform(2.0, 4.0, (8, 7))[:L]], -1)
    ang = rng.uniform(bounds[None, :, None, :, 0], bounds[None, :, None, :, 1], (S, L, N, 7))
    on = rng.random((S, L, N, 7)) < 0.08             # on a limit: either one, exactly or 1e-9 inside
    side = rng.integers(0, 2, (S, L, N, 7))
    edge = np.where(side == 0, bounds[None, :, None, :, 0] + 1e-9 * rng.integers(0, 2, (S, L, N, 7)),
                    bounds[None, :, None, :, 1] - 1e-9 * rng.integers(0, 2, (S, L, N, 7)))
    ang = np.where(on, edge, ang)
    pose = np.empty((S, L, N, 5, 3))
    pose[..., 0, :] = rng.standard_normal((S, L, N, 3))
    for s in range(S):
        for l in range(L):
            for n in range(N):
                kp = numpy_frames(ang[s, l, n], segs[l])[list(KEY_LINKS), :, 3]
                pose[s, l, n, 1:] = pose[s, l, n, 0] + kp + 0.02 * rng.standard_normal((4, 3))
    weight = rng.uniform(0.5, 2.0, (S, L, N, 4))
    none = rng.random((S, L, N, 4)) < 0.1
    weight[none] = 0.0
    pose[..., 1:, :][none] = np.nan                  # a key point without weight is not read
    sigma = rng.uniform(0.01, 0.1, (S, L, N, 4))
    fa, fp, fw, fs = ang.reshape(-1, 7), pose.reshape(-1, 15), weight.reshape(-1, 4), sigma.reshape(-1, 4)
    n = fa.shape[0]
    if n >= 15:   # records whose neighbours in the four-lane group and the 16-record pass must keep their bits
        fa[n // 3, 4] = np.nan
        fa[n - 1, 0] = 1e300
        fp[n // 2, 1] = np.inf
        fw[7, 1] = -1.0
        fs[5, 2] = np.nan
    return ang, pose, weight, sigma, segs, bounds


_GPU_CASES = {}


def gpu_case(sh, N):
    """Inputs and the host-run rule's answers for them, computed once per size: with std (the sigmas are read) and
    without (they are not: the leg-frame with the NaN sigma is clean then)."""
    if N not in _GPU_CASES:
        ang, pose, weight, sigma, segs, bounds = gpu_batch(500 + N, GPU_S, GPU_L, N)
        all4 = ("sens", "grad", "flags")
        _GPU_CASES[N] = dict(ang=ang, pose=pose, weight=weight, sigma=sigma, segs=segs, bounds=bounds,
                             with_std=host_batch(sh, ang, pose, segs, bounds, weight, sigma, want=all4),
                             no_std=host_batch(sh, ang, pose, segs, bounds, weight, None, want=all4))
    return _GPU_CASES[N]


def device_run(lib, c, want, staged="0"):
    """The device entry point on torch tensors with one guard record on each side of every output, all filled with a
    sentinel -> {name: (S, L, N, width)} of the outputs asked for; asserts that the guards and the outputs not asked for
    are untouched."""
    import torch
    S, L, N = c["ang"].shape[:3]
    n = S * L * N
    d_in = [torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("ang", "pose", "weight", "sigma")]
    bufs = {k: torch.full(((n + 2) * w,), SENTINEL_I if k == "flags" else SENTINEL,
                          dtype=torch.int32 if k == "flags" else torch.float64, device="cuda") for k, w in WIDTH.items()}
    ptr = {k: (bufs[k].data_ptr() + bufs[k].element_size() * WIDTH[k] if k in want else 0) for k in WIDTH}
    params = [lib.leg_params_from_arrays(s, b, np.zeros(27)) for s, b in zip(c["segs"], c["bounds"])]
    with switches(SEQIK_REFSENS_STAGED=staged):      # read per call: 0 = per lane (the default), 1 = the staged store path
        lib.refine_sensitivity_device(d_in[0].data_ptr(), d_in[1].data_ptr(), S, L, N, params, d_kp_weight=d_in[2].data_ptr(),
                                      d_kp_sigma=d_in[3].data_ptr(), d_sens=ptr["sens"], d_std=ptr["std"], d_grad=ptr["grad"],
                                      d_flags=ptr["flags"], stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    out = {}
    for k, w in WIDTH.items():
        got, sent = bufs[k].cpu().numpy(), SENTINEL_I if k == "flags" else SENTINEL
        assert (got[:w] == sent).all() and (got[-w:] == sent).all(), (k, "guard", want, N)
        if k in want:
            out[k] = got[w:-w].reshape(S, L, N, w)
        else:
            assert (got == sent).all(), (k, "not requested", want, N)
    return out


def check_device_against_host(lib, c, want, staged="0"):
    S, L, N = c["ang"].shape[:3]
    got = device_run(lib, c, want, staged)
    ref = c["with_std"] if "std" in want else c["no_std"]
    for k in want:
        if k == "flags":
            assert np.array_equal(got[k][..., 0], ref[k]), (k, N, want, staged)
        else:
            a, b = got[k].reshape(-1).view(np.uint64), np.ascontiguousarray(ref[k]).reshape(-1).view(np.uint64)
            assert np.array_equal(a, b), (k, N, want, staged, int((a != b).sum()))


if __name__ == "__main__":
    # The child process of the GPU tier's test of SEQIK_REFSENS_BLOCK / SEQIK_REFSENS_GRID: the environment is the
    # parent's plus the switches; the cases (inputs and the host-run rule's answers) come in an .npz.
    import sys
    from seqikpy_amd import _lib as hiplib
    cases = np.load(sys.argv[1], allow_pickle=True)["cases"].item()
    assert os.environ["SEQIK_REFSENS_BLOCK"] == "64" and os.environ["SEQIK_REFSENS_GRID"] == "1"
    for N, c in cases.items():
        for want in SUBSETS:
            for staged in ("0", "1"):
                check_device_against_host(hiplib, c, want, staged)
    print("CHILD OK", sorted(cases))
