"""Forward kinematics and link frames against a 200-bit yardstick; NaN outside the angle domain.

``seqik_forward_kinematics[_device]`` and ``seqik_link_frames[_device]`` take angles from outside the project.  Their
other tests compare them with code that shares their arithmetic (bit for bit) or with a float64 stand-in at a flat
1e-12, on angles inside +-3.3 rad.  Here the device functions of csrc/seqik_fk.hpp / seqik_frames.hpp -- run on the host
(CPU tier) and as kernels (``-m gpu``) -- are held to a bound derived from the number format, on the angles that reach
them in practice (unwrapped, multiples of pi / 2, large, tiny), and the edge of the domain is pinned: an angle that is
not finite or lies beyond ``SEQIK_ANGLE_MAX`` = 2^30 rad makes its leg-frame NaN and leaves every other one alone.

YARDSTICK.  ``mp_chain``: the nine-link chain of include/seqik_frames.h -- link order, axes and translations as that
header lists them, nothing taken from csrc -- multiplied out in mpmath at 200 bits (the issue asked for >= 160) from the
float64 inputs taken as exact.  It gives every frame; the FK rows are the translation columns, the distances
|row 4, 6, 7, 8 - key point 1, 2, 3, 4|.  Kept as a float64 pair (hi, lo), so an error is ``(got - hi) - lo``.

BOUND.  u = 2^-53.  Per link i of a leg-frame:  |got - truth| <= K u S_i, with S_i = 1 for the nine rotation entries
and S_i = |seg| summed up to link i + |origin|_inf for the position; for a distance the S of its row + |key point -
origin|.  ``K_ref`` is the smallest power of two for which the float64 numpy restatement of the reference
(oracle/shim/ikpy: its own np.sin / np.cos and matrix order) stays inside that bound on exactly the inputs below; the
tests use K = 4 K_ref, the rule and the margin of tests/test_head_accuracy.py (two correctly rounded evaluation orders
of an eight-product chain differ by a small factor).  K is never read off the code under test and no input is left out.

INPUT FAMILIES (seeded, built here; both chain kinds; (legs, frames) leg-frames, a leg = one set of segment lengths)
  a. in range (3, 130): angles in [-pi, pi], segment lengths in [0.15, 1.8], origin 0 for the first half, random after.
  b. unwrapped (8, 47): all joints in +-[pi, 200 pi]; each joint swept alone over that range, the others fixed.
  c. multiples of pi / 2 (1, 623): k pi / 2 rounded to double and +-1, +-2, +-3 ulp around it, |k| <= 40 and
     +-{100, 12345, 2^20, 2^24}; leg-frame j gives joint d value (j + 89 d) mod 623, so every joint takes every value.
  d. large (2, 103): magnitudes log-uniform in [1e3, 2^30], either sign; exactly +-2^30 on each joint.
  e. tiny and zero (1, 80): +-0.0, +-5e-324, +-1e-310, +-1e-300, +-1e-9, all joints at once and each joint alone.
     Compared by value; the sign of zero entries is counted and printed, not asserted.
  f. scaling: family a's segment lengths, origins and key points times 2^k, k in {-20, -1, 1, 20}: positions and
     distances are 2^k times the unscaled run's bit for bit, the rotation blocks the unscaled run's.
  g. large origin (1, 130): leg 0 of family a with origins of magnitude 1e6: the bound with its S, and the rotation
     blocks of the origin-0 run bit for bit.
  h. outside the domain: nextafter(+-2^30, +-inf), +-3.3731e9, +-3.38e9, +-1e12, +-1e18, +-1e300, +-inf, NaN in joint
     0, 3 or 6 of leg-frames 0, 15, 16, 63, 64, 129 of a 130-frame recording: those are NaN (27 + 4 values, or 108),
     every other leg-frame keeps the bits of the clean run.

IDENTITIES on every family: the translation column of the frames == the FK rows bit for bit.  Link 1 of the sequential
chain is R_x(angle 0), i.e. it holds cos, sin and -sin of that angle as ``sincos_cw`` (csrc/seqik_core.hpp) returns them:
equal to ``host_harness.sincos`` bit for bit on families b-e, and against mpmath within 1 ulp for |x| <= 1e7 (the
measured 0.996 ulp rounded up to the unit), within 2^-53 absolute beyond.

MEASURED (EXPERIMENTS.md, "FK and link frames accuracy"; the tests print the figures, ``-s``).  K_ref = 4 (largest
ratio of the restatement: 3.149), K = 16.  Worst error / (u S) over rotation entries, positions and distances:
    family                     a      b      c      d      e      g
    restatement (both kinds)  2.903  3.103  1.911  3.149  2.100  2.903
    host build, sequential    2.908  2.809  1.709  2.628  2.317  2.733
    host build, generic       2.903  3.103  1.911  3.149  2.100  2.903
(the rule was written to follow IKPy's order of operations, so it lands on the restatement's worst entries).  sin / cos
through link 1, host build: 0.648 ulp at |x| <= 1e7, 0.616 * 2^-53 beyond.  Family e: 129 of 964 zero entries of the
sequential chain and 7 of 966 of the generic chain differ in sign from the restatement.  Device: not measured when this was written
(no GPU run could be made); the GPU tier asserts the host build's bits and the bound on the device output itself.
"""
import os
import sys

import mpmath
import numpy as np
import pytest

from angle_map_support import gpu_lib, same_bits, switches
from conftest import ROOT, host_harness  # noqa: F401  (fixture: sincos_cw run on the host)
from test_forward_kinematics import fk_harness  # noqa: F401  (fixture: the FK rule run on the host)
from test_link_frames import frames_harness  # noqa: F401  (fixture: the frames rule run on the host)

U = 2.0 ** -53
ANGLE_MAX = 2.0 ** 30
K_REF = 4
K = 4 * K_REF
KINDS = (0, 1)
KIND_NAMES = ("seq", "generic")
FK_ROWS = (4, 6, 7, 8)
# nine links per kind as include/seqik_frames.h lists them: (axis or None, index into the 7 angles, index into seg)
SPEC = {0: [(None, None, None), ("x", 0, None), ("y", 1, None), ("z", 2, None), ("y", 3, 0), ("z", 4, None), ("y", 5, 1),
            ("y", 6, 2), (None, None, 3)],
        1: [(None, None, None), ("z", 2, None), ("x", 0, None), ("y", 1, None), ("y", 3, 0), ("z", 4, None), ("y", 5, 1),
            ("y", 6, 2), (None, None, 3)]}
# 3.38e9 first: beyond 2^31 pi / 2 the quadrant of sincos_cw's argument reduction does not fit its int (sin comes back as
# the cosine), so without the domain check these give finite, plausible, wrong rows
OUTSIDE = [3.38e9, -3.38e9, 3.3731e9, -3.3731e9, float(np.nextafter(ANGLE_MAX, np.inf)), -float(np.nextafter(ANGLE_MAX, np.inf)),
           1e12, -1e12, 1e18, -1e18, 1e300, -1e300, np.inf, -np.inf, np.nan]
H_JOINTS, H_FRAMES, H_N = (0, 3, 6), (0, 15, 16, 63, 64, 129), 130


# ------------------------------------------------------ yardstick ------------------------------------------------------

_MP = mpmath.mp.clone()
_MP.prec = 200
_SINCOS = {}


def _mp_sincos(x):
    if x not in _SINCOS:
        t = _MP.mpf(x)
        _SINCOS[x] = (_MP.sin(t), _MP.cos(t))
    return _SINCOS[x]


def _mp_rot(axis, x):
    s, c = _mp_sincos(x)
    one, zero = _MP.mpf(1), _MP.mpf(0)
    if axis == "x":
        return [[one, zero, zero], [zero, c, -s], [zero, s, c]]
    if axis == "y":
        return [[c, zero, s], [zero, one, zero], [-s, zero, c]]
    return [[c, -s, zero], [s, c, zero], [zero, zero, one]]


def _split(v):
    hi = float(v)
    return hi, float(v - _MP.mpf(hi))


def mp_chain(kind, ang, seg, pose):
    """One leg-frame -> (frames (2, 9, 3, 4), dist (2, 4)): hi and lo parts of the exact values.  Frame i = the product of
    the link matrices 0 .. i, each T(0, 0, -seg) . R(axis, angle); the origin (key point 0) is added to the position."""
    R = [[_MP.mpf(int(i == j)) for j in range(3)] for i in range(3)]
    t = [_MP.mpf(0)] * 3
    org = [_MP.mpf(float(v)) for v in pose[0]]
    frames, dist = np.zeros((2, 9, 3, 4)), np.zeros((2, 4))
    for i, (axis, a, s) in enumerate(SPEC[kind]):
        if s is not None:
            tz = -_MP.mpf(float(seg[s]))
            t = [R[r][2] * tz + t[r] for r in range(3)]
        if axis is not None:
            L = _mp_rot(axis, float(ang[a]))
            R = [[R[r][0] * L[0][c] + R[r][1] * L[1][c] + R[r][2] * L[2][c] for c in range(3)] for r in range(3)]
        for r in range(3):
            for c in range(3):
                frames[:, i, r, c] = _split(R[r][c])
            frames[:, i, r, 3] = _split(t[r] + org[r])
        if i in FK_ROWS:
            k = FK_ROWS.index(i)
            d = [t[r] + org[r] - _MP.mpf(float(pose[k + 1][r])) for r in range(3)]
            dist[:, k] = _split(_MP.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
    return frames, dist


_TRUTH = {}


def truth(fam, kind, pick=None):
    """(frames (2, n, 9, 3, 4), dist (2, n, 4)) of the flattened leg-frames ``pick`` (default: all) of a family; every
    leg-frame is evaluated once per session."""
    L, N = fam["ang"].shape[:2]
    pick = range(L * N) if pick is None else pick
    out = []
    for j in pick:
        key = (fam["name"], kind, j)
        if key not in _TRUTH:
            l, n = divmod(j, N)
            _TRUTH[key] = mp_chain(kind, fam["ang"][l, n], fam["seg"][l], fam["pose"][l, n])
        out.append(_TRUTH[key])
    return np.stack([o[0] for o in out], 1), np.stack([o[1] for o in out], 1)


def scales(fam, pick=None):
    """S of the bound: (frames (n, 9, 3, 4), dist (n, 4))."""
    L, N = fam["ang"].shape[:2]
    seg = np.abs(fam["seg"])
    cum = np.stack([0 * seg[:, 0]] * 4 + [seg[:, 0]] * 2 + [seg[:, :2].sum(1), seg[:, :3].sum(1), seg.sum(1)], 1)   # (L, 9)
    org = np.abs(fam["pose"][:, :, 0]).max(-1)                                                                # (L, N)
    S = np.ones((L, N, 9, 3, 4))
    S[..., 3] = (cum[:, None, :] + org[:, :, None])[..., None]
    Sd = S[:, :, FK_ROWS, 0, 3] + np.linalg.norm(fam["pose"][:, :, 1:] - fam["pose"][:, :, :1], axis=-1)
    S, Sd = S.reshape(L * N, 9, 3, 4), Sd.reshape(L * N, 4)
    return (S, Sd) if pick is None else (S[list(pick)], Sd[list(pick)])


def ratio(got, tr, S):
    """max |got - truth| / (u S); inf when a value that must be finite is not."""
    got = np.asarray(got, dtype=np.float64).reshape(S.shape)
    if not np.isfinite(got).all():
        return np.inf
    err = np.abs((got - tr[0]) - tr[1])
    if (err[S == 0] != 0).any():   # S = 0: rows 0-3 with origin 0, exact in any arithmetic
        return np.inf
    return float((err[S > 0] / (U * S[S > 0])).max())


# ------------------------------------------------------- families ------------------------------------------------------

def _family(name, ang, seg, rng, origin_scale=1.0, zero_origin_upto=0):
    L, N = ang.shape[:2]
    org = rng.standard_normal((L, N, 3)) * origin_scale
    org[:, :zero_origin_upto] = 0.0
    pose = org[:, :, None, :] + rng.standard_normal((L, N, 5, 3))
    pose[:, :, 0] = org
    return dict(name=name, ang=np.ascontiguousarray(ang), seg=np.ascontiguousarray(seg), pose=np.ascontiguousarray(pose))


def _pio2_values():
    ks = list(range(-40, 41)) + [s * k for k in (100, 12345, 2 ** 20, 2 ** 24) for s in (1, -1)]
    out = []
    for k in ks:
        x = float(k) * (np.pi / 2)   # k <= 2^24 and pi / 2 rounded once: the double next to k pi / 2 to within an ulp or two
        for step in (0, 1, 2, 3, -1, -2, -3):
            v = x
            for _ in range(abs(step)):
                v = np.nextafter(v, np.inf if step > 0 else -np.inf)
            out.append(v)
    return np.array(out)


def build_families():
    rng = np.random.default_rng(20261017)
    fams = {}
    seg8 = rng.uniform(0.15, 1.8, (8, 4))
    fams["a"] = _family("a", rng.uniform(-np.pi, np.pi, (3, 130, 7)), seg8[:3], rng, zero_origin_upto=65)
    # b: 8 x 19 leg-frames with every joint unwrapped, then 7 x 32: joint d swept, the others fixed inside [-pi, pi]
    unwrapped = lambda shape: rng.uniform(np.pi, 200 * np.pi, shape) * rng.choice([-1.0, 1.0], shape)  # noqa: E731
    sweep = np.repeat(rng.uniform(-np.pi, np.pi, (7, 1, 7)), 32, axis=1)
    for d in range(7):
        sweep[d, :, d] = np.sort(unwrapped(32))
    b = np.concatenate([unwrapped((152, 7)), sweep.reshape(224, 7)])
    fams["b"] = _family("b", b.reshape(8, 47, 7), seg8, rng)
    vals = _pio2_values()
    j = np.arange(len(vals))
    c = np.stack([vals[(j + 89 * d) % len(vals)] for d in range(7)], 1)
    fams["c"] = _family("c", c[None], seg8[3:4], rng)
    big = np.exp(rng.uniform(np.log(1e3), np.log(ANGLE_MAX), (206, 7))) * rng.choice([-1.0, 1.0], (206, 7))
    for d in range(7):
        big[192 + 2 * d, d], big[193 + 2 * d, d] = ANGLE_MAX, -ANGLE_MAX
    assert np.abs(big).max() == ANGLE_MAX
    fams["d"] = _family("d", big.reshape(2, 103, 7), seg8[4:6], rng)
    tiny = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 1e-300, -1e-300, 1e-9, -1e-9])
    e = np.concatenate([np.stack([tiny[(np.arange(10) + d) % 10] for d in range(7)], 1),
                        np.repeat(rng.uniform(-np.pi, np.pi, (1, 7)), 70, axis=0)])
    for d in range(7):
        e[10 + 10 * d:20 + 10 * d, d] = tiny
    fams["e"] = _family("e", e[None], seg8[6:7], rng)
    g = _family("g", fams["a"]["ang"][:1], seg8[:1], rng, origin_scale=1e6)
    assert 1e5 < np.abs(g["pose"][:, :, 0]).max() < 1e7
    fams["g"] = g
    return fams


BOUND_FAMILIES = ("a", "b", "c", "d", "e", "g")


@pytest.fixture(scope="module")
def fams():
    return build_families()


def scaled(fam, k):
    f = 2.0 ** k
    return dict(name=f"{fam['name']} * 2^{k}", ang=fam["ang"], seg=fam["seg"] * f, pose=fam["pose"] * f)


def h_batches(fam_a):
    """-> clean angles (3, 130, 7), bad angles (15, 3, 130, 7): sequence v holds value OUTSIDE[v], leg l holds it in joint
    H_JOINTS[l] of the leg-frames H_FRAMES; hit (15, 3, 130)."""
    clean = fam_a["ang"]
    bad = np.repeat(clean[None], len(OUTSIDE), axis=0)
    hit = np.zeros(bad.shape[:3], bool)
    for v, val in enumerate(OUTSIDE):
        for l, joint in enumerate(H_JOINTS):
            bad[v, l, list(H_FRAMES), joint] = val
            hit[v, l, list(H_FRAMES)] = True
    return clean, bad, hit


# ------------------------------------------------------- back ends ------------------------------------------------------

class Host:
    """csrc/seqik_fk.hpp and seqik_frames.hpp compiled for the host (tests/harness)."""
    name = "host build"

    def __init__(self, fkh, frh):
        self.fkh, self.frh = fkh, frh

    def fk(self, ang, seg, kind, pose):
        """(S, L, N, 7), (L, 4), pose (S, L, N, 5, 3) -> fk (S, L, N, 9, 3), dist (S, L, N, 4)"""
        S, L, N = ang.shape[:3]
        fk, dist = np.empty((S, L, N, 9, 3)), np.empty((S, L, N, 4))
        for l in range(L):
            f, d = self.fkh.fk(np.ascontiguousarray(ang[:, l]).reshape(-1, 7), seg[l], kind,
                               pose=np.ascontiguousarray(pose[:, l]).reshape(-1, 5, 3), want_dist=True)
            fk[:, l], dist[:, l] = f.reshape(S, N, 9, 3), d.reshape(S, N, 4)
        return fk, dist

    def frames(self, ang, seg, kind, origin):
        S, L, N = ang.shape[:3]
        out = np.empty((S, L, N, 9, 3, 4))
        for l in range(L):
            org = None if origin is None else np.ascontiguousarray(origin[:, l]).reshape(-1, 3)
            out[:, l] = self.frh.frames(np.ascontiguousarray(ang[:, l]).reshape(-1, 7), seg[l], kind,
                                        origin=org).reshape(S, N, 9, 3, 4)
        return out


class Device:
    """The kernels through the C ABI: ``entry`` "host" = seqik_forward_kinematics / seqik_link_frames on host buffers,
    "device" = the _device entry points on torch tensors."""

    def __init__(self, lib, entry):
        self.lib, self.entry, self.name = lib, entry, f"device ({entry} buffers)"

    def _params(self, seg):
        return [self.lib.leg_params_from_arrays(s, np.zeros((7, 2)), np.zeros(27)) for s in seg]

    def fk(self, ang, seg, kind, pose):
        S, L, N = ang.shape[:3]
        if self.entry == "host":
            out = self.lib.forward_kinematics(ang, self._params(seg), kind=kind, pose=pose, want_dist=True)
            return out["fk"], out["dist"]
        import torch
        d_ang, d_pose = torch.from_numpy(np.ascontiguousarray(ang)).cuda(), torch.from_numpy(np.ascontiguousarray(pose)).cuda()
        d_fk = torch.full((S, L, N, 9, 3), 7.0, dtype=torch.float64, device="cuda")
        d_dist = torch.full((S, L, N, 4), 7.0, dtype=torch.float64, device="cuda")
        self.lib.forward_kinematics_device(d_ang.data_ptr(), S, L, N, self._params(seg), d_fk.data_ptr(), kind=kind,
                                           d_pose=d_pose.data_ptr(), d_dist=d_dist.data_ptr(),
                                           stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return d_fk.cpu().numpy(), d_dist.cpu().numpy()

    def frames(self, ang, seg, kind, origin):
        S, L, N = ang.shape[:3]
        if self.entry == "host":
            return self.lib.link_frames(ang, self._params(seg), kind=kind, origin=origin, rows3=True)["frames"]
        import torch
        d_ang = torch.from_numpy(np.ascontiguousarray(ang)).cuda()
        d_org = None if origin is None else torch.from_numpy(np.ascontiguousarray(origin)).cuda()
        d_fr = torch.full((S, L, N, 9, 3, 4), 7.0, dtype=torch.float64, device="cuda")
        self.lib.link_frames_device(d_ang.data_ptr(), S, L, N, self._params(seg), d_fr.data_ptr(), kind=kind,
                                    d_origin=0 if d_org is None else d_org.data_ptr(),
                                    stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return d_fr.cpu().numpy()


@pytest.fixture(scope="module")
def host(fk_harness, frames_harness):  # noqa: F811
    return Host(fk_harness, frames_harness)


def run(be, fam, kind):
    """One family through a back end -> fk (L, N, 9, 3), dist (L, N, 4), frames (L, N, 9, 3, 4); asserts the identity
    translation column == FK rows on the way."""
    fk, dist = be.fk(fam["ang"][None], fam["seg"], kind, fam["pose"][None])
    fr = be.frames(fam["ang"][None], fam["seg"], kind, fam["pose"][None, :, :, 0])
    assert same_bits(fr[..., 3], fk), (be.name, fam["name"], kind)
    return fk[0], dist[0], fr[0]


# -------------------------------------------------------- K_ref --------------------------------------------------------

def _shim():
    sys.path.insert(0, os.path.join(ROOT, "oracle", "shim"))
    try:
        from ikpy.chain import Chain
        from ikpy.link import OriginLink, URDFLink
    finally:
        sys.path.pop(0)
    return Chain, OriginLink, URDFLink


def restatement(fam, kind):
    """The float64 numpy restatement of the reference: IKPy-shaped links and chain of oracle/shim/ikpy, built as
    the reference's KinematicChainSeq / KinematicChainGeneric build them.  -> frames (n, 9, 3, 4), dist (n, 4)."""
    Chain, OriginLink, URDFLink = _shim()
    axes = dict(x=[1, 0, 0], y=[0, 1, 0], z=[0, 0, 1])
    L, N = fam["ang"].shape[:2]
    frames, dist = np.empty((L, N, 9, 3, 4)), np.empty((L, N, 4))
    for l in range(L):
        links = []
        for i, (axis, a, s) in enumerate(SPEC[kind]):
            if i == 0:
                links.append(OriginLink())
            else:
                links.append(URDFLink(name=str(i), origin_translation=[0, 0, 0 if s is None else -fam["seg"][l, s]],
                                      origin_orientation=[0, 0, 0], rotation=axes.get(axis, [0, 0, 0]),
                                      joint_type="revolute"))
        chain = Chain(links)
        dofs = [a for _, a, _ in SPEC[kind][1:8]]
        for n in range(N):
            q = np.concatenate([[0.0], fam["ang"][l, n, dofs], [0.0]])
            full = np.stack(chain.forward_kinematics(q, full_kinematics=True))
            frames[l, n] = full[:, :3, :]
            frames[l, n, :, :, 3] += fam["pose"][l, n, 0]
            dist[l, n] = np.linalg.norm(frames[l, n, FK_ROWS, :, 3] - fam["pose"][l, n, 1:], axis=-1)
    return frames.reshape(L * N, 9, 3, 4), dist.reshape(L * N, 4)


@pytest.fixture(scope="module")
def k_ref_measured(fams):
    worst = {}
    for name in BOUND_FAMILIES:
        S, Sd = scales(fams[name])
        w = 0.0
        for kind in KINDS:
            tr_f, tr_d = truth(fams[name], kind)
            fr, dist = restatement(fams[name], kind)
            w = max(w, ratio(fr, tr_f, S), ratio(dist, tr_d, Sd))
        worst[name] = w
    print("\n[fk accuracy] numpy restatement, worst error / (u S): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    return worst


def test_k_ref_is_measured_on_the_reference_restatement(k_ref_measured):
    # 4 is what the restatement needed when the bound was set (its largest ratio: 2.13); a numpy or libm on which it needs
    # more would loosen every bound of this module, and that must not pass unseen
    assert max(k_ref_measured.values()) <= K_REF
    assert K == 4 * K_REF
    # the bound with this K must still mean something: far below the flat 1e-12 of tests/test_link_frames.py at S ~ 5
    assert K * U * 5 < 1e-14


# -------------------------------------------------------- checks --------------------------------------------------------

def check_bound(be, fam, kind, pick=None):
    fk, dist, fr = run(be, fam, kind)
    n = fk.shape[0] * fk.shape[1]
    idx = list(range(n)) if pick is None else list(pick)
    tr_f, tr_d = truth(fam, kind, pick)
    S, Sd = scales(fam, pick)
    return max(ratio(fr.reshape(n, 9, 3, 4)[idx], tr_f, S), ratio(dist.reshape(n, 4)[idx], tr_d, Sd))


@pytest.mark.parametrize("name", BOUND_FAMILIES)
def test_host_fk_and_frames_inside_the_bound(host, fams, name):
    worst = {KIND_NAMES[kind]: check_bound(host, fams[name], kind) for kind in KINDS}
    print(f"\n[fk accuracy] host build, family {name}, worst error / (u S): " +
          ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f"  (K = {K})")
    assert max(worst.values()) <= K, worst


def test_host_absent_origin_is_origin_zero(host, fams):
    a = fams["a"]
    zero = dict(a, ang=a["ang"][:, :65], pose=a["pose"][:, :65])
    assert not zero["pose"][:, :, 0].any()
    for kind in KINDS:
        with_zero = host.frames(zero["ang"][None], zero["seg"], kind, zero["pose"][None, :, :, 0])
        assert same_bits(host.frames(zero["ang"][None], zero["seg"], kind, None), with_zero)


def check_zero_signs(be, fam, kind):
    """Counted, not asserted: entries where this build and the restatement are both zero with different signs."""
    _, _, fr = run(be, fam, kind)
    ref = restatement(fam, kind)[0].reshape(fr.shape)
    both = (fr == 0) & (ref == 0)
    return int((np.signbit(fr) != np.signbit(ref))[both].sum()), int(both.sum())


def test_host_signed_zero_is_recorded(host, fams, host_harness):  # noqa: F811
    for kind in KINDS:
        diff, zeros = check_zero_signs(host, fams["e"], kind)
        print(f"\n[fk accuracy] host build, family e, {KIND_NAMES[kind]}: {diff} of {zeros} zero entries differ in sign "
              "from the restatement")
    s, c = host_harness.sincos(-0.0)
    print(f"[fk accuracy] sincos_cw(-0.0) = ({s!r}, {c!r}); numpy: ({np.sin(-0.0)!r}, {np.cos(-0.0)!r})")
    assert s == 0.0 and c == 1.0


def check_scaling(be, fam):
    for kind in KINDS:
        fk, dist, fr = run(be, fam, kind)
        for k in (-20, -1, 1, 20):
            fk_k, dist_k, fr_k = run(be, scaled(fam, k), kind)
            assert same_bits(fk_k, fk * 2.0 ** k) and same_bits(dist_k, dist * 2.0 ** k), (be.name, kind, k)
            assert same_bits(fr_k[..., :3], fr[..., :3]), (be.name, kind, k)


def test_host_scaling_by_powers_of_two_is_exact(host, fams):
    check_scaling(host, fams["a"])


def check_large_origin_keeps_the_rotation_blocks(be, fams):
    g, a = fams["g"], fams["a"]
    for kind in KINDS:
        local = be.frames(a["ang"][None, :1], a["seg"][:1], kind, None)
        assert same_bits(run(be, g, kind)[2][..., :3], local[0][..., :3]), (be.name, kind)


def test_host_large_origin_keeps_the_rotation_blocks(host, fams):
    check_large_origin_keeps_the_rotation_blocks(host, fams)


def window_angles(fams):
    return np.concatenate([fams[n]["ang"][..., 0].ravel() for n in "bcde"])


def check_link1_window(be, fams, hh):
    """Link 1 of the sequential chain holds (cos, sin, -sin) of angle 0 as sincos_cw returns them."""
    x = window_angles(fams)
    sc = np.array([hh.sincos(v) for v in x])
    blocks = np.concatenate([run(be, fams[n], 0)[2][:, :, 1, :, :3].reshape(-1, 3, 3) for n in "bcde"])
    assert same_bits(blocks[:, 1, 1], sc[:, 1]) and same_bits(blocks[:, 2, 2], sc[:, 1]), be.name
    assert same_bits(blocks[:, 2, 1], sc[:, 0]), be.name
    # -sin by value: 0 * cos + (-sin) is +0 where sin is +0, and sincos_cw never returns another zero
    assert np.array_equal(blocks[:, 1, 2], -sc[:, 0]) and same_bits(blocks[sc[:, 0] != 0, 1, 2], -sc[sc[:, 0] != 0, 0])
    assert (blocks[:, 0] == (1.0, 0.0, 0.0)).all() and (blocks[:, 1:, 0] == 0.0).all()
    return x, sc


def test_host_link1_is_sincos_cw_and_sincos_cw_is_accurate(host, fams, host_harness):  # noqa: F811
    x, sc = check_link1_window(host, fams, host_harness)
    worst_ulp = worst_abs = 0.0
    for v, (s, c) in zip(x, sc):
        for got, tr in zip((s, c), _mp_sincos(float(v))):
            err = abs(_MP.mpf(float(got)) - tr)
            if abs(v) <= 1e7:
                ulp = np.spacing(abs(float(tr)))
                worst_ulp = max(worst_ulp, float(err / _MP.mpf(float(ulp))))
            else:
                worst_abs = max(worst_abs, float(err))
    print(f"\n[fk accuracy] sincos_cw through link 1, {len(x)} angles: {worst_ulp:.3f} ulp at |x| <= 1e7, "
          f"{worst_abs / U:.3f} * 2^-53 absolute beyond")
    assert (np.abs(x) > 1e7).sum() > 50 and (np.abs(x) <= 1e7).sum() > 1000
    assert worst_ulp <= 1.0 and worst_abs <= U


def check_outside_the_domain(be, fams):
    """Family h.  The sequences of one call hold one value each, the legs one joint each."""
    a = fams["a"]
    clean, bad, hit = h_batches(a)
    V = len(OUTSIDE)
    pose = np.repeat(a["pose"][None], V, axis=0)
    for kind in KINDS:
        fk0, dist0 = be.fk(clean[None], a["seg"], kind, a["pose"][None])
        fr0 = be.frames(clean[None], a["seg"], kind, a["pose"][None, :, :, 0])
        assert np.isfinite(fk0).all() and np.isfinite(dist0).all() and np.isfinite(fr0).all()
        fk, dist = be.fk(bad, a["seg"], kind, pose)
        fr = be.frames(bad, a["seg"], kind, pose[:, :, :, 0])
        for v, val in enumerate(OUTSIDE):
            for l, joint in enumerate(H_JOINTS):
                where = (be.name, KIND_NAMES[kind], f"angle {val!r} in joint {joint}")
                h = hit[v, l]
                assert np.isnan(fk[v, l][h]).all() and np.isnan(dist[v, l][h]).all(), where + (fk[v, l][h][0, 8],)
                assert np.isnan(fr[v, l][h]).all(), where + (fr[v, l][h][0, 1],)
                assert same_bits(fk[v, l][~h], fk0[0, l][~h]) and same_bits(dist[v, l][~h], dist0[0, l][~h]), where
                assert same_bits(fr[v, l][~h], fr0[0, l][~h]), where
        assert np.isnan(fk).sum() == hit.sum() * 27 and np.isnan(dist).sum() == hit.sum() * 4
        assert np.isnan(fr).sum() == hit.sum() * 108


def test_host_angle_outside_the_domain_makes_that_leg_frame_nan(host, fams):
    check_outside_the_domain(host, fams)


def test_host_edge_of_the_domain_is_inside(host, fams):
    """+-2^30 itself is evaluated (family d holds it on every joint and is inside the bound); the next double is not."""
    d = fams["d"]
    assert float(ANGLE_MAX) == 1073741824.0
    text = open(os.path.join(ROOT, "include", "seqik_fk.h")).read()
    assert "#define SEQIK_ANGLE_MAX 1073741824.0" in text
    for kind in KINDS:
        fk, dist, fr = run(host, d, kind)
        assert np.isfinite(fk).all() and np.isfinite(dist).all() and np.isfinite(fr).all()


# ---------------------------------------------------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(hiplib):
    return gpu_lib(hiplib)


@pytest.fixture(scope="module", params=["host", "device"])
def dev(lib, request):
    return Device(lib, request.param)


@pytest.mark.gpu
@pytest.mark.parametrize("name", BOUND_FAMILIES)
def test_gpu_families_equal_the_host_rule_bit_for_bit(dev, host, fams, name):
    for kind in KINDS:
        for got, ref in zip(run(dev, fams[name], kind), run(host, fams[name], kind)):
            assert same_bits(got, ref), (dev.name, name, kind)


@pytest.mark.gpu
def test_gpu_scaling_large_origin_and_link1_window(dev, host, fams, host_harness):  # noqa: F811
    check_scaling(dev, fams["a"])
    for k in (-20, 20):
        for kind in KINDS:
            for got, ref in zip(run(dev, scaled(fams["a"], k), kind), run(host, scaled(fams["a"], k), kind)):
                assert same_bits(got, ref), (dev.name, k, kind)
    check_large_origin_keeps_the_rotation_blocks(dev, fams)
    check_link1_window(dev, fams, host_harness)


@pytest.mark.gpu
@pytest.mark.parametrize("n_legs,n_frames", [(1, 1), (3, 1), (1, 63), (8, 63), (1, 64), (3, 64), (1, 65), (8, 65), (1, 130),
                                              (3, 130), (8, 130)])
def test_gpu_sizes_around_the_tile_equal_the_host_rule(dev, host, fams, n_legs, n_frames):
    """1, 63, 64, 65 and 130 frames with 1, 3 and 8 legs: whole wavefronts, the tail, the four 16-record passes of the
    frames kernel; angles drawn from every family, staged and per-lane kernels."""
    pool = np.concatenate([fams[n]["ang"].reshape(-1, 7) for n in "abcde"])
    poses = np.concatenate([fams[n]["pose"].reshape(-1, 5, 3) for n in "abcde"])
    take = np.random.default_rng(n_legs * 1000 + n_frames).integers(0, len(pool), 2 * n_legs * n_frames)
    ang, pose = pool[take].reshape(2, n_legs, n_frames, 7), poses[take].reshape(2, n_legs, n_frames, 5, 3)
    seg = np.random.default_rng(3).uniform(0.15, 1.8, (8, 4))[:n_legs]
    for kind in KINDS:
        ref_fk, ref_dist = host.fk(ang, seg, kind, pose)
        ref_fr = host.frames(ang, seg, kind, pose[:, :, :, 0])
        for staged in ("1", "0"):
            with switches(SEQIK_FK_STAGED=staged, SEQIK_FRAMES_STAGED=staged):
                fk, dist = dev.fk(ang, seg, kind, pose)
                fr = dev.frames(ang, seg, kind, pose[:, :, :, 0])
            assert same_bits(fk, ref_fk) and same_bits(dist, ref_dist) and same_bits(fr, ref_fr), (dev.name, kind, staged)


@pytest.mark.gpu
def test_gpu_output_inside_the_bound_on_its_own(lib, fams):
    """The bound on what the device returned, not on the host build's bits: 50 leg-frames of each family, 300 in all."""
    dev = Device(lib, "host")
    worst = {}
    for name in BOUND_FAMILIES:
        n = fams[name]["ang"].shape[0] * fams[name]["ang"].shape[1]
        pick = [int(i) for i in np.linspace(0, n - 1, 50).round()]
        if name == "d":
            pick[-14:] = range(192, 206)   # the leg-frames that hold +-2^30
        worst[name] = max(check_bound(dev, fams[name], kind, pick) for kind in KINDS)
    print(f"\n[fk accuracy] device, 50 leg-frames per family, worst error / (u S): " +
          ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f"  (K = {K})")
    assert max(worst.values()) <= K, worst


@pytest.mark.gpu
def test_gpu_angle_outside_the_domain_makes_that_leg_frame_nan(dev, fams):
    check_outside_the_domain(dev, fams)


@pytest.mark.gpu
def test_gpu_outside_the_domain_in_one_wavefront_and_through_the_python_entries(lib, fams):
    """One recording of 130 frames, one leg: the hit records are 0, 15, 16, 63, 64 and 129 of the launch itself, so their
    neighbours in the 16-record pass and in the four-lane group are the leg-frames compared with the clean run."""
    a = fams["a"]
    ang0, seg, pose = a["ang"][None, :1], a["seg"][:1], a["pose"][None, :1]
    params = [lib.leg_params_from_arrays(seg[0], np.zeros((7, 2)), np.zeros(27))]
    hit = np.zeros(H_N, bool)
    hit[list(H_FRAMES)] = True
    for kind in KIND_NAMES:
        clean = lib.forward_kinematics(ang0, params, kind=kind, pose=pose, want_dist=True)
        clean_fr = lib.link_frames(ang0, params, kind=kind, origin=pose[..., 0, :])["frames"]
        for val in (np.nextafter(ANGLE_MAX, np.inf), -3.38e9, 1e300, -np.inf, np.nan):
            for joint in H_JOINTS:
                bad = ang0.copy()
                bad[0, 0, hit, joint] = val
                out = lib.forward_kinematics(bad, params, kind=kind, pose=pose, want_dist=True)
                fr = lib.link_frames(bad, params, kind=kind, origin=pose[..., 0, :])["frames"]
                assert np.isnan(out["fk"][0, 0, hit]).all() and np.isnan(out["dist"][0, 0, hit]).all(), (kind, val, joint)
                assert np.isnan(fr[0, 0, hit]).all() and fr.shape == (1, 1, H_N, 9, 4, 4), (kind, val, joint)
                assert same_bits(out["fk"][0, 0, ~hit], clean["fk"][0, 0, ~hit]), (kind, val, joint)
                assert same_bits(out["dist"][0, 0, ~hit], clean["dist"][0, 0, ~hit]), (kind, val, joint)
                assert same_bits(fr[0, 0, ~hit], clean_fr[0, 0, ~hit]), (kind, val, joint)


@pytest.mark.gpu
def test_gpu_chain_forward_kinematics_many_outside_the_domain(lib, fams):
    """Joint 0 and 3 through the stage-1 chain, joint 6 through the stage-4 chain (its other links are fixed), all three
    through the generic chain."""
    from seqikpy_amd.kinematic_chain import KinematicChainGeneric, KinematicChainSeq
    dofs = ["ThC_yaw", "ThC_pitch", "ThC_roll", "CTr_pitch", "CTr_roll", "FTi_pitch", "TiTa_pitch"]
    body = {f"RF_{s}": float(v) for s, v in zip(["Coxa", "Femur", "Tibia", "Tarsus"], fams["a"]["seg"][0])}
    bounds = {f"RF_{d}": (-np.pi, np.pi) for d in dofs}
    seq, gen = KinematicChainSeq(bounds, ["RF"], body), KinematicChainGeneric(bounds, ["RF"], body)
    prior = {f"Angle_RF_{d}": fams["a"]["ang"][0, :1, i] for i, d in enumerate(dofs)}
    cases = [(seq.create_leg_chain("RF", stage=1), (1, 3)), (seq.create_leg_chain("RF", stage=4, angles=prior, t=0), (7,)),
             (gen.create_leg_chain("RF"), (1, 4, 7))]
    hit = np.zeros(H_N, bool)
    hit[list(H_FRAMES)] = True
    for chain, links in cases:
        q = np.zeros((H_N, len(chain.links)))
        q[:, 1:-1] = fams["a"]["ang"][0][:, :len(chain.links) - 2]
        if chain.name == "chain_stage_1":
            q[:, -1] = fams["a"]["ang"][0][:, 3]
        assert chain._whole_leg_angles(q) is not None
        clean = chain.forward_kinematics_many(q)
        assert clean.shape == (H_N, len(chain.links), 4, 4) and np.isfinite(clean).all()
        for val in (np.nextafter(ANGLE_MAX, np.inf), 3.38e9, -1e18, np.inf, np.nan):
            for link in links:
                bad = q.copy()
                bad[hit, link] = val
                out = chain.forward_kinematics_many(bad)
                assert np.isnan(out[hit]).all(), (chain.name, val, link)
                assert same_bits(out[~hit], clean[~hit]), (chain.name, val, link)
