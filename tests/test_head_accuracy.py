"""Head / antenna angles against an extended-precision yardstick; NaN in, NaN out.

The arithmetic of csrc/seqik_head.hpp that matters -- ``inv_sqrt`` / ``inv`` from the hardware seeds plus Newton steps,
the branch-free ``acos_unit`` -- exists only in the device build; the host harness compiles ``1 / sqrt(v)`` and ``1 / q``
in their place.  So the same checks run twice: on the host builds (CPU tier: the rule's structure, the NaN behaviour,
``K_ref``) and through ``_lib.signed_angles`` / ``head_angles`` / ``head_angles_raw`` on the device (``-m gpu``).

YARDSTICK.  ``truth_signed``: the signed angle of two 3-vectors about an axis as ``atan2(|v1 x v2|, v1 . v2)`` in
``np.longdouble`` (eps 1.08e-19 where this was written; float64 where a machine's long double is no wider -- the form
that ran is printed), negative unless ``axis . (v1 x v2) > 0``; NaN for a zero-length or non-finite vector (atan2 alone
would answer 0 or pi/4 there).  ``truth_head`` builds the seven angles from it exactly as oracle/head_oracle.py builds
them from ``signed_angle``.  atan2 is well conditioned at 0 and pi, where acos is not.

BOUND.  u = 2^-53.  A cosine off by K u moves the angle by K u / sin(theta), saturating at sqrt(2 K u) at the ends:

    |got - truth| <= K u (1 + 1 / max(|sin theta|, sqrt(K u)))            theta: the signed angle before any offset

``K_ref`` is the smallest power of two for which the numpy float64 restatement of the reference's own formula
(head_oracle.signed_angle / head_angles) stays inside that envelope on this module's finite inputs (families a-c); rows on
which the restatement itself returns NaN because its cosine overshoots 1 by an ulp are left out and counted.  The tests
use K = 4 K_ref: a factor 2 for the documented 2-ulp ``acos_unit``, a factor 2 for the fused normalisation and the
Newton seeds against numpy's correctly rounded division and square root.  K is never read off the code under test.
Where the signed angle is within 1e-6 of +-pi its sign hangs on the rounding of a determinant that is zero in exact
arithmetic (the reference's as much as the kernel's), so there -- and only there -- a difference of 2 pi counts as none.

INPUT FAMILIES (seeded, built here)
  a. acos domain through ``signed_angles``: v2 = v1 turned by theta about a perpendicular axis, lengths in [0.1, 10];
     theta log-spaced 1e-12 .. 1 from 0 and from pi, uniform between; per-row v1 (200 000 pairs) and one broadcast v1
     (100 000); exact parallel / antiparallel / orthogonal pairs, cosines of exactly +-0.5 and their float neighbours
     (both sides of the small / big select of ``acos_unit``); the three coordinate axes and an oblique one.
  b. head frames: synthetic heads turned by roll / pitch / yaw from {0, +-pi/2, +-(pi - 1e-9), +-1e-9, ...} and at
     random, antenna poses that are parallel / antiparallel to the horizontal vector after derotation; the neck fixed
     and per frame; the 6000 fixture frames.  Own roll, given roll, without the antennae.
  c. family b times 2^k, k in {-100, -50, -10, 10, 50, 100}: every operation of the rule scales exactly, so the angles
     equal the unscaled run bit for bit (asserted as equality of bits; 2^+-100 is the documented magnitude range).
  d. NaN, +inf, -inf in each of the 15 input coordinates, NaN in the caller's head roll, zero vectors (L base = R base,
     tip = base on either side, neck = an antenna base, mid with zero (x, z)), at several positions of full wavefronts
     and of the tail of a launch of 64 m + r frames.  An output is NaN exactly where head_oracle.head_angles is NaN on
     that input and the yardstick is not finite; every other output equals the bits of the run without the injection.
     A zero-vector case moves a key point, so the outputs that READ it (``D_READS``, per case; checked to be the outputs on
     which head_oracle.head_angles differs between the clean and the edited input) cannot keep the clean bits: they are
     NaN where expected, else inside the envelope at the same K -- the head pitch with an input-conditioning term
     (``_pitch_input_term``) next to it, since the neck put on a base leaves mid = (rb + lb) / 2 - neck short against the
     rounded sum.  Every output of the edited frame that does not read the moved point keeps the clean run's bits.

MEASURED (EXPERIMENTS.md, "Head accuracy"; the tests print the figures, ``-s``).  K_ref = 8, K = 32; 17 388 overshoot
rows of the restatement left out; its 166 980 antenna angles with the frame's OWN roll are not used for K_ref either (it
derotates by cos / sin of an acos-derived roll and inherits that roll's 1 / sin(roll), up to 6e-9 rad: the conditioning
of the reference's chain, not of the rule, which is held to the envelope on those rows all the same).  Worst error /
envelope(K = 32), host build: family a 0.500 (per-row), 0.500 (broadcast), 0.036 (exact); family b 0.354, 0.354, 0.101
(fixture); family c bit-equal.  Device: not measured when this was written.
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, HostHarness, host_harness, load_golden  # noqa: F401  (fixture: the head rule run on the host)
from test_head_alignment import (HeadAlignHarness, aligner, fixture_raw, head_align_harness,  # noqa: F401
                                 rest_pitches)

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import head_oracle  # noqa: E402

LD = np.longdouble if np.finfo(np.longdouble).eps < 1e-18 else np.float64
FORM = "atan2 in np.longdouble (eps %.3g)" % np.finfo(LD).eps if LD is not np.float64 else "atan2 in float64"
U = 2.0 ** -53
PI = 4 * np.arctan(LD(1))
AXES = [np.eye(3)[0], np.eye(3)[1], np.eye(3)[2], np.array([0.3, -0.5, 0.7])]
SCALES = (-100, -50, -10, 10, 50, 100)
IDENTITY = ((np.zeros(3), 1.0, 1.0, np.zeros(3)),) * 2


# ------------------------------------------------------ yardstick ------------------------------------------------------

def truth_signed(v1, v2, axis):
    v1 = np.atleast_2d(np.asarray(v1, dtype=np.float64)).astype(LD)
    v2 = np.atleast_2d(np.asarray(v2, dtype=np.float64)).astype(LD)
    n = max(len(v1), len(v2))
    v1, v2 = np.broadcast_to(v1, (n, 3)), np.broadcast_to(v2, (n, 3))
    axis = np.asarray(axis, dtype=np.float64).astype(LD)
    with np.errstate(all="ignore"):
        cr = np.stack([v1[:, 1] * v2[:, 2] - v1[:, 2] * v2[:, 1], v1[:, 2] * v2[:, 0] - v1[:, 0] * v2[:, 2],
                       v1[:, 0] * v2[:, 1] - v1[:, 1] * v2[:, 0]], axis=1)
        dot = (v1 * v2).sum(1)
        ang = np.arctan2(np.sqrt((cr * cr).sum(1)), dot)
        det = (cr * axis).sum(1)
        bad = ~(np.isfinite(v1).all(1) & np.isfinite(v2).all(1)) | ((v1 * v1).sum(1) == 0) | ((v2 * v2).sum(1) == 0)
    return np.where(bad, LD(np.nan), np.where(det > 0, ang, -ang))


def _derot(roll, v):
    with np.errstate(all="ignore"):
        c, s = np.cos(roll), np.sin(roll)
        return np.stack([v[:, 0], c * v[:, 1] + s * v[:, 2], -s * v[:, 1] + c * v[:, 2]], axis=1)


def _zeroed(v, a):
    v = v.copy()
    v[:, a] = 0
    return v


def truth_head(r_head, l_head, neck, rest, head_roll=None, compute_ant=True):
    """-> (final (7 or 3, N), raw (7 or 3, N)): the angles, and the signed angle each one is an offset of."""
    r_head, l_head = np.asarray(r_head, dtype=np.float64).astype(LD), np.asarray(l_head, dtype=np.float64).astype(LD)
    neck = np.asarray(neck, dtype=np.float64).reshape(-1, 3).astype(LD)
    X, Y, Z = np.eye(3)
    with np.errstate(all="ignore"):
        rb, lb = r_head[:, 0], l_head[:, 0]
        hor, mid = lb - rb, (rb + lb) * LD(0.5) - neck
        roll = truth_signed(Y, _zeroed(hor, 0), X)
        pitch = truth_signed(X, _zeroed(mid, 1), Y)
        yaw = truth_signed(Y, _zeroed(hor, 2), Z)
        raw, final = [roll, pitch, yaw], [roll, pitch + LD(rest[0]), yaw]
        if compute_ant:
            if head_roll is not None:
                roll = np.broadcast_to(np.asarray(head_roll, dtype=np.float64).reshape(-1), roll.shape).astype(LD)
            hor_d = _derot(roll, hor)
            for side, head in (("L", l_head), ("R", r_head)):
                ant, hv = _derot(roll, head[:, 1] - head[:, 0]), _derot(roll, neck - head[:, 0])
                ayaw = truth_signed(_zeroed(ant, 0), _zeroed(hor_d, 0), X)
                apitch = truth_signed(_zeroed(hv, 1), _zeroed(ant, 1), Y)
                raw += [ayaw, apitch]
                final += [PI - ayaw if side == "R" else ayaw, apitch - LD(rest[1])]
    return np.stack(final), np.stack(raw)


def envelope(theta, K):
    ku = K * U
    return ku * (1.0 + 1.0 / np.maximum(np.abs(np.sin(np.asarray(theta, dtype=np.float64))), np.sqrt(ku)))


def error(got, final, raw):
    """|got - truth| as float64; near the +-pi seam of the signed angle a difference of 2 pi counts as none."""
    with np.errstate(all="ignore"):
        err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - final)
        seam = np.abs(raw) > PI - LD(1e-6)
        err = np.where(seam, np.minimum(err, np.abs(err - 2 * PI)), err)
    return err.astype(np.float64)


def worst_ratio(got, final, raw, K):
    """max over the finite-truth entries of error / envelope; inf when an entry that should be finite is not."""
    got, ok = np.asarray(got, dtype=np.float64), np.isfinite(final.astype(np.float64))
    if not np.isfinite(got[ok]).all():
        return np.inf
    ratio = error(got, final, raw)[ok] / envelope(raw.astype(np.float64)[ok], K)
    return float(ratio.max()) if ratio.size else 0.0


# ------------------------------------------------------- families ------------------------------------------------------

def _unit(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def _clear_axes(rng, n, v1=None):
    """n unit vectors k whose components along every test axis are clear of zero, so that the sign of
    det = axis . (v1 x v2) (v1 x v2 runs along k) does not hang on rounding; perpendicular to ``v1`` (3,) when given."""
    out = np.zeros((0, 3))
    while len(out) < n:
        k = rng.normal(size=(2 * n, 3))
        k = _unit(k if v1 is None else np.cross(v1, k))
        out = np.concatenate([out, k[np.all([np.abs(k @ _unit(a)) > 0.05 for a in AXES], axis=0)]])
    return out[:n]


def _turned(rng, v1, k, n):
    """v2 = v1 turned by theta about the perpendicular axis k (built in LD, rounded once), random lengths."""
    third = n // 3
    t_log = 10.0 ** np.linspace(-12, 0, third)
    theta_small = np.concatenate([t_log, t_log, rng.uniform(1e-3, np.pi - 1e-3, n - 2 * third)]).astype(LD)
    from_pi = np.zeros(n, dtype=bool)
    from_pi[third:2 * third] = True
    d1 = _unit(np.broadcast_to(v1, (n, 3)).astype(LD))
    k = k.astype(LD)
    kx = np.cross(k.astype(np.float64), d1.astype(np.float64)).astype(LD)   # direction only: any vector close to k x d1 will do
    c, s = np.cos(theta_small), np.sin(theta_small)
    c = np.where(from_pi, -c, c)          # theta = pi - t: cos = -cos t, sin = sin t (no pi - t rounding)
    v2 = (d1 * c[:, None] + kx * s[:, None]) * rng.uniform(0.1, 10.0, n).astype(LD)[:, None]
    return v2.astype(np.float64)


def _exact_pairs():
    """Pairs with exactly representable components: cosines of exactly 1, -1, 0, +-0.5 and the float neighbours of +-0.5."""
    v1, v2 = [], []
    for a in ([1.0, 2.0, 2.0], [0.5, -0.25, 4.0], [3.0, 0.0, 4.0]):
        for f in (1.0, 2.0, 0.375, -1.0, -2.0, -0.375):      # parallel and antiparallel
            v1.append(a), v2.append([f * x for x in a])
    for a, b in (([1.0, 0, 0], [0, 1.0, 0]), ([0, 0, 2.0], [3.0, 0, 0]), ([1.0, 2.0, 2.0], [2.0, 1.0, -2.0]), ([1.0, 1.0, 0], [1.0, -1.0, 8.0])):
        v1.append(a), v2.append(b)                           # orthogonal
    for sgn in (1.0, -1.0):                                  # (1,1,0) . (1,0,1) = 1, |.||.| = 2: cosine exactly 1/2
        for k in range(-8, 9):
            v1.append([1.0, 1.0, 0.0]), v2.append([sgn * (1.0 + k * 2.0 ** -52), 0.0, sgn * 1.0])
            v1.append([1.0 + k * 2.0 ** -52, 1.0, 0.0]), v2.append([sgn * 1.0, 0.0, sgn * 1.0])
    return np.array(v1), np.array(v2)


@pytest.fixture(scope="module")
def fam_a():
    """[(name, v1 (n, 3) or (3,), v2 (n, 3))]"""
    rng = np.random.default_rng(20260)
    n = 200_000
    k = _clear_axes(rng, n)
    v1 = _unit(np.cross(k, rng.normal(size=(n, 3)))) * rng.uniform(0.1, 10.0, (n, 1))
    one = np.array([0.6, -1.1, 0.8])
    e1, e2 = _exact_pairs()
    return [("per-row", v1, _turned(rng, v1, k, n)), ("broadcast", one, _turned(rng, one, _clear_axes(rng, 100_000, one), 100_000)),
            ("exact", e1, e2)]


def _rot(roll, pitch, yaw):
    """Rz(yaw) Ry(pitch) Rx(roll) per frame, (n, 3, 3) in LD; an angle of exactly 0 gives exact 1 / 0 entries."""
    roll, pitch, yaw = (np.asarray(a, dtype=np.float64).astype(LD) for a in (roll, pitch, yaw))
    n = len(roll)
    m = np.zeros((3, n, 3, 3), dtype=LD)
    for i, (a, (p, q)) in enumerate(((roll, (1, 2)), (pitch, (2, 0)), (yaw, (0, 1)))):
        m[i, :, 0, 0] = m[i, :, 1, 1] = m[i, :, 2, 2] = 1
        c, s = np.cos(a), np.sin(a)
        m[i, :, p, p], m[i, :, q, q], m[i, :, p, q], m[i, :, q, p] = c, c, -s, s
    return m[2] @ m[1] @ m[0]


ANT_POSES = np.array([[0.3, 0.1, -0.2], [0.3, -0.1, -0.2], [0.2, 0.5, 0.0], [0.2, -0.5, 0.0], [0.3, 0.0, -0.4],
                      [-0.1, 0.2, 0.3]])          # rows 2, 3: parallel / antiparallel to the horizontal vector (0, 2w, 0)
SPECIAL = np.array([0.0, np.pi / 2, -np.pi / 2, np.pi - 1e-9, -(np.pi - 1e-9), 1e-9, -1e-9, 0.3, -1.1, 2.5])


def _synthetic_heads(rng, n_random, neck_offset):
    """(R base, R tip, L base, L tip) of a head about a neck at the origin, turned by roll / pitch / yaw; with
    ``neck_offset`` every frame is then shifted by a small per-frame neck.  Frames on which a projected vector of the
    antenna pitch all but vanishes after the derotation (|projection| < 0.1 |vector|: the cancellation then amplifies
    the rounding of the reference and of the rule alike) are left out; the named edges are asserted to survive."""
    g = np.stack(np.meshgrid(SPECIAL, SPECIAL, SPECIAL, indexing="ij"), -1).reshape(-1, 3)
    # pure rolls with every pairing of the parallel / antiparallel antenna poses (the derotation removes the roll alone)
    pure = np.array([[a, 0.0, 0.0] for a in SPECIAL for _ in range(4)])
    ang = np.concatenate([g, pure, rng.uniform(-np.pi, np.pi, (n_random, 3))])
    n = len(ang)
    pose_r, pose_l = rng.integers(0, 6, n), rng.integers(0, 6, n)
    pose_r[len(g):len(g) + len(pure)] = np.tile([2, 2, 3, 3], len(SPECIAL))
    pose_l[len(g):len(g) + len(pure)] = np.tile([2, 3, 2, 3], len(SPECIAL))
    rot = _rot(ang[:, 0], ang[:, 1], ang[:, 2])
    pts = np.zeros((n, 4, 3))
    pts[:, 0], pts[:, 2] = [0.4, -0.3, 0.2], [0.4, 0.3, 0.2]
    pts[:, 1] = pts[:, 0] + ANT_POSES[pose_r] * [1, -1, 1]     # the right antenna mirrored
    pts[:, 3] = pts[:, 2] + ANT_POSES[pose_l]
    pts = np.einsum("nij,nkj->nki", rot, pts.astype(LD)).astype(np.float64)
    neck = np.zeros((n, 3))
    if neck_offset:
        neck = rng.uniform(-0.05, 0.05, (n, 3))
        pts = pts + neck[:, None, :]
    r, l = pts[:, :2], pts[:, 2:]
    return r, l, neck, ang


def _well_conditioned(r, l, neck, head_roll=None):
    """False where a projected (z, x) vector of the antenna pitch, or the projected mid vector, is short against its
    3-vector (float64 is plenty to decide that)."""
    hor = l[:, 0] - r[:, 0]
    roll = head_oracle.signed_angle(np.eye(3)[1], _zeroed(hor, 0), np.eye(3)[0]) if head_roll is None else head_roll
    ok = (np.hypot(hor[:, 1], hor[:, 2]) > 0) & (np.hypot(hor[:, 0], hor[:, 1]) > 0)   # (a zero projection is family d's)
    mid = (r[:, 0] + l[:, 0]) * 0.5 - neck
    ok &= np.hypot(mid[:, 0], mid[:, 2]) > 0.1 * np.abs(np.stack([r[:, 0], l[:, 0], neck], 1)).max((1, 2))
    for head in (r, l):
        for v in (head[:, 1] - head[:, 0], neck - head[:, 0]):
            d = head_oracle.derotate(roll, v)
            ok &= np.hypot(d[:, 0], d[:, 2]) > 0.1 * np.linalg.norm(v, axis=1)
    return ok


@pytest.fixture(scope="module")
def rest():
    z = load_golden("anipose_head")
    return float(z["rest_head_pitch"][0]), float(z["rest_antenna_pitch"][0])


DROPPED = {}      # family b member -> (frames the conditioning filter dropped, frames generated)


@pytest.fixture(scope="module")
def fam_b():
    """[(name, r (n, 2, 3), l, neck (3,) or (n, 3), given roll (n,), Euler angles or None)]"""
    rng = np.random.default_rng(20261)
    out = []
    for name, offset in (("synthetic, neck at the origin", False), ("synthetic, neck per frame", True)):
        r, l, neck, ang = _synthetic_heads(rng, 3000, offset)
        given = np.where(np.arange(len(r)) % 5 == 0, rng.choice([0.0, np.pi / 2, -np.pi / 2], len(r)),
                         rng.uniform(-np.pi, np.pi, len(r)))
        keep = _well_conditioned(r, l, neck)
        given = np.where(_well_conditioned(r, l, neck, given), given, 0.0)
        keep &= _well_conditioned(r, l, neck, given)
        print(f"\n[head accuracy] family b, {name}: {int(keep.sum())} of {len(keep)} frames kept, {int((~keep).sum())} "
              "ill-conditioned ones dropped")
        DROPPED[name] = (int((~keep).sum()), len(keep))
        out.append((name, r[keep], l[keep], neck[keep] if offset else np.zeros(3), given[keep], ang[keep]))
    z = load_golden("anipose_head")
    own = head_oracle.head_angles(z["R_head"], z["L_head"], z["Neck"][:, 0], 0.0, 0.0)[0]
    out.append(("fixture", z["R_head"], z["L_head"], z["Neck"][0, 0].copy(), own + 0.3, None))
    return out


def test_families_hold_the_named_edges(fam_a, fam_b):
    """What the generators promise (and the filter on ill-conditioned frames must not have removed)."""
    for name, v1, v2 in fam_a[:2]:
        t = np.abs(truth_signed(v1, v2, AXES[3]).astype(np.float64))
        assert t.min() < 1.1e-12 and np.pi - t.max() < 1.1e-12 and len(v2) >= 100_000, name
    assert len(fam_a[0][2]) >= 200_000
    _, e1, e2 = fam_a[2]
    cos = np.einsum("ij,ij->i", e1, e2) / np.sqrt(np.einsum("ij,ij->i", e1, e1) * np.einsum("ij,ij->i", e2, e2))
    for target in (0.5, -0.5):
        near = cos[np.abs(cos - target) < 1e-12]
        assert (near == target).any() and (np.abs(near) < 0.5).any() and (np.abs(near) > 0.5).any()   # both sides of the select
    assert (cos == 1).any() and (cos == -1).any() and (cos == 0).any()
    for name, r, l, neck, given, ang in fam_b[:2]:
        hor = l[:, 0] - r[:, 0]
        assert ((hor[:, 0] == 0) & (hor[:, 2] == 0) & (hor[:, 1] > 0)).any(), name      # hor exactly along Y: cosine exactly 1
        for col in range(3):
            for v in (0.0, np.pi / 2, -np.pi / 2, np.pi - 1e-9, -(np.pi - 1e-9)):
                assert (ang[:, col] == v).any(), (name, col, v)
        raw = truth_head(r, l, neck, (0.0, 0.0))[1].astype(np.float64)
        assert (np.pi - np.abs(raw[0]) < 2e-9).any() and (np.pi - np.abs(raw[2]) < 2e-9).any(), name   # roll, yaw at +-pi
        assert (np.abs(raw[3]) < 1e-9).any() and (np.pi - np.abs(raw[3]) < 1e-9).any(), name           # antenna || / anti-|| hor
        assert (np.abs(raw[5]) < 1e-9).any() and (np.pi - np.abs(raw[5]) < 1e-9).any(), name
        # the filter is deterministic (seeded): 4040 frames generated, 74 and 91 of them dropped when this was written (EXPERIMENTS.md); a
        # change of the generator that drops more than one frame in twenty -- the hard frames, quietly -- shows here
        assert len(r) > 2500 and DROPPED[name][1] == 4040 and DROPPED[name][0] <= 0.05 * 4040, (name, DROPPED[name])


# ------------------------------------------------- K_ref from the reference ---------------------------------------------

def _scaled(member, k):
    name, r, l, neck, given, ang = member
    s = 2.0 ** k
    return (f"{name} x 2^{k}", r * s, l * s, neck * s, given, ang)


@pytest.fixture(scope="module")
def bound(fam_a, fam_b, rest):
    """K_ref: the numpy float64 restatement of the reference's formula against the yardstick on families a-c."""
    cases, chained = [], 0      # (got by the restatement, final, raw, label)
    with np.errstate(all="ignore"):
        for name, v1, v2 in fam_a:
            for axis in AXES:
                t = truth_signed(v1, v2, axis)
                cases.append((head_oracle.signed_angle(v1, v2, axis), t, t, f"a {name}"))
        for member in fam_b + [_scaled(m, k) for m in fam_b for k in (SCALES[0], SCALES[-1])]:
            name, r, l, neck, given, _ = member
            for roll in (None, given):
                g = head_oracle.head_angles(r, l, neck, *rest, head_roll=roll)
                if roll is None:
                    # The reference derotates by cos / sin of its own acos-derived roll, so its antenna angles inherit the
                    # roll's 1 / sin(roll) (up to 1e-8 rad at a roll of 0 or pi) on top of their own: a conditioning
                    # problem of the reference's chain of two acos that the rule (normalised components) does not have.
                    # Those rows say nothing about K; the rule is still held to the envelope on them.
                    chained += g[3:].size
                    g = g[:3]
                f, raw = truth_head(r, l, neck, rest, roll)
                cases.append((g, f[:len(g)], raw[:len(g)], f"b/c {name}, {'own' if roll is None else 'given'} roll"))
    overshoot = sum(int((np.isnan(g) & np.isfinite(f.astype(np.float64))).sum()) for g, f, _, _ in cases)
    k_ref = 1
    while True:
        worst, where = 0.0, ""
        for g, f, raw, label in cases:
            ok = np.isfinite(g) & np.isfinite(f.astype(np.float64))
            ratio = error(g, f, raw)[ok] / envelope(raw.astype(np.float64)[ok], k_ref)
            if float(ratio.max()) > worst:
                i = int(ratio.argmax())
                worst, where = float(ratio.max()), f"{label}, entry {tuple(np.argwhere(ok)[i])}: truth {float(f[ok][i])!r}, restatement {float(g[ok][i])!r}"
        if worst <= 1.0:
            break
        k_ref *= 2
        assert k_ref <= 2 ** 20, "the restatement of the reference does not fit the envelope at any sensible K"
    print(f"\n[head accuracy] yardstick: {FORM}; K_ref = {k_ref} (worst ratio {worst:.3f}), K = {4 * k_ref}; "
          f"{overshoot} reference-overshoot rows left out; {chained} own-roll antenna angles of the reference not used; "
          f"worst row: {where}")
    return dict(k_ref=k_ref, K=4 * k_ref, overshoot=overshoot)


def test_k_ref_is_measured_on_the_reference_restatement(bound):
    # 8 is what the restatement needed when the bound was set (EXPERIMENTS.md, "Head accuracy"); a numpy or libm on which it
    # needs more would loosen every bound of this module, and that must not pass unseen
    assert bound["K"] == 4 * bound["k_ref"] and 1 <= bound["k_ref"] <= 8
    # the envelope with this K must still mean something: below the flat 1e-6 of tests/test_head.py everywhere
    assert envelope(0.0, bound["K"]) < 1e-6


# ------------------------------------------------------- back ends ------------------------------------------------------

class Host:
    name = "host build"

    def __init__(self, hh, hah):
        self.hh, self.hah = hh, hah

    def signed(self, v1, v2, axis):
        return self.hh.signed_angles(v1, v2, axis)

    def head(self, r, l, neck, rest, compute_ant=True, head_roll=None):
        out = self.hh.head_angles(r, l, neck, rest[0], rest[1], compute_ant=compute_ant, head_roll=head_roll)
        return out if compute_ant else out[:3]

    def raw(self, r, l, neck, rest, affine, compute_ant=True, head_roll=None):
        return self.hah.angles_raw(r, l, neck, rest, affine, compute_ant=compute_ant, roll=head_roll)[0]


class Device:
    name = "device"

    def __init__(self, lib):
        self.lib = lib

    def signed(self, v1, v2, axis):
        return self.lib.signed_angles(v1, v2, axis)

    def head(self, r, l, neck, rest, compute_ant=True, head_roll=None):
        return self.lib.head_angles(r, l, neck, rest[0], rest[1], compute_ant=compute_ant, head_roll=head_roll)

    def raw(self, r, l, neck, rest, affine, compute_ant=True, head_roll=None):
        return self.lib.head_angles_raw(r, l, neck, rest[0], rest[1], affine, compute_ant=compute_ant, head_roll=head_roll)


@pytest.fixture(scope="module")
def host(host_harness, head_align_harness):  # noqa: F811
    return Host(host_harness, head_align_harness)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_bits_or_both_nan(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(a, b, equal_nan=True) and \
        np.array_equal(np.signbit(a)[~np.isnan(a)], np.signbit(b)[~np.isnan(b)])


# -------------------------------------------------------- checks --------------------------------------------------------

def check_family_a(be, fam_a, K):
    worst = {}
    for name, v1, v2 in fam_a:
        for axis in AXES:
            t = truth_signed(v1, v2, axis)
            got = be.signed(v1, v2, axis)
            assert np.isfinite(got).all(), (be.name, name)
            worst[name] = max(worst.get(name, 0.0), worst_ratio(got, t, t, K))
    print(f"\n[head accuracy] {be.name}, family a, worst error / envelope(K = {K}): " +
          ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    return worst


def head_variants(be, member, rest, extra=()):
    """The runs of one recording: own roll, without the antennae, given roll; the fused rule with the identity map.
    -> {variant: angles}; asserts the bit equalities between them."""
    name, r, l, neck, given, _ = member
    own = be.head(r, l, neck, rest)
    three = be.head(r, l, neck, rest, compute_ant=False)
    rolled = be.head(r, l, neck, rest, head_roll=given)
    assert own.shape == (7, len(r)) and three.shape == (3, len(r))
    assert same_bits_or_both_nan(three, own[:3]) and same_bits_or_both_nan(rolled[:3], own[:3]), (be.name, name)
    # fused map + angles against the plain rule: the identity map hands the rule the same key points
    assert same_bits_or_both_nan(be.raw(r, l, neck, rest, IDENTITY), own), (be.name, name)
    assert same_bits_or_both_nan(be.raw(r, l, neck, rest, IDENTITY, compute_ant=False), three), (be.name, name)
    assert same_bits_or_both_nan(be.raw(r, l, neck, rest, IDENTITY, head_roll=given), rolled), (be.name, name)
    for fn in extra:
        fn(member, own, three, rolled)
    return dict(own=own, rolled=rolled)


def check_family_b(be, fam_b, rest, K, extra=()):
    worst = {}
    for member in fam_b:
        name, r, l, neck, given, _ = member
        runs = head_variants(be, member, rest, extra)
        w = worst_ratio(runs["own"], *truth_head(r, l, neck, rest), K)
        w = max(w, worst_ratio(runs["rolled"], *truth_head(r, l, neck, rest, given), K))
        worst[name] = w
    print(f"\n[head accuracy] {be.name}, family b, worst error / envelope(K = {K}): " +
          ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    return worst


def check_family_c(be, fam_b, rest, extra=()):
    for member in fam_b:
        base = head_variants(be, member, rest)
        assert np.isfinite(base["own"]).all() and np.isfinite(base["rolled"]).all()
        for k in SCALES:
            runs = head_variants(be, _scaled(member, k), rest, extra)
            for v in base:
                assert same_bits(runs[v], base[v]), (be.name, member[0], k, v)


# family d: one recording of 64 m + r frames, one launch per case, the case applied at every position of POSITIONS
N_D, POSITIONS = 64 * 3 + 37, (5, 63, 64, 130, 195, 228)   # 195, 228: the tail wavefront (per-lane loads)


def _d_cases():
    """[(name, fn(r, l, neck, roll, p))]: fn edits frame p in place."""
    cases = []
    for arr, point, label in ((0, 0, "R base"), (0, 1, "R tip"), (1, 0, "L base"), (1, 1, "L tip"), (2, None, "neck")):
        for c in range(3):
            for val in (np.nan, np.inf, -np.inf):
                def fn(r, l, neck, roll, p, arr=arr, point=point, c=c, val=val):
                    if arr == 2:
                        neck[p, c] = val
                    else:
                        (r, l)[arr][p, point, c] = val
                cases.append((f"{val} in {label} {'xyz'[c]}", fn))

    def roll_nan(r, l, neck, roll, p):
        roll[p] = np.nan

    def bases_equal(r, l, neck, roll, p):
        l[p, 0] = r[p, 0]

    def tip_r(r, l, neck, roll, p):
        r[p, 1] = r[p, 0]

    def tip_l(r, l, neck, roll, p):
        l[p, 1] = l[p, 0]

    def neck_r(r, l, neck, roll, p):
        neck[p] = r[p, 0]

    def neck_l(r, l, neck, roll, p):
        neck[p] = l[p, 0]

    def mid_zero(r, l, neck, roll, p):
        neck[p, 0], neck[p, 2] = (r[p, 0, 0] + l[p, 0, 0]) * 0.5, (r[p, 0, 2] + l[p, 0, 2]) * 0.5

    return cases + [("NaN in the given head roll", roll_nan), ("L base = R base", bases_equal), ("R tip = R base", tip_r),
                    ("L tip = L base", tip_l), ("neck = R base", neck_r), ("neck = L base", neck_l),
                    ("mid with zero (x, z)", mid_zero)]


def _d_base():
    z = load_golden("anipose_head")
    r, l = z["R_head"][1000:1000 + N_D].copy(), z["L_head"][1000:1000 + N_D].copy()
    neck = np.repeat(z["Neck"][:, 0], N_D, axis=0)
    roll = np.random.default_rng(20262).uniform(-1.0, 1.0, N_D)
    return r, l, neck, roll


def d_expectation(r, l, neck, rest, roll, compute_ant=True):
    """-> (must, may): NaN is REQUIRED where the reference's restatement is NaN and the yardstick is not finite either,
    ALLOWED where the restatement is NaN at all (its own ulp overshoot past 1, which the rule's clamp may absorb, and a
    difference of key points that is zero in float64 but not exactly), and nowhere else."""
    with np.errstate(all="ignore"):
        ref = head_oracle.head_angles(r, l, neck, *rest, head_roll=roll, compute_ant=compute_ant)
    may = np.isnan(ref)
    return may & ~np.isfinite(truth_head(r, l, neck, rest, roll, compute_ant)[0].astype(np.float64)), may


# The outputs (0 head roll, 1 pitch, 2 yaw, 3 antenna yaw L, 4 pitch L, 5 yaw R, 6 pitch R) that read the key point a
# zero-vector case moves.  The bases enter the roll and the yaw through hor and the pitch through mid; the antenna angles
# read hor directly (the yaws), through the derotation by the frame's OWN roll (all four; not with a given roll), and
# their own base and tip; the neck enters the pitch (mid) and the two antenna pitches (the head vector neck - base).
D_READS = {"L base = R base": dict(own={0, 1, 2, 3, 4, 5, 6}, rolled={0, 1, 2, 3, 4, 5}),      # (rolled: pitch R reads R only)
           "R tip = R base": {5, 6}, "L tip = L base": {3, 4},
           "neck = R base": {1, 4, 6}, "neck = L base": {1, 4, 6}, "mid with zero (x, z)": {1, 4, 6}}


def _d_reads(name, v):
    reads = D_READS[name]
    reads = reads["own" if v == "three" else v] if isinstance(reads, dict) else reads
    return sorted(j for j in reads if j < (3 if v == "three" else 7))


def _pitch_input_term(r, l, neck):
    """The head pitch reads mid = (rb + lb) / 2 - neck, and rb + lb is rounded (relative u) before the neck comes off:
    an error of up to u |rb + lb| / 2 per component of mid, the yardstick forming the same sum in long double.  On an
    ordinary frame that is a fraction of an ulp of the cosine; with the neck put ON a base, mid is half the short base
    to base vector and the same rounding turns its (x, z) projection by up to u |(rb + lb)_xz| / (2 |mid_xz|).  That is
    conditioning of the INPUT, not rounding of the cosine, so it stands next to the envelope (K stays 4 K_ref), with a
    factor 2 for the rule's own rounding of the difference and the arcsine's curvature."""
    s = r[:, 0] + l[:, 0]
    mid = s * 0.5 - neck
    with np.errstate(all="ignore"):
        return U * np.hypot(s[:, 0], s[:, 2]) / np.hypot(mid[:, 0], mid[:, 2])


def check_family_d(run, rest, K, label=""):
    """run(r, l, neck, roll or None, compute_ant) -> angles.  A coordinate injection leaves every finite output of its
    frame on the clean run's bits.  A zero-vector case MOVES a key point: the outputs that read it (D_READS; the same
    set as the outputs on which head_oracle.head_angles differs between the clean and the edited input, asserted) are NaN
    where expected and otherwise inside the envelope, the head pitch with the input term above; every other output of
    the frame, and every other frame, keeps the clean run's bits."""
    r0, l0, neck0, roll0 = _d_base()
    clean = {v: run(r0, l0, neck0, roll0 if v == "rolled" else None, v != "three") for v in ("own", "three", "rolled")}
    assert all(np.isfinite(c).all() for c in clean.values())
    with np.errstate(all="ignore"):
        ref0 = {v: head_oracle.head_angles(r0, l0, neck0, *rest, head_roll=roll0 if v == "rolled" else None,
                                           compute_ant=v != "three") for v in clean}
    n_nan, worst = 0, {}
    positions = list(POSITIONS)
    for name, fn in _d_cases():
        moves = " in " not in name
        r, l, neck, roll = r0.copy(), l0.copy(), neck0.copy(), roll0.copy()
        for p in POSITIONS:
            fn(r, l, neck, roll, p)
        for v in ("own", "three", "rolled"):
            given = roll if v == "rolled" else None
            got = run(r, l, neck, given, v != "three")
            must, may = d_expectation(r, l, neck, rest, given, v != "three")
            assert not may[:, [p for p in range(N_D) if p not in POSITIONS]].any()
            if v == ("rolled" if name.startswith("NaN in the given") else "own"):
                assert may[:, positions].any(0).all() and must.any(), (name, v)      # the case does something at every position
            is_nan = np.isnan(got)
            assert (is_nan >= must).all() and (is_nan <= may).all(), (label, name, v, got[:, positions], must[:, positions])
            free = is_nan.copy()      # what is NOT held to the clean run's bits
            if moves:
                reads = _d_reads(name, v)
                with np.errstate(all="ignore"):
                    ref = head_oracle.head_angles(r, l, neck, *rest, head_roll=given, compute_ant=v != "three")
                differs = np.ascontiguousarray(ref).view(np.uint64) != np.ascontiguousarray(ref0[v]).view(np.uint64)
                assert not differs[:, [p for p in range(N_D) if p not in POSITIONS]].any()
                for p in positions:      # the reference's outputs that moved are the ones that read the moved point
                    assert list(np.flatnonzero(differs[:, p])) == reads, (name, v, p, np.flatnonzero(differs[:, p]), reads)
                f, raw = truth_head(r[positions], l[positions], neck[positions], rest,
                                    None if given is None else given[positions], v != "three")
                f = np.where(is_nan[:, positions], LD(np.nan), f)      # (NaN that was allowed above)
                term = _pitch_input_term(r[positions], l[positions], neck[positions])
                for j in reads:
                    ok = np.isfinite(f[j].astype(np.float64))
                    assert np.isfinite(got[j, positions][ok]).all(), (label, name, v, j)
                    if not ok.any():
                        continue
                    bound = envelope(raw[j].astype(np.float64)[ok], K) + (2 * term[ok] if j == 1 else 0.0)
                    ratio = float((error(got[j, positions], f[j], raw[j])[ok] / bound).max())
                    worst[(name, v, j)] = ratio
                    assert ratio <= 1.0, (label, name, v, j, ratio)
                    free[j, np.array(positions)[ok]] = True
            assert same_bits(got[~free], clean[v][~free]), (label, name, v)
            n_nan += int(is_nan.sum())
    print(f"\n[head accuracy] {label}, family d, finite outputs that read a moved key point, worst error / bound: " +
          ", ".join(f"{k[0]} / {k[1]} / out {k[2]}: {w:.3f}" for k, w in worst.items()))
    return n_nan


# ======================================================= CPU tier =======================================================

def test_host_signed_angles_stay_inside_the_envelope(host, fam_a, bound):
    check_family_a(host, fam_a, bound["K"])


def test_host_head_angles_stay_inside_the_envelope(host, fam_b, rest, bound):
    check_family_b(host, fam_b, rest, bound["K"])


def test_host_head_angles_scale_exactly_by_powers_of_two(host, fam_b, rest):
    check_family_c(host, fam_b, rest)


def test_host_nan_in_nan_out_and_nothing_else_moves(host, rest, bound):
    """Family d.  On the revision before the clamps kept NaN this fails at the first case (NaN in R base x): the angles
    that hang on it came back as -pi, +pi, ... from a cosine clamped to -1 where the reference gives NaN."""
    n = check_family_d(lambda r, l, neck, roll, ant: host.head(r, l, neck, rest, compute_ant=ant, head_roll=roll), rest,
                       bound["K"], label="plain")
    assert n > 0
    check_family_d(lambda r, l, neck, roll, ant: host.raw(r, l, neck, rest, IDENTITY, compute_ant=ant, head_roll=roll), rest,
                   bound["K"], label="fused, identity map")


def _raw_case():
    """Family d through the real map: the raw fixture's first N_D frames, its constants; NaN / inf injected in RAW
    coordinates (the map hands them on: scale > 0), the expectation taken on the numpy-mapped points."""
    from seqikpy_amd.alignment import AlignPose
    z, raw = fixture_raw()
    consts = aligner(raw).head_affines()
    pair = (consts["R"], consts["L"])
    assert pair[0][1] > 0 and pair[0][2] > 0 and pair[1][1] > 0 and pair[1][2] > 0
    r0, l0 = raw["R_head"][:N_D].copy(), raw["L_head"][:N_D].copy()
    neck0 = np.repeat(z["aligned_Neck"][:, 0], N_D, axis=0)
    roll0 = _d_base()[3]
    cases = [c for c in _d_cases() if " in " in c[0]]      # the 45 coordinate injections and the NaN roll
    return pair, (r0, l0, neck0, roll0), cases, AlignPose.apply_head_affine


def check_family_d_raw(be, rest):
    pair, (r0, l0, neck0, roll0), cases, amap = _raw_case()
    clean = {v: be.raw(r0, l0, neck0, rest, pair, compute_ant=v != "three", head_roll=roll0 if v == "rolled" else None)
             for v in ("own", "three", "rolled")}
    assert all(np.isfinite(c).all() for c in clean.values())
    for name, fn in cases:
        r, l, neck, roll = r0.copy(), l0.copy(), neck0.copy(), roll0.copy()
        for p in POSITIONS:
            fn(r, l, neck, roll, p)
        with np.errstate(all="ignore"):
            ra, la = amap(r, pair[0]), amap(l, pair[1])
        for v in ("own", "three", "rolled"):
            given = roll if v == "rolled" else None
            got = be.raw(r, l, neck, rest, pair, compute_ant=v != "three", head_roll=given)
            must, may = d_expectation(ra, la, neck, rest, given, v != "three")
            assert (np.isnan(got) >= must).all() and (np.isnan(got) <= may).all(), (be.name, name, v)
            must = np.isnan(got)
            assert same_bits(got[~must], clean[v][~must]), (be.name, name, v)


def test_host_nan_in_nan_out_through_the_alignment_map(host):
    check_family_d_raw(host, rest_pitches())


def test_host_signed_angle_of_a_zero_vector_is_nan(host):
    for be_axis in AXES:
        got = host.signed([[0.0, 0, 0], [1.0, 0, 0], [np.nan, 0, 0], [1.0, np.inf, 0]], [1.0, 0, 0], be_axis)
        assert np.isnan(got[[0, 2, 3]]).all() and got[1] == 0.0


# ======================================================= GPU tier =======================================================

def _device_entry(hiplib, r, l, neck, rest, compute_ant=True, offset=True):
    """seqik_head_angles_ex_device on device buffers that are only 8-byte aligned (``offset``): the per-lane kernel
    seqik_head_kernel<false> with the antennae on.  -> (7 or 3, n) on the host."""
    import torch
    n = len(r)
    o = 1 if offset else 0
    bufs = []
    for a in (r, l):
        t = torch.zeros(n * 6 + 2, dtype=torch.float64, device="cuda")
        t[o:o + n * 6] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
        assert (t.data_ptr() + 8 * o) % 16 == 8 * o
        bufs.append(t)
    neck = np.ascontiguousarray(neck, dtype=np.float64).reshape(-1, 3)
    d_neck = torch.from_numpy(neck).cuda()
    out = torch.full((7, n), 7.0, dtype=torch.float64, device="cuda")
    rc = hiplib.load().seqik_head_angles_ex_device(bufs[0].data_ptr() + 8 * o, bufs[1].data_ptr() + 8 * o, n, 2,
                                                   d_neck.data_ptr(), 3 if len(neck) == n and n > 1 else 0, rest[0],
                                                   rest[1], 1 if compute_ant else 0, None, out.data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert compute_ant or bool((res[3:] == 7.0).all())
    return res if compute_ant else res[:3]


def _device_raw_entry(hiplib, r, l, neck, rest, affine, compute_ant=True, offset=True):
    """seqik_head_angles_raw_device on device buffers that are only 8-byte aligned (``offset``): the per-lane fused
    kernel seqik_head_raw_kernel<false, false, false> with the antennae on.  -> (7 or 3, n) on the host."""
    import torch
    n = len(r)
    o = 1 if offset else 0
    bufs = []
    for a in (r, l):
        t = torch.zeros(n * 6 + 2, dtype=torch.float64, device="cuda")
        t[o:o + n * 6] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(-1)).cuda()
        assert (t.data_ptr() + 8 * o) % 16 == 8 * o
        bufs.append(t)
    neck = np.ascontiguousarray(neck, dtype=np.float64).reshape(-1, 3)
    d_neck = torch.from_numpy(neck).cuda()
    out = torch.full((7, n), 7.0, dtype=torch.float64, device="cuda")
    hiplib.head_angles_raw_device(bufs[0].data_ptr() + 8 * o, bufs[1].data_ptr() + 8 * o, n, 2, d_neck.data_ptr(),
                                  3 if len(neck) == n and n > 1 else 0, rest[0], rest[1], affine, out.data_ptr(),
                                  compute_ant=compute_ant, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert compute_ant or bool((res[3:] == 7.0).all())
    return res if compute_ant else res[:3]


def check_aligned_out_on_injected_frames(hiplib, rest):
    """The ALIGNED_OUT instantiations of the fused kernel on NaN / inf frames: the staged one (own roll; its aligned
    records go back through LDS), <false, true, true> (given roll), <false, false, true> (no antennae).  The angles are
    the bits of the run that writes no records; the records are the numpy map of the raw points, NaN and inf included."""
    pair, (r0, l0, neck0, roll0), cases, amap = _raw_case()
    for name, fn in cases:
        if not ("x" in name.split()[-1] or name.startswith("NaN in the given")):      # a third of the cases: one coordinate
            continue
        r, l, neck, roll = r0.copy(), l0.copy(), neck0.copy(), roll0.copy()
        for p in POSITIONS:
            fn(r, l, neck, roll, p)
        with np.errstate(all="ignore"):
            ra, la = amap(r, pair[0]), amap(l, pair[1])
        for v in ("own", "three", "rolled"):
            kw = dict(compute_ant=v != "three", head_roll=roll if v == "rolled" else None)
            got, r_al, l_al = hiplib.head_angles_raw(r, l, neck, *rest, pair, want_aligned=True, **kw)
            assert same_bits_or_both_nan(got, hiplib.head_angles_raw(r, l, neck, *rest, pair, **kw)), (name, v)
            assert same_bits_or_both_nan(r_al, ra) and same_bits_or_both_nan(l_al, la), (name, v)


@pytest.fixture(scope="module")
def device(hiplib):
    return Device(hiplib)


def _per_lane_equals_staged(hiplib, rest):
    def fn(member, own, three, rolled):
        name, r, l, neck, given, _ = member
        assert same_bits_or_both_nan(_device_entry(hiplib, r, l, neck, rest), own), name           # <false>, antennae on
        assert same_bits_or_both_nan(_device_entry(hiplib, r, l, neck, rest, compute_ant=False), three), name
        assert same_bits_or_both_nan(_device_entry(hiplib, r, l, neck, rest, offset=False), own), name   # <true>
        # the fused kernel, per lane with the antennae on (8-byte-offset buffers), and staged
        assert same_bits_or_both_nan(_device_raw_entry(hiplib, r, l, neck, rest, IDENTITY), own), name
        assert same_bits_or_both_nan(_device_raw_entry(hiplib, r, l, neck, rest, IDENTITY, offset=False), own), name
    return fn


@pytest.mark.gpu
def test_device_signed_angles_stay_inside_the_envelope(device, host, fam_a, bound):
    w_dev = check_family_a(device, fam_a, bound["K"])
    w_host = check_family_a(host, fam_a, bound["K"])
    print(f"\n[head accuracy] family a, device / host worst ratios: {w_dev} / {w_host}")


@pytest.mark.gpu
def test_device_head_angles_stay_inside_the_envelope(device, hiplib, fam_b, rest, bound):
    check_family_b(device, fam_b, rest, bound["K"], extra=(_per_lane_equals_staged(hiplib, rest),))


@pytest.mark.gpu
def test_device_head_angles_scale_exactly_by_powers_of_two(device, hiplib, fam_b, rest):
    check_family_c(device, fam_b, rest, extra=(_per_lane_equals_staged(hiplib, rest),))


@pytest.mark.gpu
def test_device_nan_in_nan_out_and_nothing_else_moves(device, hiplib, rest, bound):
    n = check_family_d(lambda r, l, neck, roll, ant: device.head(r, l, neck, rest, compute_ant=ant, head_roll=roll), rest,
                       bound["K"], label="seqik_head_kernel")
    assert n > 0
    check_family_d(lambda r, l, neck, roll, ant: device.raw(r, l, neck, rest, IDENTITY, compute_ant=ant, head_roll=roll), rest,
                   bound["K"], label="seqik_head_raw_kernel, identity map")

    def per_lane(r, l, neck, roll, ant):      # 8-byte-offset buffers; the given roll has its own kernel, run above
        if roll is not None:
            return device.head(r, l, neck, rest, compute_ant=ant, head_roll=roll)
        return _device_entry(hiplib, r, l, neck, rest, compute_ant=ant)
    check_family_d(per_lane, rest, bound["K"], label="seqik_head_kernel<false>")

    def raw_per_lane(r, l, neck, roll, ant):      # the fused kernel per lane, antennae on, from 8-byte-offset buffers
        if roll is not None:
            return device.raw(r, l, neck, rest, IDENTITY, compute_ant=ant, head_roll=roll)
        return _device_raw_entry(hiplib, r, l, neck, rest, IDENTITY, compute_ant=ant)
    check_family_d(raw_per_lane, rest, bound["K"], label="seqik_head_raw_kernel<false, false, false>")
    check_aligned_out_on_injected_frames(hiplib, rest_pitches())
    check_family_d_raw(device, rest_pitches())
    for axis in AXES:
        got = device.signed([[0.0, 0, 0], [1.0, 0, 0], [np.nan, 0, 0], [1.0, np.inf, 0]], [1.0, 0, 0], axis)
        assert np.isnan(got[[0, 2, 3]]).all() and got[1] == 0.0


@pytest.mark.gpu
def test_compute_head_angles_reports_a_missing_key_point_as_nan(hiplib):
    from seqikpy_amd.data import NMF_TEMPLATE
    from seqikpy_amd.head_inverse_kinematics import ANGLE_NAMES, HeadInverseKinematics
    z = load_golden("anipose_head")
    pos = {"R_head": z["R_head"].copy(), "L_head": z["L_head"].copy(), "Neck": z["Neck"]}
    clean = HeadInverseKinematics(pos, NMF_TEMPLATE, log_level="ERROR").compute_head_angles()
    frame = 64 * 40 + 17
    pos["R_head"][frame, 0, 1] = np.nan      # y of the right antenna base: everything but the head pitch hangs on it
    got = HeadInverseKinematics(pos, NMF_TEMPLATE, log_level="ERROR").compute_head_angles()
    for name in ANGLE_NAMES:
        others = np.arange(6000) != frame
        assert same_bits(got[name][others], clean[name][others]), name
        if name == "Angle_head_pitch":
            assert got[name][frame] == clean[name][frame]
        else:
            assert np.isnan(got[name][frame]), (name, got[name][frame])
