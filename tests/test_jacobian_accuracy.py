"""Leg Jacobians, stage conditioning and key-point velocities against a 200-bit yardstick; the domain rules.

The device rule of csrc/seqik_jacobian.hpp -- run on the host (CPU tier, tests/harness/jacobian_harness.hip) and as a
kernel (``-m gpu``) -- is held to a bound derived from the number format, on the input families of
tests/test_fk_accuracy.py (in range, unwrapped, multiples of pi / 2, large, tiny) plus near-singular postures, for both
chain kinds.

YARDSTICK.  ``mp_chain`` of tests/test_fk_accuracy.py (the nine-link chain of include/seqik_frames.h multiplied out at
200 bits, nothing taken from csrc), leg-local.  On top of it, at 200 bits: every entry a_j x (p_k - o_j) as
include/seqik_jacobian.h defines it -- all 84, the structural zeros included, so the yardstick also confirms that
exactly those entries vanish --, ``mpmath.svd_r`` of the stage blocks (kind 0) and of the claw's 3 x 7 block (kind 1),
and the exact J . qdot.  Kept as float64 pairs (hi, lo): an error is ``(got - hi) - lo``.

BOUND.  u = 2^-53, S_k = seg[0] + ... + seg[k - 1].
    Jacobian entries of key point k:  |got - truth| <= K u S_k
    sigma of stage k (kind 1: S_4):   |got - truth| <= K_s u S_k     (absolute: sigma_min must meet it where it is ~0)
    velocities of key point k:        |got - truth| <= K_v u S_k sum_j |qdot_j|
``K_REF``, ``K_S_REF``, ``K_V_REF`` are the smallest powers of two for which the float64 numpy restatement -- frames from
the IKPy stand-in oracle/shim/ikpy, ``np.cross``, ``np.linalg.svd``, ``@`` -- stays inside the bound on exactly the inputs
below; the tests use 4 x that, the project's margin for two correctly rounded evaluation orders.  K is never read off
the code under test and no input is left out.

INPUT FAMILIES (seeded; both kinds).  a-e are ``build_families()`` of tests/test_fk_accuracy.py, every leg-frame of
them (1 675 in all); the rates are standard normal, those of every eighth leg-frame times 1e3.
  a. in range   b. unwrapped to +-200 pi   c. multiples of pi / 2 +- a few ulp   d. large, up to +-2^30
  e. tiny and zero
  n. near-singular: three in-range postures, each with FTi_pitch in {0, +-1e-300, +-1e-12, +-1e-8, +-1e-4}, with CTr_pitch
     in the same set, and with ThC_pitch at +-pi/2 (as doubles): stages 3, 2 and 1 of the sequential chain at and next to
     their singularity.  sigma_min meets its absolute bound here.
  scaling: family a's segment lengths times 2^k, k in {-20, -1, 1, 20}: jac, sigma and vel are 2^k times the unscaled
     run's bit for bit.
  outside the domain: the values and places of family h of tests/test_fk_accuracy.py: those leg-frames are NaN (84 + 8 +
     12), every other one keeps the bits of the clean run; the same for a non-finite rate and the 12 velocities.

MEASURED (EXPERIMENTS.md, "Leg Jacobians"; the tests print the figures, ``-s``).  Worst error / (u S ...):
    family                      a      b      c      d      e      n
    restatement   jac         3.730  3.363  1.587  2.642  2.243  2.514     -> K_REF = 4,    K = 16
                  sigma       5.369  6.556  5.114  7.117  4.529  5.249     -> K_S_REF = 8,  K_s = 32
                  vel         1.562  1.850  1.004  1.347  0.936  1.751     -> K_V_REF = 2,  K_v = 8
    host build    jac         3.730  3.363  1.587  2.642  2.243  2.514
                  sigma seq   3.347  3.347  1.268  3.532  1.761  2.005
                  sigma gen   7.113  8.138  4.014  6.357  3.187  3.377
                  vel         1.562  1.246  1.173  1.434  1.032  1.283
(jac and vel: the larger of the two kinds).  Device (MI355X), families a and n, on its own output: jac 3.730 / 2.514,
sigma 7.113 / 3.377, vel 1.562 / 1.283 -- the host build's figures; everywhere else the GPU tier asserts the host build's
bits (tests/test_jacobians.py)."""
import numpy as np
import pytest

from angle_map_support import gpu_lib, same_bits
from conftest import ROOT  # noqa: F401
from test_fk_accuracy import (H_FRAMES, H_JOINTS, H_N, OUTSIDE, SPEC, _MP, _split, build_families, h_batches, mp_chain,
                              restatement)
from test_jacobians import (KEY_LINKS, STAGE_DOFS, jac_harness, nonzero_mask, numpy_jacobian)  # noqa: F401

U = 2.0 ** -53
K_REF, K_S_REF, K_V_REF = 4, 8, 2
K, K_S, K_V = 4 * K_REF, 4 * K_S_REF, 4 * K_V_REF
KINDS = (0, 1)
NEAR = (0.0, 1e-300, -1e-300, 1e-12, -1e-12, 1e-8, -1e-8, 1e-4, -1e-4)
BOUND_FAMILIES = ("a", "b", "c", "d", "e", "n")


# ------------------------------------------------------ families -------------------------------------------------------

def _rates(rng, n):
    q = rng.standard_normal((n, 7))
    q[::8] *= 1e3
    return q


@pytest.fixture(scope="module")
def fams():
    """name -> dict(ang (n, 7), seg (n, 4), qdot (n, 7)): flat leg-frames, each with its own segment lengths."""
    base = build_families()
    rng = np.random.default_rng(20261020)
    out = {}
    for name in "abcde":
        L, N = base[name]["ang"].shape[:2]
        ang = base[name]["ang"].reshape(L * N, 7)
        seg = np.repeat(base[name]["seg"], N, axis=0)
        out[name] = dict(name=name, ang=np.ascontiguousarray(ang), seg=np.ascontiguousarray(seg), qdot=_rates(rng, len(ang)))
    postures, rows = rng.uniform(-np.pi, np.pi, (3, 7)), []
    for p in postures:
        for dof in (5, 3):
            for v in NEAR:
                rows.append(p.copy())
                rows[-1][dof] = v
        for v in (np.pi / 2, -np.pi / 2):
            rows.append(p.copy())
            rows[-1][1] = v
    n = len(rows)
    assert n == 3 * 20
    out["n"] = dict(name="n", ang=np.array(rows), seg=np.repeat(rng.uniform(0.15, 1.8, (3, 4)), 20, axis=0), qdot=_rates(rng, n))
    return out


def by_leg(fam):
    """Runs of consecutive leg-frames with the same segment lengths: (slice, seg)."""
    seg, start, out = fam["seg"], 0, []
    for i in range(1, len(seg) + 1):
        if i == len(seg) or (seg[i] != seg[start]).any():
            out.append((slice(start, i), seg[start]))
            start = i
    return out


# ------------------------------------------------------ yardstick ------------------------------------------------------

_TRUTH = {}


def mp_jacobian(kind, ang, seg, qdot):
    """One leg-frame -> jac (2, 4, 3, 7), sigma (2, 8), vel (2, 4, 3): hi and lo parts of the exact values."""
    fr = mp_chain(kind, ang, seg, np.zeros((5, 3)))[0]
    F = [[[_MP.mpf(float(fr[0, i, r, c])) + _MP.mpf(float(fr[1, i, r, c])) for c in range(4)] for r in range(3)] for i in range(9)]
    J = [[[_MP.mpf(0)] * 7 for _ in range(3)] for _ in range(4)]
    for link, (axis, dof, _) in enumerate(SPEC[kind]):
        if axis is None:
            continue
        col = "xyz".index(axis)
        a = [F[link][r][col] for r in range(3)]
        for k, kl in enumerate(KEY_LINKS):
            if link > kl:
                continue   # a joint behind the key point does not move it
            d = [F[kl][r][3] - F[link][r][3] for r in range(3)]
            cr = [a[1] * d[2] - a[2] * d[1], a[2] * d[0] - a[0] * d[2], a[0] * d[1] - a[1] * d[0]]
            for c in range(3):
                J[k][c][dof] = cr[c]
    jac, sigma, vel = np.zeros((2, 4, 3, 7)), np.full((2, 8), np.nan), np.zeros((2, 4, 3))
    q = [_MP.mpf(float(v)) for v in qdot]
    for k in range(4):
        for c in range(3):
            for d in range(7):
                jac[:, k, c, d] = _split(J[k][c][d])
            vel[:, k, c] = _split(sum((J[k][c][d] * q[d] for d in range(7)), _MP.mpf(0)))
    if kind == 0:
        for s, dofs in enumerate(STAGE_DOFS):
            sv = _MP.svd_r(_MP.matrix([[J[s][c][d] for d in dofs] for c in range(3)]), compute_uv=False)
            sigma[:, 2 * s], sigma[:, 2 * s + 1] = _split(sv[0]), _split(sv[len(dofs) - 1])
    else:
        sv = _MP.svd_r(_MP.matrix([[J[3][c][d] for d in range(7)] for c in range(3)]), compute_uv=False)
        for i in range(3):
            sigma[:, i] = _split(sv[i])
    return jac, sigma, vel


def truth(fam, kind):
    out = []
    for j in range(len(fam["ang"])):
        key = (fam["name"], kind, j)
        if key not in _TRUTH:
            _TRUTH[key] = mp_jacobian(kind, fam["ang"][j], fam["seg"][j], fam["qdot"][j])
        out.append(_TRUTH[key])
    return tuple(np.stack([o[i] for o in out], 1) for i in range(3))


def ratios(fam, kind, jac, sigma, vel):
    """Worst |got - truth| / (u S ...) of the three outputs; inf when a value that must be finite is not."""
    tj, ts, tv = truth(fam, kind)
    S = np.cumsum(np.abs(fam["seg"]), axis=1)                                   # (n, 4): S_1 .. S_4
    S_sigma = np.repeat(S, 2, axis=1) if kind == 0 else np.repeat(S[:, 3:], 3, axis=1)
    sigma = sigma[:, :S_sigma.shape[1]]
    if not (np.isfinite(jac).all() and np.isfinite(sigma).all() and np.isfinite(vel).all()):
        return np.inf, np.inf, np.inf
    rj = np.abs((jac - tj[0]) - tj[1]) / (U * S[:, :, None, None])
    rs = np.abs((sigma - ts[0][:, :S_sigma.shape[1]]) - ts[1][:, :S_sigma.shape[1]]) / (U * S_sigma)
    rv = np.abs((vel - tv[0]) - tv[1]) / (U * S[:, :, None] * np.abs(fam["qdot"]).sum(1)[:, None, None])
    return float(rj.max()), float(rs.max()), float(rv.max())


# ------------------------------------------------------- back ends ------------------------------------------------------

def host_run(jh, fam, kind):
    n = len(fam["ang"])
    jac, sigma, vel = np.empty((n, 4, 3, 7)), np.empty((n, 8)), np.empty((n, 4, 3))
    for sl, seg in by_leg(fam):
        jac[sl], sigma[sl], vel[sl] = jh.run(fam["ang"][sl], seg, kind, fam["qdot"][sl])
    return jac, sigma, vel


def numpy_run(fam, kind):
    """The float64 restatement: IKPy stand-in frames, np.cross, np.linalg.svd, @."""
    n = len(fam["ang"])
    jac, sigma = np.empty((n, 4, 3, 7)), np.full((n, 8), np.nan)
    for sl, seg in by_leg(fam):
        f = dict(name="r", ang=fam["ang"][None, sl], seg=seg[None], pose=np.zeros((1, sl.stop - sl.start, 5, 3)))
        jac[sl] = numpy_jacobian(restatement(f, kind)[0], kind)
    if kind == 0:
        for s, dofs in enumerate(STAGE_DOFS):
            sv = np.linalg.svd(jac[:, s][:, :, list(dofs)], compute_uv=False)
            sigma[:, 2 * s], sigma[:, 2 * s + 1] = sv[:, 0], sv[:, -1]
    else:
        sigma[:, :3] = np.linalg.svd(jac[:, 3], compute_uv=False)
    vel = (jac @ fam["qdot"][:, None, :, None])[..., 0]
    return jac, sigma, vel


def device_run(lib, fam, kind):
    n = len(fam["ang"])
    jac, sigma, vel = np.empty((n, 4, 3, 7)), np.empty((n, 8)), np.empty((n, 4, 3))
    for sl, seg in by_leg(fam):
        params = [lib.leg_params_from_arrays(seg, np.zeros((7, 2)), np.zeros(27))]
        out = lib.leg_jacobians(fam["ang"][None, None, sl], params, kind=kind, qdot=fam["qdot"][None, None, sl])
        jac[sl], vel[sl] = out["jac"][0, 0], out["vel"][0, 0]
        sigma[sl] = np.nan
        sigma[sl, :8 if kind == 0 else 3] = out["sigma"][0, 0].reshape(sl.stop - sl.start, -1)
    return jac, sigma, vel


# -------------------------------------------------------- K_ref --------------------------------------------------------

def _fmt(worst):
    return "; ".join(f"{name}: jac {r[0]:.3f} sigma {r[1]:.3f} vel {r[2]:.3f}" for name, r in worst.items())


def test_k_ref_is_measured_on_the_numpy_restatement(fams):
    worst = {name: tuple(max(r) for r in zip(*[ratios(fams[name], kind, *numpy_run(fams[name], kind)) for kind in KINDS]))
             for name in BOUND_FAMILIES}
    print("\n[jacobian accuracy] numpy restatement, worst error / (u S ...): " + _fmt(worst))
    top = [max(r[i] for r in worst.values()) for i in range(3)]
    # each K_ref is the smallest power of two that held the restatement when the bounds were set (3.730, 7.117, 1.850): a
    # numpy or LAPACK on which it needs more would loosen every bound of this module, and that must not pass unseen
    for got, k_ref in zip(top, (K_REF, K_S_REF, K_V_REF)):
        assert got <= k_ref, (top, (K_REF, K_S_REF, K_V_REF))
    assert (K, K_S, K_V) == (4 * K_REF, 4 * K_S_REF, 4 * K_V_REF)


def test_the_yardstick_confirms_the_zero_pattern(fams):
    """Evaluated from the formula at every posture of family a, exactly the entries the header lists vanish (to the 1e-30
    that frames kept as hi + lo pairs leave); every other entry is far from zero somewhere."""
    for kind in KINDS:
        tj = truth(fams["a"], kind)[0]
        mag = np.abs(tj[0] + tj[1]).max(axis=(0, 2))   # (4, 7)
        nz = nonzero_mask(kind)
        assert (mag[~nz] < 1e-30).all() and (mag[nz] > 1e-2).all(), (kind, mag)


# -------------------------------------------------------- checks --------------------------------------------------------

@pytest.mark.parametrize("name", BOUND_FAMILIES)
def test_host_rule_inside_the_bound(jac_harness, fams, name):  # noqa: F811
    worst = {f"kind {kind}": ratios(fams[name], kind, *host_run(jac_harness, fams[name], kind)) for kind in KINDS}
    print(f"\n[jacobian accuracy] host build, family {name}, worst error / (u S ...): " + _fmt(worst) +
          f"  (K = {K}, K_s = {K_S}, K_v = {K_V})")
    for r in worst.values():
        assert r[0] <= K and r[1] <= K_S and r[2] <= K_V, worst


def test_host_sigma_min_survives_the_singular_postures(jac_harness, fams):  # noqa: F811
    """Family n, sequential chain: at FTi_pitch = 0 / CTr_pitch = 0 / ThC_pitch = +-pi/2 the stage's sigma_min is at
    rounding level (the bound of the previous test is absolute, so it held there), and next to the singularity it follows
    the offset -- 1e-12 rad away it is of order 1e-12, which the small eigenvalue of the Gram matrix cannot show."""
    fam = fams["n"]
    _, sigma, _ = host_run(jac_harness, fam, 0)
    ts = truth(fam, 0)[1][0]
    for p in range(3):
        base = 20 * p
        for stage, first in ((2, base), (1, base + 9)):           # FTi_pitch rows, then CTr_pitch rows
            smin, tmin = sigma[first:first + 9, 2 * stage + 1], ts[first:first + 9, 2 * stage + 1]
            assert (smin[:3] <= K_S * U * np.abs(fam["seg"][first, :stage + 1]).sum()).all(), (p, stage, smin[:3])
            for i, off in ((3, 1e-12), (5, 1e-8), (7, 1e-4)):
                assert (np.abs(smin[i:i + 2] / tmin[i:i + 2] - 1) < 1e-3).all(), (p, stage, off, smin, tmin)
                assert (0.01 * off < smin[i:i + 2]).all() and (smin[i:i + 2] < 4 * off).all(), (p, stage, off, smin)
        assert (sigma[base + 18:base + 20, 1] < 4e-15).all()        # ThC_pitch = +-pi/2 as doubles: 6e-17 rad off


def test_host_scaling_by_powers_of_two_is_exact(jac_harness, fams):  # noqa: F811
    a = fams["a"]
    for kind in KINDS:
        ref = host_run(jac_harness, a, kind)
        for k in (-20, -1, 1, 20):
            got = host_run(jac_harness, dict(a, seg=a["seg"] * 2.0 ** k), kind)
            for g, r in zip(got, ref):
                assert same_bits(g, r * 2.0 ** k), (kind, k)


def check_outside_the_domain(run, fam_a):
    """``run(ang (V, 3, 130, 7), qdot, seg (3, 4), kind) -> jac, sigma, vel`` with leading (V, 3, 130)."""
    clean, bad, hit = h_batches(fam_a)
    rng = np.random.default_rng(77)
    qdot = rng.standard_normal(clean.shape)
    V = len(OUTSIDE)
    for kind in KINDS:
        j0, s0, v0 = run(clean[None], qdot[None], fam_a["seg"], kind)
        width = 8 if kind == 0 else 3
        assert np.isfinite(j0).all() and np.isfinite(s0[..., :width]).all() and np.isfinite(v0).all()
        j, s, v = run(bad, np.repeat(qdot[None], V, axis=0), fam_a["seg"], kind)
        assert np.isnan(j[hit]).all() and np.isnan(s[hit]).all() and np.isnan(v[hit]).all(), kind
        assert np.isnan(j).sum() == hit.sum() * 84 and np.isnan(v).sum() == hit.sum() * 12
        assert np.isnan(s[..., :width]).sum() == hit.sum() * width
        for val in range(V):
            keep = ~hit[val]
            assert same_bits(j[val][keep], j0[0][keep]) and same_bits(v[val][keep], v0[0][keep]), (kind, OUTSIDE[val])
            assert same_bits(s[val][keep], s0[0][keep]), (kind, OUTSIDE[val])
        # a non-finite rate: the 12 velocities of that leg-frame and nothing else
        bad_q = np.repeat(qdot[None], 3, axis=0)
        qhit = np.zeros(bad_q.shape[:3], bool)
        for i, val in enumerate((np.inf, -np.inf, np.nan)):
            for l, joint in enumerate(H_JOINTS):
                bad_q[i, l, list(H_FRAMES), joint] = val
                qhit[i, l, list(H_FRAMES)] = True
        j, s, v = run(np.repeat(clean[None], 3, axis=0), bad_q, fam_a["seg"], kind)
        assert np.isnan(v[qhit]).all() and np.isnan(v).sum() == qhit.sum() * 12
        for i in range(3):
            assert same_bits(j[i], j0[0]) and same_bits(s[i], s0[0]) and same_bits(v[i][~qhit[i]], v0[0][~qhit[i]]), kind


def test_host_outside_the_domain_makes_that_leg_frame_nan(jac_harness):  # noqa: F811
    from test_jacobians import host_batch
    check_outside_the_domain(lambda ang, q, seg, kind: host_batch(jac_harness, ang, seg, kind, q), build_families()["a"])
    assert H_N == 130


# ---------------------------------------------------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(hiplib):
    return gpu_lib(hiplib)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a", "n"])
def test_gpu_output_inside_the_bound_on_its_own(lib, fams, name):
    """The bound on what the device returned, not on the host build's bits: the in-range and the near-singular family."""
    worst = {f"kind {kind}": ratios(fams[name], kind, *device_run(lib, fams[name], kind)) for kind in KINDS}
    print(f"\n[jacobian accuracy] device, family {name}, worst error / (u S ...): " + _fmt(worst))
    for r in worst.values():
        assert r[0] <= K and r[1] <= K_S and r[2] <= K_V, worst


@pytest.mark.gpu
def test_gpu_outside_the_domain_makes_that_leg_frame_nan(lib):
    def run(ang, q, seg, kind):
        params = [lib.leg_params_from_arrays(s, np.zeros((7, 2)), np.zeros(27)) for s in seg]
        S, L, N = ang.shape[:3]
        jac, sigma, vel = np.full((S, L, N, 4, 3, 7), 7.0), np.full((S, L, N, 8), 7.0), np.full((S, L, N, 4, 3), 7.0)
        dp = lib._dp
        lib._call("seqik_leg_jacobians", ang.ctypes.data_as(dp), S, L, N, (lib.SeqikLegParams * L)(*params), kind,
                  np.ascontiguousarray(q).ctypes.data_as(dp), jac.ctypes.data_as(dp), sigma.ctypes.data_as(dp),
                  vel.ctypes.data_as(dp), -1)
        return jac, sigma, vel
    check_outside_the_domain(lambda ang, q, seg, kind: run(np.ascontiguousarray(ang), q, seg, kind), build_families()["a"])
