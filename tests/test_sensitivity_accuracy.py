"""Key-point sensitivity of the sequential leg fit against a 200-bit yardstick; flags, zeros, scaling, the domain rules.

The device rule of csrc/seqik_sensitivity.hpp -- run on the host (CPU tier, tests/harness/sensitivity_harness.hip) and as
a kernel (``-m gpu``) -- is held to a bound derived from the number format and the conditioning of its own solves.

YARDSTICK.  ``mp_rule`` of tests/sensitivity_support.py: the rule of include/seqik_sensitivity.h at 200 bits on
``mp_chain`` of tests/test_fk_accuracy.py, nothing taken from csrc.  The held set and the positive-definite verdict come
from the yardstick's own g and G.

INPUTS (seeded; 621 leg-frames).
  a. every leg-frame of family a of ``build_families()`` (390).  Targets: the yardstick's FK of those angles plus a radial
     offset (along the key point's direction from the leg's base) of {0, +-1e-3, +-5e-2, +-2e-1} S_k -- cycled over
     leg-frames and key points, so residuals of both signs and stages that are not at a strict minimum occur -- plus a
     tangential offset of 1e-2 S_k (which makes g != 0).  Limits far away.
  l. limits (168 + 3): three postures of a; each of the seven DOFs in turn placed at lb, lb + 1e-9, ub - 1e-9 and lb +
     1e-3, with the target of its stage moved along -+J_a so that g_a takes either sign.  Per posture one more input with
     the claw's target pulled back past the tibia end, where stage 4 is not at a minimum (a and n do not reach that).
  n. near-singular (60): the postures of family n of tests/test_jacobian_accuracy.py (FTi_pitch / CTr_pitch at and next
     to 0, ThC_pitch at +-pi/2), targets as in a.

BOUND.  u = 2^-53.  For the rows of stage s of a leg-frame:
    |got - truth| <= K u kappa max|truth, rows of stage s|,   kappa = prod_{s' <= s} cond_2(G_FF of stage s')
(cond_2 from the yardstick; 1 where one DOF or none is free).  Rows the yardstick makes NaN must be NaN, held rows exactly
0.  ``K_REF`` is the smallest power of two for which the float64 numpy restatement (``numpy_rule``: np.cross,
np.linalg.solve) stays inside on exactly these inputs; the tests use K = 4 K_REF, the project's margin.  No input is left
out of the bound, except: an input whose held / positive-definite verdict flips when g or det G moves by 1e3 u of its
scale (``margin`` of the yardstick) is compared on flags only -- its record must be what its own flags say.  At most 2 %
of the inputs may be such; asserted.

MEASURED (the tests print the figures, ``-s``).  Worst error / (u kappa max|truth|):
    family                a       l       n
    restatement        10.38    5.94    5.12      -> K_REF = 16, K = 64
    host build          8.59    6.02    4.72
    device (MI355X)     not measured when this was written: the GPU tier asserts the bound on the device's own output
                        and the host build's bits
Verdicts within 1e3 u of flipping: 0 of 621."""
import numpy as np
import pytest

from angle_map_support import gpu_lib, same_bits
from conftest import ROOT  # noqa: F401
from sensitivity_support import (BAD_INPUT, KEY_LINKS, STAGE_DOFS, WIDE, mp_key_points, mp_rule, numpy_frames, numpy_rule,
                                 sens_harness, structural_zero_mask)  # noqa: F401
from test_fk_accuracy import OUTSIDE, build_families
from test_jacobian_accuracy import NEAR, _rates

U = 2.0 ** -53
K_REF = 16
K = 4 * K_REF
RADIAL = (0.0, 1e-3, -1e-3, 5e-2, -5e-2, 2e-1, -2e-1)
FLIP = 1e3 * U
FAMILIES = ("a", "l", "n")


# ------------------------------------------------------- families ------------------------------------------------------

def _targets(rng, ang, seg, origin, j):
    """pose (5, 3): the yardstick's key points (rounded to double) + radial and tangential offsets + origin."""
    kp = np.array([[float(v) for v in p] for p in mp_key_points(ang, seg)])
    S = np.cumsum(np.abs(seg))
    pose = np.zeros((5, 3))
    pose[0] = origin
    for k in range(4):
        rad = kp[k] / np.linalg.norm(kp[k])
        tan = np.cross(rad, rng.standard_normal(3))
        tan /= np.linalg.norm(tan)
        pose[k + 1] = origin + kp[k] + RADIAL[(j + k) % 7] * S[k] * rad + 1e-2 * S[k] * tan
    return pose


def near_singular_postures():
    """Family n of tests/test_jacobian_accuracy.py: the same draws from the same generator -> ang (60, 7), seg (60, 4)."""
    base = build_families()
    rng = np.random.default_rng(20261020)
    for name in "abcde":
        _rates(rng, base[name]["ang"].shape[0] * base[name]["ang"].shape[1])
    postures, rows = rng.uniform(-np.pi, np.pi, (3, 7)), []
    for p in postures:
        for dof in (5, 3):
            for v in NEAR:
                rows.append(p.copy())
                rows[-1][dof] = v
        for v in (np.pi / 2, -np.pi / 2):
            rows.append(p.copy())
            rows[-1][1] = v
    return np.array(rows), np.repeat(rng.uniform(0.15, 1.8, (3, 4)), 20, axis=0)


def build_inputs():
    """name -> list of dict(ang (7,), pose (5, 3), seg (4,), bounds (7, 2))"""
    a = build_families()["a"]
    rng = np.random.default_rng(20261101)
    out = {"a": [], "l": [], "n": []}
    L, N = a["ang"].shape[:2]
    for l in range(L):
        for n in range(N):
            j = l * N + n
            out["a"].append(dict(ang=a["ang"][l, n], seg=a["seg"][l], bounds=WIDE,
                                 pose=_targets(rng, a["ang"][l, n], a["seg"][l], a["pose"][l, n, 0], j)))
    for l in range(3):
        ang, seg = a["ang"][l, 7], a["seg"][l]
        fr = numpy_frames(ang, seg)
        S = np.cumsum(np.abs(seg))
        for dof in range(7):
            s = dof // 2
            link, col = ((1, 0), (2, 1), (3, 2), (4, 1), (5, 2), (6, 1), (7, 1))[dof]
            Ja = np.cross(fr[link, :, col], fr[KEY_LINKS[s], :, 3] - fr[link, :, 3])
            for place in ("lb", "lb+1e-9", "ub-1e-9", "lb+1e-3"):
                for sign in (1.0, -1.0):
                    bounds = WIDE.copy()
                    if place == "ub-1e-9":
                        bounds[dof, 1] = ang[dof] + 1e-9
                    else:
                        bounds[dof, 0] = ang[dof] - {"lb": 0.0, "lb+1e-9": 1e-9, "lb+1e-3": 1e-3}[place]
                    pose = _targets(rng, ang, seg, np.zeros(3), 0)
                    pose[s + 1] = fr[KEY_LINKS[s], :, 3] - sign * 1e-2 * S[s] * Ja / np.linalg.norm(Ja)   # r = sign ... J_a
                    out["l"].append(dict(ang=ang, seg=seg, bounds=bounds, pose=pose, dof=dof, place=place, sign=sign))
        # the claw's target pulled back past the tibia end along the tarsus: stage 4 sits on a maximum (G < 0)
        pose = _targets(rng, ang, seg, np.zeros(3), 0)
        pose[4] = fr[8, :, 3] - 1.5 * (fr[8, :, 3] - fr[7, :, 3])
        out["l"].append(dict(ang=ang, seg=seg, bounds=WIDE, pose=pose))
    n_ang, n_seg = near_singular_postures()
    for j in range(len(n_ang)):
        out["n"].append(dict(ang=n_ang[j], seg=n_seg[j], bounds=WIDE, pose=_targets(rng, n_ang[j], n_seg[j], np.zeros(3), j)))
    assert [len(out[k]) for k in FAMILIES] == [390, 171, 60]
    return out


@pytest.fixture(scope="module")
def inputs():
    return build_inputs()


_TRUTH = {}


def truth(inputs, name):
    if name not in _TRUTH:
        _TRUTH[name] = [mp_rule(i["ang"], i["pose"], i["seg"], i["bounds"]) for i in inputs[name]]
    return _TRUTH[name]


# -------------------------------------------------------- checks --------------------------------------------------------

def consistent_with_its_own_flags(sens, flags):
    """What the flags say about the record: a held DOF's row is +0.0; the free rows of a stage that is not positive
    definite are NaN in the stage's own key point."""
    for d in range(7):
        if flags >> d & 1 and sens[d].view(np.uint64).any():
            return False
    for s, own in enumerate(STAGE_DOFS):
        for d in own:
            if flags >> (8 + s) & 1 and not flags >> d & 1 and not np.isnan(sens[d, s]).all():
                return False
    return True


def worst_ratio(inputs, name, got_sens, got_flags):
    """-> (worst error / (u kappa max|truth|), number of inputs compared on flags only); asserts flags, NaN pattern and
    exact zeros on the way."""
    worst, flags_only = 0.0, 0
    for j, (inp, tr) in enumerate(zip(inputs[name], truth(inputs, name))):
        s = got_sens[j]
        if tr["margin"] < FLIP:
            flags_only += 1
            assert consistent_with_its_own_flags(s, int(got_flags[j])), (name, j)
            continue
        assert int(got_flags[j]) == tr["flags"], (name, j, hex(int(got_flags[j])), hex(tr["flags"]))
        assert np.array_equal(np.isnan(s), np.isnan(tr["sens"])), (name, j)
        kappa = np.cumprod(tr["kappa"])
        for st, own in enumerate(STAGE_DOFS):
            t_rows, g_rows = tr["sens"][list(own)], s[list(own)]
            ok = ~np.isnan(t_rows)
            if not ok.any():
                continue
            scale = np.abs(t_rows[ok]).max()
            err = np.abs(g_rows[ok] - t_rows[ok]).max()
            if scale == 0.0:
                assert err == 0.0, (name, j, st)
                continue
            worst = max(worst, err / (U * kappa[st] * scale))
        for d in range(7):
            if tr["flags"] >> d & 1:
                assert not s[d].view(np.uint64).any(), (name, j, d)   # held: +0.0 by bits
    return worst, flags_only


def numpy_run(inputs, name):
    out = [numpy_rule(i["ang"], i["pose"], i["seg"], i["bounds"]) for i in inputs[name]]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out])


def host_run(sh, inputs, name):
    out = [sh.run(i["ang"][None], i["pose"][None], i["seg"], i["bounds"]) for i in inputs[name]]
    return np.concatenate([o[0] for o in out]), np.concatenate([o[2] for o in out])


def test_k_ref_is_measured_on_the_numpy_restatement(inputs):
    worst, flags_only = {}, 0
    for name in FAMILIES:
        worst[name], n = worst_ratio(inputs, name, *numpy_run(inputs, name))
        flags_only += n
    total = sum(len(inputs[n]) for n in FAMILIES)
    print("\n[sensitivity accuracy] numpy restatement, worst error / (u kappa max|truth|): " +
          ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f"; verdicts within 1e3 u of flipping: {flags_only} of {total}")
    # K_REF is the smallest power of two that held the restatement when the bound was set (10.38): a numpy or LAPACK on
    # which it needs more would loosen every bound of this module, and that must not pass unseen
    assert K_REF / 2 < max(worst.values()) <= K_REF and K == 4 * K_REF
    assert flags_only <= 0.02 * total


def test_the_families_reach_every_branch_of_the_rule(inputs):
    """Held at lb, lb + 1e-9 and ub - 1e-9 with the pushing sign of g and only there; stages that are not at a strict
    minimum; NaN inherited by later stages; kappa from 1 to beyond 1e6."""
    for inp, tr in zip(inputs["l"], truth(inputs, "l")):
        if "dof" not in inp:
            assert tr["flags"] == 1 << 11 and np.isnan(tr["sens"][6]).all()
            continue
        pushing = inp["sign"] > 0 if inp["place"].startswith("lb") else inp["sign"] < 0
        expect = inp["place"] != "lb+1e-3" and pushing
        assert bool(tr["flags"] >> inp["dof"] & 1) == expect, (inp["dof"], inp["place"], inp["sign"], hex(tr["flags"]))
    flags = np.array([t["flags"] for n in FAMILIES for t in truth(inputs, n)])
    for s in range(4):
        assert (flags >> (8 + s) & 1).any(), s
    assert any(np.isnan(t["sens"][6, 0]).all() and not t["flags"] >> 11 & 1 and np.isfinite(t["sens"][6, 3]).all()
               for t in truth(inputs, "a"))
    kappa = np.array([np.prod(t["kappa"]) for n in FAMILIES for t in truth(inputs, n)])
    assert kappa.min() >= 1 and kappa.max() > 1e6


@pytest.mark.parametrize("name", FAMILIES)
def test_host_rule_inside_the_bound(sens_harness, inputs, name):  # noqa: F811
    sens, flags = host_run(sens_harness, inputs, name)
    worst, flags_only = worst_ratio(inputs, name, sens, flags)
    print(f"\n[sensitivity accuracy] host build, family {name}: worst error / (u kappa max|truth|) {worst:.3f} (K = {K}); "
          f"{flags_only} of {len(inputs[name])} on flags only")
    assert worst <= K
    zero = np.broadcast_to(structural_zero_mask()[None, :, :, None], sens.shape)
    assert not sens.view(np.uint64)[zero].any()          # structural zeros: +0.0 by bits
    assert (sens[~zero] != 0).any()


def _batch(inputs, name, pick):
    """ang (n, 7), pose (n, 5, 3) and the leg (seg, bounds) of the first of the inputs ``pick`` of a family"""
    sel = [inputs[name][j] for j in pick]
    return np.stack([i["ang"] for i in sel]), np.stack([i["pose"] for i in sel]), sel[0]["seg"], sel[0]["bounds"]


def test_host_scaling_by_powers_of_two_is_exact(sens_harness, inputs):  # noqa: F811
    """Segment lengths and key points times 2^k: S times 2^-k bit for bit, the flags unchanged (leg 0 of family a, and the
    limit family's leg 0 with its held joints)."""
    for name, pick in (("a", range(130)), ("l", range(56))):
        for j in ([None] if name == "a" else pick):
            ang, pose, seg, bounds = _batch(inputs, name, pick if j is None else [j])
            ref, _, f0 = sens_harness.run(ang, pose, seg, bounds)
            for k in (-20, 1, 20):
                got, _, f = sens_harness.run(ang, pose * 2.0 ** k, seg * 2.0 ** k, bounds)
                assert same_bits(got, ref * 2.0 ** -k) and np.array_equal(f, f0), (name, j, k)


def check_bad_input(run, inputs):
    """``run(ang (n, 7), pose (n, 5, 3), sigma (n, 4), seg, bounds) -> sens, std, flags``: a non-finite or out-of-domain
    value in one leg-frame makes that record NaN with bit 16 alone; every other record keeps its bits."""
    ang, pose, seg, bounds = _batch(inputs, "a", range(130))
    sigma = np.random.default_rng(5).uniform(0.01, 0.1, (130, 4))
    s0, d0, f0 = run(ang, pose, sigma, seg, bounds)
    assert np.isfinite(d0[np.isfinite(s0).all(axis=(1, 2, 3))]).all() and not (f0 & BAD_INPUT).any()
    hit_frames = [0, 15, 16, 63, 64, 129]
    hit = np.zeros(130, bool)
    hit[hit_frames] = True
    cases = [("ang", d, v) for d in (0, 3, 6) for v in OUTSIDE]
    cases += [("pose", i, v) for i in (0, 4, 14) for v in (np.nan, np.inf, -np.inf)]
    cases += [("sigma", k, v) for k in (0, 3) for v in (np.nan, np.inf)]
    for what, idx, val in cases:
        a, p, g = ang.copy(), pose.copy(), sigma.copy()
        dict(ang=a, pose=p.reshape(130, 15), sigma=g)[what][hit, idx] = val
        s, d, f = run(a, p, g, seg, bounds)
        assert np.isnan(s[hit]).all() and np.isnan(d[hit]).all() and (f[hit] == BAD_INPUT).all(), (what, idx, val)
        assert same_bits(s[~hit], s0[~hit]) and same_bits(d[~hit], d0[~hit]) and np.array_equal(f[~hit], f0[~hit]), (what, idx, val)


def test_host_bad_input_makes_that_leg_frame_nan(sens_harness, inputs):  # noqa: F811
    check_bad_input(lambda a, p, g, seg, b: sens_harness.run(a, p, seg, b, kp_sigma=g), inputs)
    # a sigma that is not read (no std asked for) does not count
    ang, pose, seg, bounds = _batch(inputs, "a", range(16))
    assert not (sens_harness.run(ang, pose, seg, bounds)[2] & BAD_INPUT).any()


# ---------------------------------------------------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(hiplib):
    return gpu_lib(hiplib)


def device_run(lib, inputs, name):
    """One call per run of inputs with the same leg (segment lengths and limits)."""
    items = inputs[name]
    sens, flags, start = np.empty((len(items), 7, 4, 3)), np.empty(len(items), np.int32), 0
    same = lambda i, j: np.array_equal(items[i]["seg"], items[j]["seg"]) and np.array_equal(items[i]["bounds"], items[j]["bounds"])  # noqa: E731
    for j in range(1, len(items) + 1):
        if j == len(items) or not same(start, j):
            ang, pose, seg, bounds = _batch(inputs, name, range(start, j))
            out = lib.fit_sensitivity(ang[None, None], pose[None, None], [lib.leg_params_from_arrays(seg, bounds, np.zeros(27))])
            sens[start:j], flags[start:j] = out["sens"][0, 0], out["flags"][0, 0]
            start = j
    return sens, flags


@pytest.mark.gpu
@pytest.mark.parametrize("name", FAMILIES)
def test_gpu_output_inside_the_bound_and_equal_to_the_host_rule(lib, sens_harness, inputs, name):  # noqa: F811
    sens, flags = device_run(lib, inputs, name)
    worst, flags_only = worst_ratio(inputs, name, sens, flags)
    print(f"\n[sensitivity accuracy] device, family {name}: worst error / (u kappa max|truth|) {worst:.3f} (K = {K}); "
          f"{flags_only} of {len(inputs[name])} on flags only")
    assert worst <= K
    ref_s, ref_f = host_run(sens_harness, inputs, name)
    assert same_bits(sens, ref_s) and np.array_equal(flags, ref_f)


@pytest.mark.gpu
def test_gpu_bad_input_makes_that_leg_frame_nan(lib, inputs):
    def run(a, p, g, seg, b):
        out = lib.fit_sensitivity(a[None, None], p[None, None], [lib.leg_params_from_arrays(seg, b, np.zeros(27))],
                                  kp_sigma=g[None, None])
        return out["sens"][0, 0], out["std"][0, 0], out["flags"][0, 0]
    check_bad_input(run, inputs)
