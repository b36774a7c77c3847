"""The sensitivity rule describes the solver: central differences of the C oracle against the host-run rule (CPU tier).

include/seqik_sensitivity.h defines d (fitted angle) / d (aligned key point) in closed form.  Here the sequential solver
itself -- ``oracle.seq_leg``, the C restatement of the reference -- is differentiated numerically and compared with
csrc/seqik_sensitivity.hpp run on the host (tests/harness/sensitivity_harness.hip).

FRAMES.  df3d_100 RF and LM at frames 5, 40, 77; anipose_scipy_cut RF 63, 129, 215, 329 and LF 45, 249, 268, 329, which
have TiTa_pitch (RF 63, 129, 215; LF 45, 249, 268) or CTr_roll (frame 329 of both) on a limit: 14 frames.
TRUTH.  Central differences, h = 1e-3, of the oracle's angles of frame t on the recording's prefix 0 .. t with one
key-point coordinate of frame t moved (12 coordinates, 24 solves of the prefix per frame).
TOLERANCE.  The worst disagreement of the float64 numpy restatement of the rule (tests/sensitivity_support.numpy_rule)
with those differences, measured: 8.06e-3 (RF 77 of df3d_100; the solver's termination noise dominates -- most frames
agree to 1e-3 or better), kept as MEASURED = 8.1e-3; the host-run rule must agree within TOL = 4 x MEASURED.
THE WRONG RULES on the same frames: Gauss-Newton, i.e. without the residual-times-curvature term, disagrees with the
differences by 0.198 .. 1.98 (smallest: LM 5 of df3d_100); ignoring the held joints by 2.56 .. 4.92 on the limit frames
(one of them, LF 268, is then not even at a minimum: NaN).  MEASURED lies below a tenth of the smaller of the two,
0.0198, and TOL below a sixth of it."""
import numpy as np
import pytest

from conftest import leg_arrays, load_golden
from sensitivity_support import numpy_rule, sens_harness  # noqa: F401

H = 1e-3
MEASURED = 8.1e-3          # worst |numpy restatement - central differences| over the 14 frames (8.06e-3)
TOL = 4 * MEASURED
WRONG_GN, WRONG_HOLD = 0.198, 2.56   # the smallest disagreement of each wrong rule, as measured
TITA, CTR_ROLL = 6, 4
FRAMES = [("df3d_100", "RF", 5, None), ("df3d_100", "RF", 40, None), ("df3d_100", "RF", 77, None),
          ("df3d_100", "LM", 5, None), ("df3d_100", "LM", 40, None), ("df3d_100", "LM", 77, None),
          ("anipose_scipy_cut", "RF", 63, TITA), ("anipose_scipy_cut", "RF", 129, TITA),
          ("anipose_scipy_cut", "RF", 215, TITA), ("anipose_scipy_cut", "RF", 329, CTR_ROLL),
          ("anipose_scipy_cut", "LF", 45, TITA), ("anipose_scipy_cut", "LF", 249, TITA),
          ("anipose_scipy_cut", "LF", 268, TITA), ("anipose_scipy_cut", "LF", 329, CTR_ROLL)]


@pytest.fixture(scope="module")
def cases(oracle):
    """Per frame: dict(angles (7,), pose (5, 3), seg, bounds, fd (7, 4, 3), on_limit) -- computed once."""
    out = []
    for fixture, leg, t, on_limit in FRAMES:
        pose, seg, bounds, seeds = leg_arrays(load_golden(fixture), leg)
        pose = np.array(pose[:t + 1], dtype=np.float64)
        angles = oracle.seq_leg(pose, seg, bounds, seeds, want_fk=False)["angles"][t]
        fd = np.zeros((7, 4, 3))
        for k in range(1, 5):
            for c in range(3):
                side = []
                for sign in (1.0, -1.0):
                    moved = pose.copy()
                    moved[t, k, c] += sign * H
                    side.append(oracle.seq_leg(moved, seg, bounds, seeds, want_fk=False)["angles"][t])
                fd[:, k - 1, c] = (side[0] - side[1]) / (2 * H)
        out.append(dict(name=f"{fixture} {leg} {t}", angles=angles, pose=pose[t], seg=seg, bounds=bounds, fd=fd,
                        on_limit=on_limit))
    return out


def _worst(a, b):
    """max |a - b|; a NaN anywhere counts as an infinite disagreement"""
    d = np.abs(a - b)
    return np.inf if np.isnan(d).any() else float(d.max())


def test_the_tolerance_is_measured_on_the_numpy_restatement_and_separates_the_wrong_rules(cases):
    exact = {c["name"]: _worst(numpy_rule(c["angles"], c["pose"], c["seg"], c["bounds"])[0], c["fd"]) for c in cases}
    gauss_newton = {c["name"]: _worst(numpy_rule(c["angles"], c["pose"], c["seg"], c["bounds"], curvature=False)[0], c["fd"])
                    for c in cases}
    no_hold = {c["name"]: _worst(numpy_rule(c["angles"], c["pose"], c["seg"], c["bounds"], hold=False)[0], c["fd"])
               for c in cases if c["on_limit"] is not None}
    print("\n[sensitivity solver] |rule - central differences|, worst entry per frame:")
    for name in exact:
        print(f"    {name:28s} exact {exact[name]:.3g}   Gauss-Newton {gauss_newton[name]:.3g}   " +
              (f"no held joints {no_hold[name]:.3g}" if name in no_hold else ""))
    assert max(exact.values()) <= MEASURED, exact
    assert min(gauss_newton.values()) >= WRONG_GN * 0.99 and min(no_hold.values()) >= WRONG_HOLD * 0.99
    wrong = min(min(gauss_newton.values()), min(no_hold.values()))
    assert MEASURED < wrong / 10 and TOL < wrong / 6, (MEASURED, TOL, wrong)


def test_the_host_rule_agrees_with_the_solvers_own_differences(sens_harness, cases):  # noqa: F811
    for c in cases:
        sens, _, flags = sens_harness.run(c["angles"][None], c["pose"][None], c["seg"], c["bounds"])
        worst = _worst(sens[0], c["fd"])
        print(f"\n[sensitivity solver] host build, {c['name']}: {worst:.3g} (TOL = {TOL:.3g}), flags {int(flags[0]):#x}")
        assert worst <= TOL, (c["name"], worst)
        # the flags name the DOF the oracle leaves at its limit, that row is exactly 0, and nothing else is held
        if c["on_limit"] is None:
            assert flags[0] == 0, (c["name"], hex(int(flags[0])))
        else:
            d = c["on_limit"]
            assert flags[0] == 1 << d, (c["name"], hex(int(flags[0])))
            assert min(c["angles"][d] - c["bounds"][d][0], c["bounds"][d][1] - c["angles"][d]) <= 1e-6
            assert not sens[0, d].any(), c["name"]
            # the oracle keeps the angle strictly inside, within bound_tol of the limit on both sides of the difference
            assert np.abs(c["fd"][d]).max() <= 1e-6 / H, c["name"]
