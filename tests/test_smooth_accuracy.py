"""Trajectory refinement against real scipy on the stacked problem (include/seqik_smooth.h; the rule run on the host,
tests/harness/smooth_harness.hip).

``scipy.optimize.least_squares`` (TRF, bounds, analytic Jacobian of the stacked residuals -- the 12 data residuals of every
frame plus sqrt(s_j) times the differences of neighbouring frames --, xtol = ftol = 1e-14, gtol = 1e-12) from the same
clamped sequential start, on the four RF windows of the shipped recording on which the sequential fit jumps by 2.6 rad, and
on LF 276:308 with the accepted steps capped at 200.  LF 276:308 at smooth = 0.01 is NOT compared: from the sequential
start this rule and scipy end in different local minima there, which is the limit of any local method.

The bars are those of the whole-leg refinement's scipy test: the cost to 1e-9 relative, the angles and the largest
frame-to-frame change to 1e-4 rad.  Measured (profiles/smooth_vs_scipy.json): cost within 3e-13, angles within 1.4e-6 rad,
the largest change within 2e-7 rad; LF capped at 200 steps: cost within 1.5e-12."""
import numpy as np
import pytest

from smooth_support import largest_change, record, scipy_smooth, shipped_window, smooth_harness  # noqa: F401

WINDOWS = [("RF", 272, 296, 0.1), ("RF", 1210, 1243, 0.1), ("RF", 272, 296, 1.0), ("RF", 272, 296, 0.01)]


@pytest.mark.parametrize("leg,lo,hi,smooth", WINDOWS)
def test_shipped_windows_reach_scipys_minimum(smooth_harness, leg, lo, hi, smooth):  # noqa: F811
    ang, pose, seg, bounds = shipped_window(leg, lo, hi)
    res = smooth_harness.run_one(ang, pose, seg, bounds, smooth=smooth)
    x, c = scipy_smooth(ang, pose, seg, bounds, smooth)
    start = np.clip(ang, bounds[:, 0], bounds[:, 1])
    jump0, jump, jump_scipy = largest_change(start), largest_change(res["angles"]), largest_change(x)
    measured = dict(cost=float(res["cost"][1]), cost_vs_scipy=float((res["cost"][1] - c) / c), angles_vs_scipy=float(np.abs(res["angles"] - x).max()),
                    largest_change=[jump0, jump, jump_scipy], reason=int(res["info"][0]), steps=int(res["info"][1]),
                    rejected=int(res["info"][2]))
    print(leg, lo, hi, smooth, measured)
    record(f"{leg}_{lo}_{hi}_smooth_{smooth}", measured)
    assert abs(res["cost"][1] - c) <= 1e-9 * c
    assert np.abs(res["angles"] - x).max() <= 1e-4
    assert res["info"][0] in (0, 1)                         # never on the cap or on damping
    assert abs(jump - jump_scipy) <= 1e-4
    assert jump0 > 2.6                                      # the start does jump
    if smooth == 0.1 and lo == 272:
        assert jump < 0.5


def test_lf_window_capped_at_200_steps(smooth_harness):  # noqa: F811
    """LF 276:308 at smooth = 0.1 needs more than 200 accepted steps: capped there it reports the cap, at scipy's cost."""
    ang, pose, seg, bounds = shipped_window("LF", 276, 308)
    res = smooth_harness.run_one(ang, pose, seg, bounds, smooth=0.1, max_iter=200)
    x, c = scipy_smooth(ang, pose, seg, bounds, 0.1)
    measured = dict(cost=float(res["cost"][1]), cost_vs_scipy=float((res["cost"][1] - c) / c), angles_vs_scipy=float(np.abs(res["angles"] - x).max()),
                    reason=int(res["info"][0]), steps=int(res["info"][1]), rejected=int(res["info"][2]))
    print(measured)
    record("LF_276_308_smooth_0.1_max_iter_200", measured)
    assert tuple(res["info"][:2]) == (4, 200)
    assert abs(res["cost"][1] - c) <= 1e-9 * c
    # with the default cap it stops by itself, no higher
    full = smooth_harness.run_one(ang, pose, seg, bounds, smooth=0.1)
    assert full["info"][0] in (0, 1) and full["info"][1] > 200 and full["cost"][1] <= res["cost"][1]
