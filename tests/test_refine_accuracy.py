"""Whole-leg refinement against real scipy and a 200-bit gradient (include/seqik_refine.h), on the host-run rule
(tests/harness/refine_harness.hip; the GPU tier of tests/test_refine.py holds the kernel to it bit for bit).

Against scipy: the 575 frames of the shipped recording (refine_support.shipped_frames), ``least_squares(method="trf",
bounds, jac=analytic, xtol=ftol=1e-14, gtol=1e-12)`` from the same clamped start.  The bar is on the cost, cost[1] <=
scipy's x (1 + 1e-9) on every frame; the angles are recorded, not asserted (one LF frame of the singular episode is flat:
0.17 rad apart at the same cost).  No frame may stop on the iteration cap or on exhausted damping.

Yardstick: the gradient g = J^T r at the returned angles at 200 bits, for those 575 frames and the 960 made-up ones.  A
lane that stopped on the gradient test (reason 0) must meet it: free DOFs |g_j| <= gtol (seg_0 + .. + seg_3)^2, a DOF held
on its lower limit g_j >= 0, on its upper limit g_j <= 0 -- up to the float64 rounding of g, which the test measures as
E = max |g_float64 - g_200bit| / (len (len + |r|)) over every lane and DOF (g_float64: the numpy restatement's gradient at
the same angles; len the leg length, |r| the residual norm: |g_j| <= |J_j| |r| with |J_j| <= len) and allows four times.
For a lane that stopped on the cost decrease (reason 1) the projected gradient is recorded, not barred.

``python tests/test_refine_accuracy.py`` writes the figures to profiles/refine_vs_scipy.json."""
import json
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import conftest  # noqa: F401  (puts the package on the path)

from refine_support import (GTOL, RefineHarness, held_bits, iterations, made_up_legs, mp_gradient, numpy_model, reason,  # noqa: F401
                            refine_harness, scipy_refine, shipped_frames, targets_of)

_SCIPY, _GRAD = {}, {}


def against_scipy(rh):
    """Per leg: the harness's answer and scipy's on the shipped frames (computed once)."""
    if not _SCIPY:
        for leg, fr, ang, pose, seg, bounds in shipped_frames():
            out, cost, info = rh.run(ang, pose, seg, bounds)
            sc = [scipy_refine(ang[i], pose[i], seg, bounds) for i in range(len(ang))]
            _SCIPY[leg] = dict(frames=fr, out=out, cost=cost, info=info, scipy_x=np.array([s[0] for s in sc]),
                               scipy_cost=np.array([s[1] for s in sc]))
    return _SCIPY


def gradients(rh):
    """Per data set ("shipped", "made_up"): per lane the 200-bit gradient at the returned angles, the float64 one, the
    unit len (len + |r|), the bar gtol len^2, the info word and which DOFs sit on which limit (computed once)."""
    if not _GRAD:
        sets = {"shipped": [(a, p, s, b) for _, _, a, p, s, b in shipped_frames()], "made_up": made_up_legs()}
        for name, legs in sets.items():
            rows = dict(g=[], g64=[], unit=[], bar=[], info=[], at_lb=[], at_ub=[])
            for ang, pose, seg, bounds in legs:
                out, cost, info = rh.run(ang, pose, seg, bounds)
                length = float(np.sum(seg))
                for i in range(len(ang)):
                    r, J = numpy_model(out[i], targets_of(pose[i], np.ones(4)), np.ones(4), seg)
                    rows["g"].append(mp_gradient(out[i], pose[i], seg))
                    rows["g64"].append(J.T @ r)
                    rows["unit"].append(length * (length + np.linalg.norm(r)))
                    rows["bar"].append(GTOL * length ** 2)
                    rows["info"].append(info[i])
                    rows["at_lb"].append(out[i] == bounds[:, 0])
                    rows["at_ub"].append(out[i] == bounds[:, 1])
            _GRAD[name] = {k: np.array(v) for k, v in rows.items()}
    return _GRAD


def gradient_figures(d):
    """-> (E, the largest violation of the three conditions by a reason-0 lane in units of its `unit`, the largest
    projected gradient of a reason-1 lane in units of its bar)"""
    E = float((np.abs(d["g64"] - d["g"]) / d["unit"][:, None]).max())
    held = held_bits(d["info"])
    lower, upper, free = held & d["at_lb"], held & d["at_ub"], ~held
    # what a lane's gradient is short of its condition by, >= 0 (0: met exactly)
    short = np.where(free, np.maximum(np.abs(d["g"]) - d["bar"][:, None], 0.0), 0.0)
    short = np.where(lower, np.maximum(-d["g"], 0.0), short)
    short = np.where(upper, np.maximum(d["g"], 0.0), short)
    assert (held == (lower | upper)).all()          # a held DOF sits on one of its limits
    r0, r1 = reason(d["info"]) == 0, reason(d["info"]) == 1
    worst0 = float((short[r0] / d["unit"][r0, None]).max())
    projected = np.where(free, np.abs(d["g"]), 0.0).max(1) / d["bar"]
    return E, worst0, float(projected[r1].max()) if r1.any() else 0.0


def scipy_figures(res):
    out = {}
    for leg, d in res.items():
        its = iterations(d["info"])
        out[leg] = {"frames": int(len(its)), "max_cost_over_scipy_cost_minus_1": float((d["cost"][:, 1] / d["scipy_cost"]).max() - 1.0),
                    "min_cost_over_scipy_cost_minus_1": float((d["cost"][:, 1] / d["scipy_cost"]).min() - 1.0),
                    "stop_reasons": {str(k): int(v) for k, v in enumerate(np.bincount(reason(d["info"]), minlength=5)) if v},
                    "iterations_median": float(np.median(its)), "iterations_max": int(its.max()),
                    "iterations_histogram_by_10": np.bincount(its // 10).tolist(),
                    "max_angle_difference_rad": float(np.abs(d["out"] - d["scipy_x"]).max()),
                    "frame_of_max_angle_difference": int(d["frames"][np.abs(d["out"] - d["scipy_x"]).max(1).argmax()]),
                    "median_angle_difference_rad": float(np.median(np.abs(d["out"] - d["scipy_x"]).max(1))),
                    "rms_key_point_distance_before": float(np.sqrt(d["cost"][:, 0].mean() / 4)),
                    "rms_key_point_distance_after": float(np.sqrt(d["cost"][:, 1].mean() / 4)),
                    "median_cost_after_over_before": float(np.median(d["cost"][:, 1] / d["cost"][:, 0])),
                    "frames_worse": int((d["cost"][:, 1] > d["cost"][:, 0]).sum())}
    return out


def test_the_rule_reaches_scipys_cost_on_the_shipped_frames(refine_harness):  # noqa: F811
    res = against_scipy(refine_harness)
    fig = scipy_figures(res)
    print(json.dumps(fig, indent=1))
    assert sum(f["frames"] for f in fig.values()) == 575
    for leg, d in res.items():
        assert (d["cost"][:, 1] <= d["scipy_cost"] * (1 + 1e-9)).all(), leg
        assert np.isin(reason(d["info"]), (0, 1)).all(), (leg, "a frame stopped on the cap or on damping")
        assert (d["cost"][:, 1] <= d["cost"][:, 0]).all()
    # what the refinement is for (the issue's table): the rms key-point distance roughly halves
    assert fig["RF"]["rms_key_point_distance_after"] < 0.6 * fig["RF"]["rms_key_point_distance_before"]
    assert fig["LF"]["rms_key_point_distance_after"] < 0.6 * fig["LF"]["rms_key_point_distance_before"]


def test_the_gradient_at_200_bits_meets_the_stop_test(refine_harness):  # noqa: F811
    for name, d in gradients(refine_harness).items():
        E, worst0, projected1 = gradient_figures(d)
        n0 = int((reason(d["info"]) == 0).sum())
        print(name, "lanes", len(d["info"]), "reason 0:", n0, "E", E, "worst shortfall of a reason-0 lane / unit", worst0,
              "largest projected gradient of a reason-1 lane / bar", projected1)
        assert n0 >= 60, name
        assert 0.0 < E < 1e-14, (name, E)         # a rounding error, not a mistake of the restatement
        assert worst0 <= 4 * E, (name, worst0, E)


if __name__ == "__main__":
    from harness_build import build_harness
    from conftest import ROOT
    rh = RefineHarness(build_harness(os.path.join(ROOT, "tests", "harness", "refine_harness.hip")),
                       build_harness(os.path.join(ROOT, "tests", "harness", "fk_harness.hip")))
    report = {"what": "tests/test_refine_accuracy.py: the host-run rule of csrc/seqik_refine.hpp against scipy.optimize.least_squares "
                      "(TRF, bounds, analytic Jacobian, xtol = ftol = 1e-14, gtol = 1e-12) on 575 frames of "
                      "tests/golden/anipose_shipped.npz, and its stop test against the gradient at 200 bits",
              "against_scipy": scipy_figures(against_scipy(rh)), "gradient_at_200_bits": {}}
    for name, d in gradients(rh).items():
        E, worst0, projected1 = gradient_figures(d)
        report["gradient_at_200_bits"][name] = {
            "lanes": int(len(d["info"])), "lanes_stopped_on_the_gradient_test": int((reason(d["info"]) == 0).sum()),
            "rounding_of_g_E": E, "asserted_bound_4E": 4 * E, "worst_shortfall_of_a_reason_0_lane": worst0,
            "largest_projected_gradient_of_a_reason_1_lane_in_units_of_the_bar": projected1,
            "stop_reasons": {str(k): int(v) for k, v in enumerate(np.bincount(reason(d["info"]), minlength=5)) if v}}
    with open(os.path.join(ROOT, "profiles", "refine_vs_scipy.json"), "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report, indent=1))
