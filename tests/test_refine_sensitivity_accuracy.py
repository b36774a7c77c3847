"""Error bars of the whole-leg refinement (include/seqik_refine_sensitivity.h): the host-run rule against a 200-bit
yardstick and against finite differences of the solver.  CPU tier; tests/test_refine_sensitivity.py holds the rest.

1. Yardstick: H, g, the held verdicts and sens at 200 bits on ``mp_chain`` with an mpmath linear solve
   (refine_sens_support.mp_rule, independent of csrc), on the 575 shipped frames and the 960 made-up leg-frames, all
   refined first by the host-run rule of seqik_refine.h.  The bar per leg-frame is 100 x the forward error of the float64
   numpy restatement against the same yardstick, relative to max |sens| of the leg-frame (never below 100 eps: the
   convention of the trajectory refinement's linear-solve test).  A leg-frame is skipped only when a verdict is not
   robust at 200 bits (mp_rule), at most 5 % of the cases.
2. Meaning: central differences (h = 1e-5 and 2e-5) of the float64 solver ``numpy_refine`` polished to gtol = 1e-15,
   ftol = 0, on frames 0, 400, ..., 5600 of RF and LF.  The host-run rule must lie closer to the h = 1e-5 differences
   than 10 x the distance between the two difference estimates, the Gauss-Newton rule at least 20 x farther than the
   host-run rule, and a held joint's row must be 0 in both.

Measured (profiles/refine_sensitivity_accuracy.json): see the docstrings."""
import numpy as np

from conftest import load_golden
from refine_sens_support import (EPS, FD_FRAMES, NOT_PD, mp_rule, numpy_rule, record, refine_rule_harness,  # noqa: F401
                                 refine_sens_harness, refined_inputs)
from refine_support import numpy_refine


def test_host_rule_against_the_200_bit_yardstick(refine_sens_harness, refine_rule_harness):  # noqa: F811
    """Measured (profiles/refine_sensitivity_accuracy.json, "yardstick"), relative to max |sens| of the leg-frame:
    restatement 1.7e-14, host build 2.6e-14 on the 575 shipped frames; 2.6e-6 / 5.1e-6 on the made-up legs (targets on
    the base make H_FF nearly singular); 890 leg-frames with a held joint, 96 not positive definite, every verdict
    equal; 9 of the 1535 leg-frames skipped."""
    worst = {}
    n_cases = n_skipped = n_held = n_not_pd = 0
    for name, q, pose, seg, b, _ in refined_inputs(refine_rule_harness):
        group = "shipped" if name in ("RF", "LF") else "made_up"
        got = refine_sens_harness.run(q, pose, seg, b)
        for i in range(len(q)):
            n_cases += 1
            mp = mp_rule(q[i], pose[i], seg, b)
            if not mp["robust"]:
                n_skipped += 1
                continue
            ref = numpy_rule(q[i], pose[i], seg, b)
            assert got["flags"][i] == mp["flags"], (name, i, got["flags"][i], mp["flags"])
            n_held += bool(mp["flags"] & 0x7F)
            n_not_pd += bool(mp["flags"] & NOT_PD)
            nan = np.isnan(mp["sens"])
            assert np.array_equal(np.isnan(got["sens"][i]), nan), (name, i)
            scale = np.abs(mp["sens"][~nan]).max() if (~nan).any() else 0.0
            if scale == 0.0:
                assert not got["sens"][i][~nan].any()
                continue
            err = np.abs(got["sens"][i] - mp["sens"])[~nan].max() / scale
            if ref["flags"] == mp["flags"]:
                err_ref = np.abs(ref["sens"] - mp["sens"])[~nan].max() / scale
            else:       # (the restatement's own verdict flipped: it sets no bar)
                err_ref = 0.0
            w = worst.setdefault(group, dict(restatement=0.0, host=0.0, grad=0.0))
            w["restatement"], w["host"] = max(w["restatement"], float(err_ref)), max(w["host"], float(err))
            assert err <= 100 * max(err_ref, EPS), (name, i, err, err_ref)
            # grad: g_a sums products |J| |r| <= len (len + |t|), each with a few eps of the chain's rounding, so grad's error
            # is a few eps (1 + |t| / len); 1e-12 max(1, |t| / len)^2 is above that
            gerr = abs(got["grad"][i] - mp["grad"])
            w["grad"] = max(w["grad"], float(gerr))
            assert gerr <= 1e-12 * max(1.0, np.abs(pose[i, 1:] - pose[i, 0]).max() / np.sum(seg)) ** 2, (name, i, gerr)
    print(f"{n_cases} leg-frames, {n_skipped} skipped, {n_held} with a held joint, {n_not_pd} not positive definite: {worst}")
    assert n_cases == 575 + 960 and n_skipped <= 0.05 * n_cases
    assert n_held > 50
    record("yardstick", dict(cases=n_cases, skipped=n_skipped, with_held_joint=n_held, not_positive_definite=n_not_pd,
                             relative_error=worst))


def test_the_rule_is_the_response_of_the_solver(refine_sens_harness):  # noqa: F811
    """Measured on the 30 frames (profiles/refine_sensitivity_accuracy.json, "solver"): the host-run rule 8.8e-5 ..
    2.9e-3 from the h = 1e-5 differences (entries up to 3.2), the two difference estimates 8.9e-5 .. 2.4e-3 apart,
    Gauss-Newton 0.13 .. 2.08 from the differences: 300 x .. 3400 x farther than the rule; 5 held rows."""
    z = load_golden("anipose_shipped")
    polish = dict(max_iter=2000, gtol=1e-15, ftol=0)
    rows, n_held_rows = [], 0
    for leg in ("RF", "LF"):
        seg, b = z[f"{leg}_seg"], z[f"{leg}_bounds"]
        for fr in FD_FRAMES:
            pose = z[f"{leg}_pose"][fr][:5]
            q = numpy_refine(z[f"{leg}_angles"][fr], pose, seg, b, **polish)[0]
            fd = {}
            for h in (1e-5, 2e-5):
                d = np.zeros((7, 4, 3))
                for k in range(4):
                    for c in range(3):
                        up, dn = pose.copy(), pose.copy()
                        up[k + 1, c] += h
                        dn[k + 1, c] -= h
                        d[:, k, c] = (numpy_refine(q, up, seg, b, **polish)[0] - numpy_refine(q, dn, seg, b, **polish)[0]) / (2 * h)
                fd[h] = d
            got = refine_sens_harness.run(q[None], pose[None], seg, b)
            sens, flags = got["sens"][0], int(got["flags"][0])
            gn = numpy_rule(q, pose, seg, b, curvature=False)["sens"]
            noise = np.abs(fd[1e-5] - fd[2e-5]).max()
            dist, dist_gn = np.abs(sens - fd[1e-5]).max(), np.abs(gn - fd[1e-5]).max()
            print(f"{leg} {fr}: flags {flags:#x} rule {dist:.3g} differences apart {noise:.3g} Gauss-Newton {dist_gn:.3g} "
                  f"max |sens| {np.abs(sens).max():.3g}")
            assert not flags & ~0x7F, (leg, fr, flags)
            assert dist < 10 * noise, (leg, fr, dist, noise)
            assert dist_gn >= 20 * dist, (leg, fr, dist_gn, dist)
            for d in range(7):
                if flags >> d & 1:
                    n_held_rows += 1
                    assert not sens[d].any() and not fd[1e-5][d].any() and not fd[2e-5][d].any(), (leg, fr, d)
            rows.append(dict(leg=leg, frame=int(fr), flags=flags, rule=float(dist), differences_apart=float(noise),
                             gauss_newton=float(dist_gn), largest_entry=float(np.abs(sens).max())))
    assert n_held_rows >= 3
    record("solver", rows)
