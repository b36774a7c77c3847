"""CPU tier: the C oracle against (1) the shipped outputs of the reference pipeline and (2) the
reference's own source re-run in the build container over real scipy (tests/golden/*.npz)."""
import numpy as np
import pytest

from conftest import good_frames, leg_arrays, load_golden

TOL = 1e-4  # rad -- BASELINE.json north star


def test_sincos_is_accurate(oracle):
    rng = np.random.default_rng(0)
    xs = np.concatenate([rng.uniform(-3.3, 3.3, 20000), [0.0, np.pi, -np.pi, np.pi / 2, -np.pi / 2, 1e-300]])
    sc = np.array([oracle.sincos(x) for x in xs])
    assert np.all(np.abs(sc[:, 0] - np.sin(xs)) <= np.spacing(np.abs(np.sin(xs))) + 1e-300)
    assert np.all(np.abs(sc[:, 1] - np.cos(xs)) <= np.spacing(np.abs(np.cos(xs))) + 1e-300)
    assert oracle.sincos(0.0) == (0.0, 1.0)


@pytest.mark.parametrize("leg", ["RF", "LF"])
def test_oracle_vs_shipped_anipose_golden(oracle, leg):
    """leg_joint_angles.pkl / forward_kinematics.pkl shipped with the reference (6000 frames)."""
    z = load_golden("anipose_shipped")
    r = oracle.seq_leg(*leg_arrays(z, leg))
    ok = good_frames(leg, 6000)
    err = np.abs(r["angles"] - z[f"{leg}_angles"])
    assert err[ok].max() < TOL
    # outside the documented degenerate episode nothing may exceed the bar; inside, only there
    bad = np.where(err.max(1) >= TOL)[0]
    assert np.all(~ok[bad])
    cut = z["fk_frames"]
    fk_err = np.abs(r["fk"][cut] - z[f"{leg}_fk_cut"])
    assert fk_err[ok[cut]].max() < TOL


@pytest.mark.parametrize("name", ["anipose_scipy_cut", "df3d_100", "df3d_1000"])
def test_oracle_vs_reference_source_run(oracle, name):
    """Outputs of the reference's LegInvKinSeq/KinematicChainSeq source, run over real scipy."""
    z = load_golden(name)
    for leg in z["legs"]:
        leg = str(leg)
        r = oracle.seq_leg(*leg_arrays(z, leg))
        n = r["angles"].shape[0]
        ok = good_frames(leg, n) if name.startswith("anipose") else np.ones(n, bool)
        assert np.abs(r["angles"] - z[f"{leg}_angles"])[ok].max() < TOL, leg
        assert np.abs(r["fk"] - z[f"{leg}_fk"])[ok].max() < TOL, leg
        # stage 1 (exact-zero singular values) and stage 4 (one unknown) follow scipy's iteration
        # path itself, not just its answer: same number of function evaluations
        same = (r["nfev"] == z[f"{leg}_nfev"])[ok].mean(0)
        assert same[0] > 0.97 and same[3] > 0.97, (leg, same)
        assert set(np.unique(r["status"])) <= {1, 2, 3, 4}


def test_oracle_stage_subsets_compose(oracle):
    z = load_golden("df3d_100")
    pose, seg, b, seeds = leg_arrays(z, "RM")
    full = oracle.seq_leg(pose, seg, b, seeds)
    a = oracle.seq_leg(pose, seg, b, seeds, 1, 2, want_fk=False)
    c = oracle.seq_leg(pose, seg, b, seeds, 3, 4, prior_angles=a["angles"])
    assert np.array_equal(c["angles"], full["angles"])
    assert np.array_equal(c["fk"], full["fk"])


def test_oracle_rejects_seed_outside_bounds(oracle):
    z = load_golden("df3d_100")
    pose, seg, b, seeds = leg_arrays(z, "RF")
    bad = seeds.copy()
    bad[1] = b[0, 1] + 0.1  # stage-1 yaw seed above its upper bound
    with pytest.raises(ValueError, match="outside of provided bounds"):
        oracle.seq_leg(pose[:2], seg, b, bad)


def test_oracle_empty_input(oracle):
    z = load_golden("df3d_100")
    pose, seg, b, seeds = leg_arrays(z, "RF")
    r = oracle.seq_leg(pose[:0], seg, b, seeds)
    assert r["angles"].shape == (0, 7)


def test_algorithm_variants_kept_as_hooks(oracle):
    """The restatement's deliberate departures from "scipy verbatim" stay checkable:
      * the root-search shortcut (Gauss-Newton step inside the trust region: ten resets + one Newton step) gives
        the SAME BITS as the verbatim ten iterations -- angles, FK, status, nfev -- on recordings, synthetic data
        and made-up legs with nasty targets;
      * the closed-form 2 x 2 trust-region step follows the one-sided Jacobi SVD variant to < 1e-5 rad on the
        recordings (same evaluation counts on > 99 % of the solves);
      * the generic chain's SVD-free step reaches the same claw positions as its SVD variant."""
    from conftest import random_leg_case
    try:
        cases, refs = [], []
        for name in ("anipose_shipped", "anipose_scipy_cut", "df3d_100", "df3d_1000"):   # every fixture, full length
            z = load_golden(name)
            for leg in [str(l) for l in z["legs"]]:
                cases.append((z[f"{leg}_pose"], z[f"{leg}_seg"], z[f"{leg}_bounds"], z[f"{leg}_seeds"]))
                refs.append((name, leg, z[f"{leg}_angles"]))
        n_fixture = len(cases)
        rng = np.random.default_rng(5)
        cases += [random_leg_case(rng, 40) for _ in range(150)]
        for c in cases:
            oracle.set_variant(tr2_shortcut=False)
            a = oracle.seq_leg(*c)
            oracle.set_variant(tr2_shortcut=True)
            b = oracle.seq_leg(*c)
            for k in ("angles", "fk", "status", "nfev"):
                assert np.array_equal(a[k], b[k]), k
        worst = 0.0
        for c, (name, leg, ref) in zip(cases[:n_fixture], refs):
            # scipy's loop verbatim (one-sided Jacobi SVD of the augmented matrix + the ten-iteration root search)
            oracle.set_variant(closed_form_2x2=False, tr2_shortcut=False)
            a = oracle.seq_leg(*c)
            oracle.set_variant(closed_form_2x2=True, tr2_shortcut=True)
            b = oracle.seq_leg(*c)
            ok = good_frames(leg, len(ref)) if name.startswith("anipose") else np.ones(len(ref), bool)
            assert np.abs(a["angles"] - b["angles"])[ok].max() < 1e-5, (name, leg)
            assert (a["nfev"] == b["nfev"]).mean() > 0.99
            # ... and the verbatim variant is exactly as far from the reference outputs as the default one
            assert np.abs(a["angles"] - ref)[ok].max() < 1e-4, (name, leg)
            worst = max(worst, np.abs(a["angles"] - ref)[ok].max())
        assert worst < 9e-5   # profiles/r02_oracle_variants.json: 8.39e-5 for the default and the verbatim variant alike
        zg = load_golden("generic_rf_100")
        oracle.set_variant(generic_svd=True)
        a = oracle.generic_leg(zg["RF_pose"], zg["RF_seg"], zg["RF_bounds"], zg["RF_seeds"][18:27])
        oracle.set_variant(generic_svd=False)
        b = oracle.generic_leg(zg["RF_pose"], zg["RF_seg"], zg["RF_bounds"], zg["RF_seeds"][18:27])
        assert np.abs(a["fk"][:, 8] - b["fk"][:, 8]).max() < 1e-6
        # round 4: the generic chain's forward kinematics evaluated right to left as a vector and the 3 x 3 step in its
        # second push-through form (form 1; the default is form 0 again, tests/test_generic_answers.py) are other
        # association orders of the same numbers: same claw (1e-6), comparable evaluation counts; the angles -- which the
        # reference itself does not reproduce -- may differ
        for kw in (dict(generic_rtl=False), dict(woodbury_form=1), dict(generic_rtl=False, woodbury_form=1)):
            oracle.set_variant(**kw)
            a = oracle.generic_leg(zg["RF_pose"], zg["RF_seg"], zg["RF_bounds"], zg["RF_seeds"][18:27])
            oracle.reset_variants()
            assert np.abs(a["fk"][:, 8] - b["fk"][:, 8]).max() < 1e-6, kw
            assert np.abs(a["fk"][:, 8] - zg["RF_fk"][:, 8]).max() < 1e-6, kw
            assert 0.8 < a["nfev"].mean() / b["nfev"].mean() < 1.25, kw
    finally:
        oracle.reset_variants()
