"""Accuracy of the smoothed trajectory's error bars (include/seqik_smooth_sensitivity.h), CPU tier, on the host-run rule:
the linear part (Schur sweeps, combine, off-centre products, covariance sweeps) on caller-given blocks against a 200-bit
solve and against one dense numpy inverse, with the not-a-minimum verdicts; the whole rule against a 200-bit yardstick on
``mp_chain``; and the rule against central differences of the float64 host solver of seqik_smooth.h.

The bar of the first two is the issue's: 100 x the forward error of a float64 numpy restatement of the same recursions
against the 200-bit values, never below 100 eps, relative to the largest magnitude of the compared quantity in the
trajectory.  The measured values are kept in profiles/smooth_sensitivity_accuracy.json (SEQIK_RECORD_PROFILES=1)."""
import numpy as np
import pytest

from smooth_sens_support import (BAD_INPUT, EPS, IDENTITY_ROW, NOT_PD, banded, dense_linear, dense_mp, fd_polish, mp_trajectory,  # noqa: F401
                                 random_system, record, smooth_sens_harness, smoothed_window, sweeps_mp, sweeps_numpy)
from refine_sens_support import refine_sens_harness  # noqa: F401
from smooth_support import made_up_trajectories, shipped_window, smooth_harness  # noqa: F401

LINEAR_SIZES = (1, 2, 3, 4, 5, 7, 9, 16, 24, 33, 64, 65)
W_LINEAR = 4


def rel(a, b, scale):
    return float(np.abs(np.asarray(a, dtype=float) - np.asarray(b, dtype=float)).max() / scale)


def test_linear_part_against_a_200_bit_solve_and_dense_numpy(smooth_sens_harness):  # noqa: F811
    """Random symmetric positive definite block-tridiagonal systems, N = 1..65, with held masks, broken pairs and identity
    rows: every block G_ts B_s within the band (the first seven columns of B are the identity: G_ts itself) and the
    covariance diagonal."""
    worst = dict(sens=0.0, var=0.0, sens_numpy=0.0, var_numpy=0.0, sens_dense=0.0, var_dense=0.0)
    for N in LINEAR_SIZES:
        for seed in (N, 100 + N):
            H, word, s, B, sigma = random_system(N, seed)
            good = (word & IDENTITY_ROW) == 0
            sens, std, flags = smooth_sens_harness.linear(H, word, s, B, sigma, W_LINEAR)
            assert np.array_equal(flags[good], word[good] & 0x7F) and (flags[~good] == BAD_INPUT).all()
            truth_s, truth_v = sweeps_mp(H, word, s, B, sigma, W_LINEAR)
            np_s, np_v = sweeps_numpy(H, word, s, B, sigma, W_LINEAR)
            scale_s, scale_v = np.abs(truth_s[good]).max(), np.abs(truth_v[good]).max()
            e_np_s, e_np_v = rel(np_s[good], truth_s[good], scale_s), rel(np_v[good], truth_v[good], scale_v)
            e_s, e_v = rel(sens[good], truth_s[good], scale_s), rel(std[good] ** 2, truth_v[good], scale_v)
            print(f"N={N} seed={seed}: sens {e_s:.2e} (numpy {e_np_s:.2e}), var {e_v:.2e} (numpy {e_np_v:.2e})")
            assert e_s <= max(100 * e_np_s, 100 * EPS), (N, seed, e_s, e_np_s)
            assert e_v <= max(100 * e_np_v, 100 * EPS), (N, seed, e_v, e_np_v)
            # the same against ONE dense inverse: the recursions are the inverse's blocks, and std is inv(H) M inv(H)
            GB, var, pd = dense_linear(H, word, s, B, sigma)
            assert pd
            d_s, d_v = rel(sens[good], banded(GB, W_LINEAR)[good], scale_s), rel(std[good] ** 2, var[good], scale_v)
            cond = np.linalg.cond(dense_linear.last_matrix)
            assert d_s <= 100 * cond * EPS and d_v <= 100 * cond * EPS, (N, seed, d_s, d_v, cond)
            # the blocks of an identity row: inside the recording the one NaN, outside +0.0; and nothing reaches across it
            for t in np.where(~good)[0]:
                for d in range(2 * W_LINEAR + 1):
                    u = t + d - W_LINEAR
                    assert np.isnan(sens[t, d]).all() if 0 <= u < N else not sens[t, d].view(np.uint64).any()
                assert np.isnan(std[t]).all()
                for u in range(max(0, t - W_LINEAR), min(N, t + W_LINEAR + 1)):
                    if good[u]:
                        assert not sens[u, t - u + W_LINEAR].any()
            for k, v in (("sens", e_s), ("var", e_v), ("sens_numpy", e_np_s), ("var_numpy", e_np_v), ("sens_dense", d_s),
                         ("var_dense", d_v)):
                worst[k] = max(worst[k], v)
    record("linear_part", dict(sizes=list(LINEAR_SIZES), half_width=W_LINEAR, systems=2 * len(LINEAR_SIZES), worst=worst))


def test_the_200_bit_recursions_are_a_dense_200_bit_solve():
    """A self-check of the yardstick, not of the product (it runs test-support code only): the 200-bit recursions equal a
    dense 200-bit inverse of the whole matrix to 1e-50 -- at N <= 5 without identity rows, and at N = 9 and 12 with
    identity rows, held masks, an all-held frame and broken pairs, where the masks and the run logic matter."""
    for N, ident_rate in ((1, 0.0), (2, 0.0), (3, 0.0), (5, 0.0), (9, 0.25), (12, 0.2)):
        H, word, s, B, sigma = random_system(N, 40 + N, ident_rate=ident_rate)
        assert ident_rate == 0.0 or (((word & IDENTITY_ROW) != 0).any() and ((word & 0x7F) == 0x7F).any())
        truth_s, truth_v = sweeps_mp(H, word, s, B, sigma, W_LINEAR, as_float=False)
        dense_s, dense_v = dense_mp(H, word, s, B, sigma, W_LINEAR)
        assert max(abs(a - b) for a, b in zip(truth_s.ravel(), dense_s.ravel())) < 1e-50
        assert max(abs(a - b) for a, b in zip(truth_v.ravel(), dense_v.ravel())) < 1e-50


def scalar_system(h, s0=2.0, word=None):
    """Scalar blocks h_t on DOF 0 embedded in 7 x 7 identity blocks, couplings s0 on DOF 0 alone."""
    N = len(h)
    H = np.stack([np.diag([v, 1, 1, 1, 1, 1, 1.0]) for v in h])
    word = np.zeros(N, dtype=np.int32) if word is None else np.asarray(word, dtype=np.int32)
    s = np.array([s0, 0, 0, 0, 0, 0, 0.0])
    B = np.zeros((N, 7, 12))
    B[:, :, :7] = np.eye(7)
    return H, word, s, B, np.ones((N, 4))


def test_not_a_minimum_verdicts_of_the_linear_part(smooth_sens_harness):  # noqa: F811
    # scalar blocks 1, 5, 1 with couplings 2: both sweeps pass frame 1 and the combine fails there; all three are flagged
    H, word, s, B, sigma = scalar_system([1.0, 5.0, 1.0])
    assert not dense_linear(H, word, s, B, sigma)[2]
    sens, std, flags = smooth_sens_harness.linear(H, word, s, B, sigma, 2)
    assert (flags == NOT_PD).all() and np.isnan(std).all()
    for t in range(3):
        for d in range(5):
            assert np.isnan(sens[t, d]).all() if 0 <= t + d - 2 < 3 else not sens[t, d].view(np.uint64).any()
    fine = smooth_sens_harness.linear(*scalar_system([3.0, 5.0, 3.0]), 2)
    assert dense_linear(*scalar_system([3.0, 5.0, 3.0]))[2] and not fine[2].any() and np.isfinite(fine[0]).all()
    # a system that fails only in a later Schur step (Sf passes frames 0..2, fails at 3; Sb passes 5, 4, fails at 3): its
    # whole run is flagged, and nothing beyond the identity row that follows
    h = [3.0, 3.0, 3.0, 0.2, 3.0, 3.0, 1.0, 3.0, 3.0, 3.0]
    word = np.zeros(10, dtype=np.int32)
    word[6] = IDENTITY_ROW
    H, word, s, B, sigma = scalar_system(h, word=word)
    assert not dense_linear(H, word, s, B, sigma)[2]
    sens, std, flags = smooth_sens_harness.linear(H, word, s, B, sigma, 3)
    assert (flags[:6] == NOT_PD).all() and flags[6] == BAD_INPUT and not flags[7:].any()
    assert np.isnan(std[:7]).all() and np.isfinite(std[7:]).all() and np.isfinite(sens[7:]).all()
    assert np.isnan(sens[:6, 3]).all()
    tail = smooth_sens_harness.linear(H[7:], word[7:], s, B[7:], sigma[7:], 3)
    assert np.array_equal(sens[7:].view(np.uint64), tail[0].view(np.uint64)) and np.array_equal(std[7:].view(np.uint64), tail[1].view(np.uint64))
    # the same with the coupling cut by a held DOF instead of an identity row: the runs are the coupled runs
    word = np.zeros(10, dtype=np.int32)
    word[6] = 1                      # DOF 0, the only coupled one, is held in frame 6
    H, word, s, B, sigma = scalar_system(h, word=word)
    sens, std, flags = smooth_sens_harness.linear(H, word, s, B, sigma, 3)
    assert (flags[:6] == NOT_PD).all() and flags[6] == 1 and not flags[7:].any() and np.isfinite(std[6:]).all()
    # the free rows are NaN, held rows are +0.0 even in a poisoned frame
    word = np.zeros(3, dtype=np.int32)
    word[1] = 1 << 3
    H, word, s, B, sigma = scalar_system([1.0, 5.0, 1.0], word=word)
    sens, std, flags = smooth_sens_harness.linear(H, word, s, B, sigma, 1)
    assert (flags == NOT_PD | word).all() and not sens[1, :, 3].view(np.uint64).any() and std[1, 3] == 0 and np.isnan(std[1, [0, 1, 2, 4, 5, 6]]).all()


def test_bad_sigma_poisons_the_std_of_its_run_only(smooth_sens_harness):  # noqa: F811
    H, word, s, B, sigma = random_system(12, 7, ident_rate=0.0, held_rate=0.05, zero_s_rate=0.0)
    word[:] &= 0x7F
    word[8] = IDENTITY_ROW
    clean = smooth_sens_harness.linear(H, word, s, B, sigma, 2)
    sg = sigma.copy()
    sg[3, 2] = np.nan
    got = smooth_sens_harness.linear(H, word, s, B, sg, 2)
    # (the linear harness carries no bit 17 -- the verdict on sigma is assemble's --, but NaN in W_t must not leak past the run)
    assert np.array_equal(got[0].view(np.uint64), clean[0].view(np.uint64))
    assert np.array_equal(got[1][9:].view(np.uint64), clean[1][9:].view(np.uint64)) and np.isfinite(got[1][9:]).all()


@pytest.mark.parametrize("leg,lo,hi", [("RF", 272, 296), ("LF", 276, 308)])
def test_whole_rule_on_the_smoothed_windows_against_200_bits(smooth_sens_harness, smooth_harness, leg, lo, hi):  # noqa: F811
    q, pose, seg, bounds = smoothed_window(smooth_harness, leg, lo, hi)
    check_against_200_bits(smooth_sens_harness, f"{leg}_{lo}_{hi}", [(q, pose, seg, bounds, None)])


def test_whole_rule_on_made_up_trajectories_against_200_bits(smooth_sens_harness, smooth_harness):  # noqa: F811
    """40 made-up trajectories of 24 frames (targets out of reach, seeds on a limit), smoothed by the host-run 7o rule; in
    every fourth a bad frame, in every fifth a key point without weight."""
    cases = []
    for i, (ang, pose, seg, bounds) in enumerate(made_up_trajectories()):
        w = None
        pose = pose.copy()
        if i % 5 == 2:
            w = np.ones((len(ang), 4))
            w[:, i % 3] = 0.0              # (never the claw: without it the tarsus angle has no data in any frame, only
            pose[:, 1 + i % 3] = np.nan    # differences are penalised, and the Hessian is singular -- bit 8, rightly)
        if i % 4 == 1:
            pose[7 + i % 9, 0, 1] = np.nan
        q = smooth_harness.run_one(ang, pose, seg, bounds, smooth=0.1, weight=w)["angles"]
        cases.append((q, pose, seg, bounds, w))
    assert len(cases) == 40 and all(len(c[0]) == 24 for c in cases)
    check_against_200_bits(smooth_sens_harness, "made_up", cases)


def check_against_200_bits(ssh, name, cases, W=3, sigma=0.01):
    """Per trajectory: sens (all blocks within W) and the variance against the 200-bit values, the bar from the float64
    numpy restatement of the recursions on the same (200-bit, rounded) blocks.  Verdicts (held, positive definite) that are
    not robust at 200 bits make the trajectory's frames skipped; the cap is 2 % of all frames."""
    frames = skipped = 0
    worst = dict(sens=0.0, var=0.0, sens_numpy=0.0, var_numpy=0.0, grad=0.0)
    for q, pose, seg, bounds, w in cases:
        N = len(q)
        frames += N
        mp = mp_trajectory(q, pose, seg, bounds, 0.1, w, W, sigma)
        got = ssh.run_one(q, pose, seg, bounds, smooth=0.1, weight=w, kp_sigma=np.full((N, 4), sigma), half_width=W)
        bad = mp["bad"]
        assert np.array_equal(got["flags"] == BAD_INPUT, bad)
        if not mp["robust"]:
            print(f"{name}: a verdict is not robust at 200 bits, {N} frames skipped")
            skipped += N
            continue
        assert np.array_equal(got["flags"][~bad], mp["flags"][~bad]), (name, got["flags"], mp["flags"])
        good = ~bad & ((mp["flags"] & NOT_PD) == 0)
        # grad: a sum of about thirty products; its error against the magnitudes that were summed (grad_scale), not against
        # the sum, which cancels at a minimum
        e_g = rel(got["grad"][~bad], mp["grad"][~bad], mp["grad_scale"][~bad].max())
        assert e_g <= 100 * EPS, (name, e_g)
        worst["grad"] = max(worst["grad"], e_g)
        if not good.any():
            continue
        scale_s, scale_v = np.abs(mp["sens"][good]).max(), np.abs(mp["var"][good]).max()
        e_np_s, e_np_v = rel(mp["sens_numpy"][good], mp["sens"][good], scale_s), rel(mp["var_numpy"][good], mp["var"][good], scale_v)
        e_s = rel(got["sens"][good].reshape(good.sum(), 2 * W + 1, 7, 12), mp["sens"][good], scale_s)
        e_v = rel(got["std"][good] ** 2, mp["var"][good], scale_v)
        print(f"{name}: sens {e_s:.2e} (numpy {e_np_s:.2e}), var {e_v:.2e} (numpy {e_np_v:.2e})")
        assert e_s <= max(100 * e_np_s, 100 * EPS), (name, e_s, e_np_s)
        assert e_v <= max(100 * e_np_v, 100 * EPS), (name, e_v, e_np_v)
        for k, v in (("sens", e_s), ("var", e_v), ("sens_numpy", e_np_s), ("var_numpy", e_np_v)):
            worst[k] = max(worst[k], v)
    assert skipped <= 0.02 * frames, (name, skipped, frames)
    record(f"whole_rule_{name}", dict(trajectories=len(cases), frames=frames, skipped_frames=skipped, half_width=W, worst=worst))


def test_rule_against_central_differences_of_the_host_solver(smooth_sens_harness, smooth_harness, refine_sens_harness):  # noqa: F811
    """RF 272:296 at smooth 0.1, polished until the reported grad stops falling.  Each of the 12 coordinates of frame 12 is
    moved by +-h and +-2h (h = 1e-5), the float64 host solver of seqik_smooth.h runs again from the polished angles, and the
    change of ALL 24 frames is compared with sens at half_width 16.  Bar (7p's convention): 10 x the distance between the
    two difference estimates.  seqik_refine_sensitivity at the same angles must be farther from the differences."""
    ang, pose, seg, bounds = shipped_window("RF", 272, 296)
    q, grad_reached, rounds = fd_polish(smooth_harness, smooth_sens_harness, ang, pose, seg, bounds)
    N, T, W, h = len(q), 12, 16, 1e-5
    got = smooth_sens_harness.run_one(q, pose, seg, bounds, smooth=0.1, half_width=W)
    assert not (got["flags"] & ~0x7F).any()
    free = (got["flags"][:, None] >> np.arange(7)) & 1 == 0
    solve = lambda p: smooth_harness.run_one(q, p, seg, bounds, smooth=0.1, max_iter=1000, gtol=0.0, ftol=0.0)["angles"]  # noqa: E731
    est = np.zeros((2, N, 7, 4, 3))
    for k in range(4):
        for c in range(3):
            for i, step in enumerate((h, 2 * h)):
                pp, pm = pose.copy(), pose.copy()
                pp[T, k + 1, c] += step
                pm[T, k + 1, c] -= step
                est[i, :, :, k, c] = (solve(pp) - solve(pm)) / (2 * step)
    fd, spread = est[0], np.abs(est[0] - est[1]).max()
    # the rule's statement about frame t and the key points of frame T: block d = T - t + W
    rule = np.stack([got["sens"][t, T - t + W] for t in range(N)])
    mask = np.broadcast_to(free[:, :, None, None], rule.shape)
    err = np.abs(rule - fd)[mask].max()
    per_frame = refine_sens_harness.run(q, pose, seg, bounds)["sens"]
    alone = np.zeros_like(rule)
    alone[T] = per_frame[T]
    ok = np.isfinite(alone)
    err_alone = np.abs(alone - fd)[mask & ok].max()
    decay = [float(np.abs(got["sens"][T, W + d]).max()) for d in range(-11, 12)]
    print(f"grad reached {grad_reached:.3e} after {rounds} polishing calls; |rule - fd| {err:.3e}, |fd(h) - fd(2h)| {spread:.3e}, "
          f"|refine_sensitivity - fd| {err_alone:.3e}; max |fd| {np.abs(fd).max():.3e}")
    print("block norm (max |entry|) of frame 12 by offset -11..11:", " ".join(f"{v:.2e}" for v in decay))
    record("central_differences", dict(window="RF 272:296", frame=T, h=[h, 2 * h], grad_reached=grad_reached,
                                       polishing_calls=rounds, rule_minus_fd=float(err), fd_spread=float(spread),
                                       refine_sensitivity_minus_fd=float(err_alone), ratio=float(err_alone / err),
                                       max_abs_fd=float(np.abs(fd).max()), block_max_abs_by_offset=dict(zip(map(str, range(-11, 12)), decay))))
    assert err <= 10 * spread, (err, spread)
    assert err_alone > err, (err_alone, err)
