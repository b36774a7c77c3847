"""The generic chain's ANSWERS, judged where "right" does not depend on the restatement (tests/test_generic.py pins the
kernel code to the C oracle on one smooth recording; kernel and oracle are two copies of one restatement).  The angles are
not reproducible, the objective is: the distance d from the claw to its target.  On made-up legs (tests/generic_cases.py:
random segments and limits, open and narrow limits, targets out of reach / on the origin, repeated frames):

  1. not worse than real scipy (oracle/scipy_oracle.py::generic_leg_arrays, the way IKPy calls it): d_kernel <= d_scipy +
     MARGIN * reach except where the two sit in different minima -- which may happen no more often than it happens to
     scipy against itself under a 1-ulp change of its key points;
  2. locally optimal: what real scipy still gains when it continues from the answer with tolerances 1e-15 (the polish gain)
     is no more than 4 x what it gains from scipy's own answer;
  3. feasible and self-consistent: lb <= x <= ub by plain comparison, fk[:, 8] - fk[:, 0] is the claw of the returned angles
     (mpmath, 200 bits), fk[:, 0] is pose[:, 0] by bits, status in 0..4, 1 <= nfev <= max_nfev.

All three on the CPU with the host build of the kernel code; the GPU tier (below) then needs bit equality with the oracle
only, on the inputs where the eight lanes of a group disagree in pass count, step rejection and termination.  Measured
values, histograms and seeds: EXPERIMENTS.md "Generic chain: answers against real scipy"."""
import warnings

import numpy as np
import pytest

import generic_cases as gc

KEYS = ("angles", "fk", "status", "nfev")
MAX_NFEV = 900                 # GenericConst::max_nfev = scipy's default 100 * n for the 9 links IKPy passes
# Statement 1.  4 x the largest |d_scipy(pose) - d_scipy(nextafter(pose))| / reach over the frames of all families on which
# the two scipy runs end in the same minimum (claws within 1e-3 reach): scipy's own spread in the objective when it stops
# on ftol = 1e-8.  Measured 1.925e-4 (family open_limits; 8.96e-6 unreachable, 3.88e-6 made_up, 1.38e-6 repeat, 5.8e-8 narrow).
SAME_MINIMUM = 1e-3
SCIPY_SPREAD = 1.925e-4
MARGIN = 4 * SCIPY_SPREAD
WORSE_SHARE, WORSE_BY, WORSE_OVERALL = 0.03, 0.5, 2      # the caps (conditions: scipy's 1-ulp twin must meet them too)
# Statement 3.  Largest |(fk[:, 8] - fk[:, 0]) - claw_mp| / ulp(reach) measured over all families: 1.67 (family repeat; the
# origin is added to a left-to-right product of seven links, both roundings count).
FK_ULPS_MEASURED = 1.67
FK_ULPS = 4 * FK_ULPS_MEASURED
POLISH_STRIDE = 4              # statement 2 on every 4th frame of every family: 110 frames
POLISH_FACTOR = 4.0
STATUS0_CASE = ("folded", 0, 1)   # (family, leg, frame): real scipy spends its evaluation budget there (status 0)


def _solve_family(name, oracle, host_harness):
    from oracle import scipy_oracle as so
    out = []
    for pose, seg, bounds, seeds in gc.family(name):
        twin_pose = np.nextafter(pose, np.inf)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            scipy_ans = so.generic_leg_arrays(pose, seg, bounds, seeds)
            twin_ans = so.generic_leg_arrays(twin_pose, seg, bounds, seeds)
        r = gc.reach(seg)
        out.append(dict(pose=pose, seg=seg, bounds=bounds, seeds=seeds, reach=r,
                        kernel=host_harness.run_generic(pose, seg, bounds, seeds),
                        oracle=oracle.generic_leg(pose, seg, bounds, seeds[18:27]), scipy=scipy_ans, twin=twin_ans,
                        d_kernel=None, d_scipy=gc.claw_distance(scipy_ans["angles"], seg, pose) / r,
                        d_twin=gc.claw_distance(twin_ans["angles"], seg, twin_pose) / r,
                        same_minimum=np.array([np.linalg.norm(gc.claw(a, seg) - gc.claw(b, seg)) / r < SAME_MINIMUM
                                               for a, b in zip(scipy_ans["angles"], twin_ans["angles"])])))
        out[-1]["d_kernel"] = gc.claw_distance(out[-1]["kernel"]["angles"], seg, pose) / r
    return out


@pytest.fixture(scope="module")
def answers(oracle, host_harness):
    """family -> per leg: the case, the answers of kernel code, oracle, real scipy and scipy on the 1-ulp twin of the key
    points, and their claw distances in units of the leg's reach.  Computed once."""
    return {name: _solve_family(name, oracle, host_harness) for name in gc.FAMILIES}


def _cat(legs, key):
    return np.concatenate([l[key] for l in legs])


# ---- the yardsticks (functions, so that the teeth test can hand them wrong answers) ----------------------------------------
def statement1(d_a, d_b):
    """a against b, claw distances in units of reach: (frames on which a is the worse one, by how much at most)."""
    excess = np.asarray(d_a) - np.asarray(d_b)
    return int((excess > MARGIN).sum()), float(excess.max())


def statement1_holds(d_a, d_b):
    n_worse, by = statement1(d_a, d_b)
    return n_worse <= WORSE_SHARE * len(d_a) and by <= WORSE_BY


def statement2_holds(gain_a, gain_scipy):
    return (np.max(gain_a) <= POLISH_FACTOR * np.max(gain_scipy) and
            np.quantile(gain_a, 0.95) <= POLISH_FACTOR * np.quantile(gain_scipy, 0.95))


def fk_ulps(pose, seg, ans):
    """(N,) largest |(fk[t, 8] - fk[t, 0]) - claw_mp(angles[t])| over the three axes in units of ulp(reach)."""
    import mpmath
    ulp = float(np.spacing(gc.reach(seg)))
    out = np.empty(len(pose))
    with mpmath.workdps(61):
        for t in range(len(pose)):
            want = gc.claw_mp(ans["angles"][t], seg)
            out[t] = max(float(abs(mpmath.mpf(float(ans["fk"][t, 8, a])) - mpmath.mpf(float(ans["fk"][t, 0, a])) - want[a]))
                         for a in range(3)) / ulp
    return out


def statement3_violations(pose, seg, bounds, ans):
    bad = []
    x = ans["angles"]
    if not ((x >= bounds[:, 0]).all() and (x <= bounds[:, 1]).all()):
        bad.append("an angle outside its limits")
    if not np.array_equal(ans["fk"][:, 0], pose[:, 0]):
        bad.append("fk[:, 0] is not pose[:, 0]")
    worst = fk_ulps(pose, seg, ans).max()
    if not worst <= FK_ULPS:
        bad.append(f"fk[:, 8] - fk[:, 0] is {worst:.1f} ulp(reach) from the claw of the angles")
    if not np.isin(ans["status"], (0, 1, 2, 3, 4)).all():
        bad.append("status outside 0..4")
    if not ((ans["nfev"] >= 1).all() and (ans["nfev"] <= MAX_NFEV).all()):
        bad.append("nfev outside 1..max_nfev")
    return bad


def _polish_gain(angles, leg, t):
    _, before, after = gc.polish(angles, leg["seg"], leg["bounds"], leg["pose"][t, 4] - leg["pose"][t, 0])
    return (before - after) / leg["reach"]


@pytest.fixture(scope="module")
def polish_gains(answers):
    """(leg, frame, gain of the kernel code's answer, gain of scipy's answer) on every POLISH_STRIDE-th frame of every family."""
    rows = []
    for legs in answers.values():
        k = 0
        for leg in legs:
            for t in range(len(leg["pose"])):
                if k % POLISH_STRIDE == 0:
                    rows.append((leg, t, _polish_gain(leg["kernel"]["angles"][t], leg, t),
                                 _polish_gain(leg["scipy"]["angles"][t], leg, t)))
                k += 1
    return rows


# ---- CPU tier -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gc.FAMILIES))
def test_kernel_code_equals_oracle_on_made_up_legs(answers, name):
    for i, leg in enumerate(answers[name]):
        for k in KEYS:
            assert np.array_equal(leg["kernel"][k], leg["oracle"][k]), (name, i, k)


@pytest.mark.parametrize("name", list(gc.FAMILIES))
def test_answers_are_feasible_and_self_consistent(answers, name):
    """Statement 3 on every frame."""
    worst = 0.0
    for i, leg in enumerate(answers[name]):
        worst = max(worst, fk_ulps(leg["pose"], leg["seg"], leg["kernel"]).max())
        assert statement3_violations(leg["pose"], leg["seg"], leg["bounds"], leg["kernel"]) == [], (name, i)
    print(f"{name}: fk[:, 8] - fk[:, 0] against the claw at 200 bits: {worst:.2f} ulp(reach)")


def test_margin_is_scipys_own_spread(answers):
    """MARGIN is 4 x the spread of scipy's objective between a run and its 1-ulp twin where both end in the same minimum."""
    spread = 0.0
    for name, legs in answers.items():
        same = _cat(legs, "same_minimum")
        s = np.abs(_cat(legs, "d_scipy") - _cat(legs, "d_twin"))[same].max()
        print(f"{name}: scipy against its 1-ulp twin, same minimum on {same.mean():.0%} of the frames, spread {s:.3g} reach")
        spread = max(spread, s)
    assert spread <= SCIPY_SPREAD * 1.0001 and spread >= SCIPY_SPREAD / 1.5, spread


@pytest.mark.parametrize("name", list(gc.FAMILIES))
def test_not_worse_than_real_scipy(answers, name):
    """Statement 1.  The caps are conditions on the seeds: scipy's 1-ulp twin meets them on this family (asserted first), so
    they cannot hide the kernel."""
    legs = answers[name]
    d_k, d_s, d_t = _cat(legs, "d_kernel"), _cat(legs, "d_scipy"), _cat(legs, "d_twin")
    print(f"{name}: {len(d_k)} frames; worse than scipy (frames, by at most): kernel code {statement1(d_k, d_s)}, "
          f"scipy's twin {statement1(d_t, d_s)}; scipy worse than: kernel code {statement1(d_s, d_k)}, twin {statement1(d_s, d_t)}; "
          f"status kernel code {np.bincount(_cat([l['kernel'] for l in legs], 'status'), minlength=5)} "
          f"scipy {np.bincount(_cat([l['scipy'] for l in legs], 'status'), minlength=5)}")
    assert statement1_holds(d_t, d_s) and statement1_holds(d_s, d_t), "the seeds of this family do not meet the condition"
    assert statement1_holds(d_k, d_s), statement1(d_k, d_s)


def test_worse_than_scipy_no_more_often_than_scipy_is_worse(answers):
    legs = [l for fam in answers.values() for l in fam]
    d_k, d_s = _cat(legs, "d_kernel"), _cat(legs, "d_scipy")
    kernel_worse, scipy_worse = statement1(d_k, d_s)[0], statement1(d_s, d_k)[0]
    print(f"all families, {len(d_k)} frames: kernel code worse on {kernel_worse}, scipy worse on {scipy_worse}")
    assert kernel_worse <= scipy_worse + WORSE_OVERALL


def test_answers_are_locally_optimal(polish_gains):
    """Statement 2."""
    g_k, g_s = np.array([r[2] for r in polish_gains]), np.array([r[3] for r in polish_gains])
    print(f"polish gain / reach on {len(g_k)} frames: kernel code median {np.median(g_k):.3g} 95 % {np.quantile(g_k, 0.95):.3g} "
          f"max {g_k.max():.3g}; scipy median {np.median(g_s):.3g} 95 % {np.quantile(g_s, 0.95):.3g} max {g_s.max():.3g}")
    assert g_k.max() <= POLISH_FACTOR * g_s.max()
    assert np.quantile(g_k, 0.95) <= POLISH_FACTOR * np.quantile(g_s, 0.95)


def test_the_spent_evaluation_budget(answers):
    """status == 0: IKPy returns such an answer silently.  On a frame where REAL scipy spends its 900 evaluations (a target on
    the ThC origin that the leg cannot fold onto) the kernel code spends them too, stays inside the limits and is not
    worse than scipy."""
    name, i, t = STATUS0_CASE
    leg = answers[name][i]
    assert leg["scipy"]["status"][t] == 0 and leg["scipy"]["nfev"][t] == MAX_NFEV
    assert leg["kernel"]["nfev"][t] == MAX_NFEV and leg["kernel"]["status"][t] == 0
    x = leg["kernel"]["angles"][t]
    assert (x >= leg["bounds"][:, 0]).all() and (x <= leg["bounds"][:, 1]).all()
    assert leg["d_kernel"][t] <= leg["d_scipy"][t] + MARGIN, (leg["d_kernel"][t], leg["d_scipy"][t])


def test_the_yardsticks_reject_wrong_answers(answers, polish_gains):
    """Teeth: each yardstick passes the real answers (the tests above) and fails a planted defect."""
    # statement 2: every answer moved by 1e-3 rad along the direction the claw is most sensitive to (the first right
    # singular vector of its Jacobian: as far from the null space as a direction gets), kept inside the limits
    moved = []
    for leg, t, _, _ in polish_gains:
        x = leg["kernel"]["angles"][t]
        v = np.linalg.svd(gc.claw_jacobian(x, leg["seg"]))[2][0]
        lb, ub = leg["bounds"][:, 0], leg["bounds"][:, 1]
        cand = [np.clip(x + s * 1e-3 * v, lb, ub) for s in (1.0, -1.0)]
        moved.append(_polish_gain(max(cand, key=lambda c: np.abs(c - x).sum()), leg, t))
    g_s = np.array([r[3] for r in polish_gains])
    assert statement2_holds(np.array([r[2] for r in polish_gains]), g_s)
    assert not statement2_holds(np.array(moved), g_s), (np.max(moved), np.quantile(moved, 0.95))
    # statement 1: the answer of frame t reported for frame t + 1
    legs = answers["made_up"]
    d_s = _cat(legs, "d_scipy")
    late = np.concatenate([gc.claw_distance(np.roll(l["kernel"]["angles"], 1, axis=0), l["seg"], l["pose"]) / l["reach"] for l in legs])
    assert statement1_holds(_cat(legs, "d_kernel"), d_s)
    assert not statement1_holds(late, d_s), statement1(late, d_s)
    # statement 3: one angle one ulp past a limit
    leg = answers["narrow"][0]
    ans = {k: leg["kernel"][k].copy() for k in KEYS}
    assert statement3_violations(leg["pose"], leg["seg"], leg["bounds"], ans) == []
    ans["angles"][3, 5] = np.nextafter(leg["bounds"][5, 1], np.inf)
    assert "an angle outside its limits" in statement3_violations(leg["pose"], leg["seg"], leg["bounds"], ans)
    ans["angles"][3, 5] = np.nextafter(leg["bounds"][5, 0], -np.inf)
    assert "an angle outside its limits" in statement3_violations(leg["pose"], leg["seg"], leg["bounds"], ans)


def _pre_transformed(pose, affine):
    fixed, scale, template = affine
    out = np.empty_like(pose)
    out[..., :, :] = template                       # row 0 is all the generic chain reads besides the claw
    out[..., 4, :] = (pose[..., 4, :] - fixed) * scale + template
    return out


# ---- GPU tier: bit equality with the oracle on made-up legs ---------------------------------------------------------------
@pytest.fixture(scope="module")
def made_up_batch(oracle):
    """8 made-up legs and, lazily, the oracle's answer of any (leg, key points[, warm start]) -- computed once per module."""
    from concurrent.futures import ThreadPoolExecutor
    from conftest import random_leg_case
    rng = np.random.default_rng(2024)
    legs = [gc.generic_case(rng, 8) for _ in range(8)]
    extra = np.stack([np.stack([random_leg_case(rng, 8)[0] for _ in range(8)]) for _ in range(129)])   # other legs' key points
    cache = {}

    class Batch:
        pass
    b = Batch()
    b.legs = legs

    def pose(S, n_legs=8, n_frames=8):
        """(S, n_legs, n_frames, 5, 3): the leg's own nasty key points first, then those of other made-up legs."""
        own = np.stack([l[0] for l in legs])[None]
        return np.ascontiguousarray(np.concatenate([own, extra[:S - 1]])[:S, :n_legs, :n_frames])
    b.pose = pose

    def reference(pose, init=None):
        S, L = pose.shape[:2]

        def one(idx):
            s, li = divmod(idx, L)
            key = (pose[s, li].tobytes(), li, None if init is None else init[s, li].tobytes())
            if key not in cache:
                _, seg, bounds, seeds = legs[li]
                if init is None:
                    cache[key] = oracle.generic_leg(pose[s, li], seg, bounds, seeds[18:27])
                else:   # the oracle's seed vector is positional (link order): the warm start replaces links 1..7
                    seed9 = seeds[18:27].copy()
                    seed9[1:8] = init[s, li][gc.GENERIC_LINK_DOF]
                    cache[key] = oracle.generic_leg(pose[s, li], seg, bounds, seed9)
            return cache[key]
        with ThreadPoolExecutor(8) as ex:
            refs = list(ex.map(one, range(S * L)))
        return {k: np.stack([r[k] for r in refs]).reshape((S, L) + refs[0][k].shape) for k in KEYS}
    b.reference = reference
    return b


def _params(hiplib, batch, n_legs=8):
    return [hiplib.leg_params_from_arrays(*l[1:]) for l in batch.legs[:n_legs]]


def _assert_equal(got, want, what, keys=KEYS):
    for k in keys:
        assert np.array_equal(got[k], want[k]), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("S, n_legs", [(1, 8), (2, 8), (7, 8), (8, 8), (1, 1), (1, 7), (3, 3)])
def test_lane_groups_on_made_up_legs(hiplib, made_up_batch, S, n_legs):
    """run_generic<.., GROUPED>: 8, 16, 56, 64 chains and 1, 7, 9 (one below and one above a group of eight) on thin waves of
    1, 5 and 8 chains -- the eight lanes of a group carry one chain whose passes they split; the made-up legs are where
    neighbouring chains differ in pass count, step rejection and termination.  == the one-lane code == the oracle."""
    pose = made_up_batch.pose(S, n_legs)
    params = _params(hiplib, made_up_batch, n_legs)
    ref = made_up_batch.reference(pose)
    for lanes in (1, 5, 8):
        grouped = hiplib.solve_generic(pose, params, want_diag=True, lanes_per_wave=lanes)
        one_lane = hiplib.solve_generic(pose, params, want_diag=True, lanes_per_wave=lanes, lane_groups=False)
        plain = hiplib.solve_generic(pose, params, want_diag=False, lanes_per_wave=lanes)
        _assert_equal(grouped, ref, ("grouped", lanes))
        _assert_equal(one_lane, ref, ("one lane", lanes))
        _assert_equal(plain, ref, ("grouped, no diagnostics", lanes), keys=("angles", "fk"))


@pytest.fixture(scope="module")
def big_batch(made_up_batch):
    """8 legs x 130 sequences x 6 frames: 1040 chains = 16 full wavefronts and a ragged one; per-chain warm starts."""
    pose = made_up_batch.pose(130, 8, 6)
    rng = np.random.default_rng(77)
    lb = np.stack([l[2][:, 0] for l in made_up_batch.legs])
    ub = np.stack([l[2][:, 1] for l in made_up_batch.legs])
    init = lb + rng.random((130, 8, 7)) * (ub - lb)
    init[::5] = lb                                  # some warm starts exactly on the limits
    return pose, made_up_batch.reference(pose), init, made_up_batch.reference(pose, init)


@pytest.mark.gpu
@pytest.mark.parametrize("chain_queue", [1, 2])
def test_one_lane_per_chain_and_the_queue_on_made_up_legs(hiplib, made_up_batch, big_batch, chain_queue):
    """The static launch (chain_queue = 1) and the forced chain queue (2) on 1040 made-up chains, every chain against the
    oracle; with warm starts per chain, with workgroups of 64 and 256, without diagnostics, and with one frame."""
    pose, ref, init, ref_init = big_batch
    params = _params(hiplib, made_up_batch)
    for block in (64, 256):
        got = hiplib.solve_generic(pose, params, want_diag=True, chain_queue=chain_queue, block_size=block)
        _assert_equal(got, ref, ("block", block))
    got = hiplib.solve_generic(pose, params, want_diag=True, chain_queue=chain_queue, init_angles=init)
    _assert_equal(got, ref_init, "warm starts")
    got = hiplib.solve_generic(pose, params, want_diag=False, chain_queue=chain_queue)
    _assert_equal(got, ref, "no diagnostics", keys=("angles", "fk"))
    one = np.ascontiguousarray(pose[:, :, :1])
    got = hiplib.solve_generic(one, params, want_diag=True, chain_queue=chain_queue)
    _assert_equal(got, {k: v[:, :, :1] for k, v in ref.items()}, "one frame")


@pytest.mark.gpu
def test_affine_equals_pre_transformed_key_points_on_made_up_legs(hiplib, made_up_batch):
    """`affine` through solve_generic == the same call on key points transformed beforehand, bit for bit, on lane groups and
    on one lane per chain.  The host rule (seqik_generic.hpp, new_solve): target = ((kp - fixed_coxa) * scale + template_coxa)
    - template_coxa and the stored origin is template_coxa; on transformed key points (row 4 the aligned claw, row 0
    template_coxa) the kernel forms row 4 - row 0 from the same two numbers, and the library is built without contraction,
    so numpy's transform gives the same bits.  (test_gpu_fk_fused_alignment_origin_is_template_coxa covers only that FK of
    the returned angles reproduces the stored fk.)"""
    rng = np.random.default_rng(5)
    aff = [(rng.normal(size=3), float(rng.uniform(0.5, 2.0)), rng.normal(size=3)) for _ in range(8)]
    params = _params(hiplib, made_up_batch)
    for S in (2, 130):
        raw = made_up_batch.pose(S, 8, 6)
        # raw key points whose aligned claw is the made-up target: claw_raw = (target - template) / scale + fixed, roughly
        for li, (fixed, scale, template) in enumerate(aff):
            raw[:, li, :, 4] = (raw[:, li, :, 4] - raw[:, li, :, 0]) / scale + fixed
        pre = np.stack([_pre_transformed(raw[:, li], aff[li]) for li in range(8)], axis=1)
        fused = hiplib.solve_generic(raw, params, want_diag=True, affine=[hiplib.make_affine(*a) for a in aff])
        plain = hiplib.solve_generic(pre, params, want_diag=True)
        _assert_equal(fused, plain, S)
        _assert_equal(plain, made_up_batch.reference(pre), ("oracle", S))


def _device_call(hiplib, pose, params, layout=None, guard=3, chain_queue=0, lanes_per_wave=0):
    """seqik_solve_generic_device on torch buffers with `guard` sentinel rows in front of and behind every output."""
    import ctypes
    import torch
    S, L, N = pose.shape[:3]
    lib = hiplib.load()
    arr = (hiplib.SeqikLegParams * L)(*params)
    d_pose = torch.from_numpy(np.ascontiguousarray(pose.transpose(0, 1, 3, 2, 4)) if layout else pose).cuda()
    shapes = dict(angles=((S * L * N, 7), torch.float64, 12345.0), fk=((S * L * N, 27), torch.float64, 12345.0),
                  status=((S * L * N, 1), torch.int32, -77), nfev=((S * L * N, 1), torch.int32, -77))
    buf = {k: torch.full((shape[0] + 2 * guard, shape[1]), fill, dtype=dt, device="cuda") for k, (shape, dt, fill) in shapes.items()}
    ptr = {k: buf[k][guard:].data_ptr() for k in buf}
    opt = hiplib.SeqikOptions()
    opt.reserved[0], opt.reserved[1] = lanes_per_wave, chain_queue
    rc = lib.seqik_solve_generic_device(d_pose.data_ptr(), S, L, N, arr, ptr["angles"], ptr["fk"], ptr["status"], ptr["nfev"],
                                        None, ctypes.byref(layout) if layout else None, None, ctypes.byref(opt), None)
    assert rc == 0
    torch.cuda.synchronize()
    hiplib.check_faults()
    out = {}
    for k, (shape, dt, fill) in shapes.items():
        host = buf[k].cpu().numpy()
        assert (host[:guard] == fill).all() and (host[-guard:] == fill).all(), ("guard rows", k)
        out[k] = host[guard:-guard]
    ang = out["angles"].reshape(S, L, 7, N).transpose(0, 1, 3, 2) if layout else out["angles"].reshape(S, L, N, 7)
    return dict(angles=ang, fk=out["fk"].reshape(S, L, N, 9, 3), status=out["status"].reshape(S, L, N), nfev=out["nfev"].reshape(S, L, N))


@pytest.mark.gpu
def test_planar_layout_and_guard_rows_on_made_up_legs(hiplib, made_up_batch, big_batch):
    """The device entry point writes its outputs and nothing else (sentinel rows around every output buffer of one launch
    per path: lane groups, one lane per chain, chain queue), and the planar SeqikLayout (pose [chain][5][frame][3], angles
    [chain][7][frame]; this path takes the strides as they are) gives the dense call's bits on an 8-leg batch."""
    params = _params(hiplib, made_up_batch)
    small = made_up_batch.pose(1)
    ref = made_up_batch.reference(small)
    _assert_equal(_device_call(hiplib, small, params), ref, "lane groups, dense")
    _assert_equal(_device_call(hiplib, small, params, layout=hiplib.planar_layout(small.shape[2])), ref, "lane groups, planar")
    pose, big_ref = big_batch[0], big_batch[1]
    _assert_equal(_device_call(hiplib, pose, params, chain_queue=1), big_ref, "one lane per chain")
    _assert_equal(_device_call(hiplib, pose, params, chain_queue=2), big_ref, "chain queue")
    _assert_equal(_device_call(hiplib, pose, params, chain_queue=2, layout=hiplib.planar_layout(pose.shape[2])), big_ref,
                  "chain queue, planar")
