"""Forward kinematics from joint angles (include/seqik_fk.h, csrc/seqik_fk.hpp / seqik_fk.hip).

CPU tier: the header and exports, the device function run on the host against the solvers' own FK rows and the oracle
(bit for bit), the reference's shipped FK, argument errors through the C ABI.  GPU tier (`-m gpu`): the kernel against
the solvers' FK (bit for bit), the device entry point, size-independent invariants, the distances, NaN / empty inputs
and the LegInvKin* methods."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

from angle_map_support import (_generic_params, _params, _stack, SENTINEL, gpu_lib, guarded, made_up_batch, same_bits,
                               switches, unguarded)
from conftest import DOFS, ROOT, LegParamsC, leg_arrays, load_golden
from harness_build import build_harness

FK_SYMBOLS = ["seqik_forward_kinematics", "seqik_forward_kinematics_device"]


def _lp(seg, bounds=None, seeds=None):
    lp = LegParamsC()
    for i in range(4):
        lp.seg[i] = float(seg[i])
    if bounds is not None:
        for i in range(7):
            lp.bounds[i][0], lp.bounds[i][1] = float(bounds[i][0]), float(bounds[i][1])
    if seeds is not None:
        for i in range(27):
            lp.seeds[i] = float(seeds[i])
    return lp


class FkHarness:
    def __init__(self, so):
        self.lib = ctypes.CDLL(so)
        dp = ctypes.POINTER(ctypes.c_double)
        self.lib.harness_fk.restype = ctypes.c_int
        self.lib.harness_fk.argtypes = [dp, ctypes.c_int64, ctypes.POINTER(LegParamsC), ctypes.c_int32, dp,
                                        ctypes.c_int64, dp, dp]
        self.lib.harness_leg_map_plan.restype = None
        self.lib.harness_leg_map_plan.argtypes = [ctypes.c_char_p, ctypes.c_int64] + [ctypes.c_int32] * 4 + [
            ctypes.POINTER(ctypes.c_int64)]

    def plan(self, prefix, n_total, unit, **env):
        """plan_leg_map under the switches `env` (without the prefix) -> (staged, block, workgroups, LDS bytes)."""
        out = (ctypes.c_int64 * 4)()
        with switches(**{f"{prefix}_{k}": str(v) for k, v in env.items()}):
            self.lib.harness_leg_map_plan(prefix.encode(), n_total, *unit, out)
        return tuple(out)

    def fk(self, angles, seg, kind, pose=None, origin=None, want_dist=False):
        dp = ctypes.POINTER(ctypes.c_double)
        angles = np.ascontiguousarray(angles, dtype=np.float64)
        n = angles.shape[0]
        src, stride = None, 0
        if pose is not None:
            src, stride = np.ascontiguousarray(pose, dtype=np.float64), 15
        elif origin is not None:
            src, stride = np.ascontiguousarray(np.broadcast_to(origin, (n, 3)), dtype=np.float64), 3
        fk = np.full((n, 9, 3), np.nan)
        dist = np.full((n, 4), np.nan) if want_dist else None
        lp = _lp(seg)
        rc = self.lib.harness_fk(angles.ctypes.data_as(dp), n, ctypes.byref(lp), kind,
                                 src.ctypes.data_as(dp) if src is not None else None, stride, fk.ctypes.data_as(dp),
                                 dist.ctypes.data_as(dp) if dist is not None else None)
        assert rc == 0
        return fk, dist


@pytest.fixture(scope="module")
def fk_harness():
    return FkHarness(build_harness(os.path.join(ROOT, "tests", "harness", "fk_harness.hip")))


# ---------------------------------------------------------------------------------------------------------------------
# CPU tier
# ---------------------------------------------------------------------------------------------------------------------

def test_fk_header_declares_exactly_the_new_entry_points(hiplib):
    text = open(os.path.join(ROOT, "include", "seqik_fk.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(seqik_[a-z_]+)\s*\(", text)))
    assert declared == sorted(FK_SYMBOLS)
    assert sorted(hiplib.FK_EXPORTED_SYMBOLS) == declared
    assert not set(declared) & set(hiplib.EXPORTED_SYMBOLS)
    lib = hiplib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.seqik_abi_version() == 7 == hiplib.ABI_VERSION
    assert "seqik_fk.hip" in hiplib.COMPILE_UNITS
    assert {"seqik_fk.hip", "seqik_fk.hpp"} <= set(hiplib.SOURCES)


@pytest.mark.parametrize("name", ["df3d_100", "df3d_1000"])
def test_host_fk_equals_solver_fk_and_oracle_bit_for_bit(host_harness, fk_harness, oracle, name):
    """fk_leg_frame<seq> on the angles the solver's device code (run on the host) returned == the FK rows it wrote
    while solving, for all six legs; and == the oracle's FK."""
    z = load_golden(name)
    for leg in [str(l) for l in z["legs"]]:
        pose, seg, b, seeds = leg_arrays(z, leg)
        solved = host_harness.run(pose, seg, b, seeds, diag=False)
        fk, _ = fk_harness.fk(solved["angles"], seg, 0, pose=pose)
        assert np.array_equal(fk, solved["fk"]), leg
        ref = oracle.seq_leg(pose, seg, b, seeds)
        assert np.array_equal(fk_harness.fk(ref["angles"], seg, 0, pose=pose)[0], ref["fk"]), leg


def test_host_fk_generic_equals_generic_solver_bit_for_bit(host_harness, fk_harness):
    z = load_golden("generic_rf_100")
    for leg in [str(l) for l in z["legs"]]:
        pose, seg, b, seeds = leg_arrays(z, leg)
        solved = host_harness.run_generic(pose, seg, b, seeds)
        fk, _ = fk_harness.fk(solved["angles"], seg, 1, pose=pose)
        assert np.array_equal(fk, solved["fk"]), leg
        # the thorax-coxa order matters: the same angles under the sequential chain are another leg posture
        assert not np.allclose(fk_harness.fk(solved["angles"], seg, 0, pose=pose)[0], fk)


def test_host_fk_of_reference_shipped_angles_matches_its_shipped_fk(fk_harness):
    """Reference-held pin: the reference's own angles of the 6000-frame anipose recording, through the sequential chain
    with the fixture's segment lengths and key point 0 as origin, against the FK the reference shipped (at fk_frames).
    Measured maximum: 2.4e-15 on both legs, with positions up to 2.07; the bar is 1e-12."""
    z = load_golden("anipose_shipped")
    cut = z["fk_frames"]
    for leg in ("RF", "LF"):
        fk, _ = fk_harness.fk(z[f"{leg}_angles"], z[f"{leg}_seg"], 0, origin=z[f"{leg}_pose"][:, 0])
        err = np.abs(fk[cut] - z[f"{leg}_fk_cut"]).max()
        assert err <= 1e-12, (leg, err)


def test_host_fk_nan_angle_and_leg_local_origin(fk_harness):
    z = load_golden("df3d_100")
    ang, seg, pose = z["RF_angles"].copy(), z["RF_seg"], z["RF_pose"]
    ang[7, 6] = np.nan
    fk, dist = fk_harness.fk(ang, seg, 0, pose=pose, want_dist=True)
    assert np.isnan(fk[7]).all() and np.isnan(dist[7]).all()
    ok = np.ones(len(ang), bool)
    ok[7] = False
    assert np.isfinite(fk[ok]).all() and np.isfinite(dist[ok]).all()
    local, _ = fk_harness.fk(z["RF_angles"], seg, 0)
    assert (local[:, :4] == 0.0).all()
    assert np.abs(local + pose[:, :1] - fk_harness.fk(z["RF_angles"], seg, 0, pose=pose)[0])[ok].max() < 1e-15


# what each unit hands to plan_leg_map: staging allowed, largest block per lane and staged, doubles of LDS per wavefront
PLAN_UNITS = {"SEQIK_FK": (1, 1024, 256, 64 * 27), "SEQIK_FRAMES": (1, 256, 256, 64 * 27), "SEQIK_JAC": (1, 256, 256, 64 * 21)}


@pytest.mark.parametrize("prefix", sorted(PLAN_UNITS))
def test_launch_plan_defaults_clamps_and_caps(fk_harness, prefix):
    """The launch plan the three angle-map units share, with the numbers each unit's own launch code gave before the plan
    was shared: 256 threads and the staged kernel by default; a block that is no multiple of 64 in 64..max means 256;
    a staged FK launch takes at most 256; at most 256 * 64 workgroups; <prefix>_GRID caps them further."""
    unit = PLAN_UNITS[prefix]
    w, fk = 8 * unit[3], prefix == "SEQIK_FK"
    plan = lambda n, **env: fk_harness.plan(prefix, n, unit, **env)  # noqa: E731
    assert not [k for k in os.environ if k.startswith(prefix + "_")]
    assert plan(1000) == (1, 256, 4, 4 * w) and plan(1) == (1, 256, 1, 4 * w) and plan(1025) == (1, 256, 5, 4 * w)
    assert plan(1000, STAGED=0) == (0, 256, 4, 0) and plan(1000, STAGED=7) == (1, 256, 4, 4 * w)
    assert fk_harness.plan(prefix, 1000, (0,) + unit[1:], STAGED=1) == (0, 256, 4, 0)   # a request without a record
    for staged in (0, 1):
        lds = lambda block: staged * w * (block // 64)  # noqa: E731
        for bad in (63, 65, 2048, 0, -64, 1088):
            assert plan(1000, STAGED=staged, BLOCK=bad) == (staged, 256, 4, lds(256)), (staged, bad)
        assert plan(1000, STAGED=staged, BLOCK=64) == (staged, 64, 16, lds(64))
        assert plan(1000, STAGED=staged, BLOCK=128) == (staged, 128, 8, lds(128))
        big = 512 if fk and not staged else 256   # per lane FK goes up to 1024; everything else stops at 256
        assert plan(1000, STAGED=staged, BLOCK=512) == (staged, big, -(-1000 // big), lds(big))
        assert plan(5000, STAGED=staged, BLOCK=1024) == ((0, 1024, 5, 0) if fk and not staged else (staged, 256, 20, lds(256)))
    full = 256 * 64 * 256
    assert plan(full)[2] == 256 * 64 == plan(full + 1)[2] == plan(6_000_000_000)[2] and plan(full - 256)[2] == 256 * 64 - 1
    assert plan(full + 1, BLOCK=64)[2] == 256 * 64
    assert plan(1573, GRID=3) == (1, 256, 3, 4 * w) and plan(421, GRID=3, BLOCK=64, STAGED=0) == (0, 64, 3, 0)
    assert plan(1000, GRID=4)[2] == 4 == plan(1000, GRID=9)[2] == plan(1000, GRID=0)[2] == plan(1000, GRID=-2)[2]
    assert plan(1000, GRID=1)[2] == 1


def _call(lib, fn, angles, n_seq, n_legs, n_frames, legs, kind, pose, origin, fk, dist):
    dp = ctypes.POINTER(ctypes.c_double)
    p = lambda a: a.ctypes.data_as(dp) if a is not None else None  # noqa: E731
    if fn == "host":
        return lib.seqik_forward_kinematics(p(angles), n_seq, n_legs, n_frames, legs, kind, p(pose), p(origin), p(fk),
                                            p(dist), -1)
    v = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None  # noqa: E731
    return lib.seqik_forward_kinematics_device(v(angles), n_seq, n_legs, n_frames, legs, kind, v(pose), v(origin),
                                               v(fk), v(dist), None)


@pytest.mark.parametrize("fn", ["host", "device"])
def test_fk_argument_errors_through_the_c_abi(hiplib, fn):
    """Every SEQIK_ERR_BAD_ARG case, each with its message, before anything touches HIP (host pointers are fine: the
    checks come first)."""
    lib = hiplib.load()
    z = load_golden("df3d_100")
    legs = (hiplib.SeqikLegParams * 8)(*[hiplib.leg_params_from_arrays(z["RF_seg"], z["RF_bounds"], z["RF_seeds"])] * 8)
    ang, fk = np.zeros((1, 1, 4, 7)), np.zeros((1, 1, 4, 9, 3))
    pose, org, dist = np.zeros((1, 1, 4, 5, 3)), np.zeros((1, 1, 4, 3)), np.zeros((1, 1, 4, 4))
    cases = [
        (dict(n_legs=0), "n_legs must lie in 1..8"),
        (dict(n_legs=9), "n_legs must lie in 1..8"),
        (dict(n_seq=-1), "negative n_seq or n_frames"),
        (dict(n_frames=-4), "negative n_seq or n_frames"),
        (dict(angles=None), "angles and fk must not be null"),
        (dict(fk=None), "angles and fk must not be null"),
        (dict(kind=2), "kind must be 0"),
        (dict(kind=-1), "kind must be 0"),
        (dict(pose=pose, origin=org), "pose or origin, not both"),
        (dict(dist=dist), "dist needs pose"),
        (dict(dist=dist, origin=org), "dist needs pose"),
    ]
    bad_seg = (hiplib.SeqikLegParams * 1)(hiplib.leg_params_from_arrays(z["RF_seg"], z["RF_bounds"], z["RF_seeds"]))
    bad_seg[0].seg[2] = float("inf")
    for kw, msg in cases + [(dict(legs=bad_seg), "non-finite segment length")]:
        a = dict(angles=ang, n_seq=1, n_legs=1, n_frames=4, legs=legs, kind=0, pose=None, origin=None, fk=fk, dist=None)
        a.update(kw)
        rc = _call(lib, fn, **a)
        assert rc == hiplib.ERR_ARG, (kw, rc)
        assert msg in lib.seqik_last_error().decode(), (kw, lib.seqik_last_error())
    nan_seg = (hiplib.SeqikLegParams * 1)(hiplib.leg_params_from_arrays(z["RF_seg"], z["RF_bounds"], z["RF_seeds"]))
    nan_seg[0].seg[0] = float("nan")
    a = dict(angles=ang, n_seq=1, n_legs=1, n_frames=4, legs=nan_seg, kind=1, pose=None, origin=None, fk=fk, dist=None)
    assert _call(lib, fn, **a) == hiplib.ERR_ARG


def test_fk_python_argument_errors(hiplib):
    z = load_golden("df3d_100")
    lp = [hiplib.leg_params_from_arrays(z["RF_seg"], z["RF_bounds"], z["RF_seeds"])]
    ang = z["RF_angles"][None, None]
    with pytest.raises(ValueError, match="shape"):
        hiplib.forward_kinematics(ang[0], lp)
    with pytest.raises(ValueError, match="kind"):
        hiplib.forward_kinematics(ang, lp, kind="ikpy")
    with pytest.raises(ValueError, match="want_dist needs pose"):
        hiplib.forward_kinematics(ang, lp, want_dist=True)
    with pytest.raises(ValueError, match="not both"):
        hiplib.forward_kinematics(ang, lp, pose=z["RF_pose"][None, None], origin=np.zeros(3))
    with pytest.raises(ValueError, match="one SeqikLegParams per leg"):
        hiplib.forward_kinematics(ang, lp * 2)


# ---------------------------------------------------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(hiplib):
    return gpu_lib(hiplib)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["df3d_100", "df3d_1000"])
def test_gpu_fk_equals_solve_seq_fk_bit_for_bit(lib, name):
    z = load_golden(name)
    legs = [str(l) for l in z["legs"]]
    pose, params = _stack(z, legs), _params(lib, z, legs)
    for chunk in (0, -1):
        out = lib.solve_seq(pose, params, want_fk=True, frame_chunk=chunk)
        fk = lib.forward_kinematics(out["angles"], params, kind="seq", pose=pose)["fk"]
        assert np.array_equal(fk, out["fk"]), chunk


@pytest.mark.gpu
def test_gpu_fk_equals_solve_seq_fk_on_the_shipped_recording(lib):
    """The full 6000-frame anipose recording, RF + LF, serial walk and frame chunks."""
    z = load_golden("anipose_shipped")
    legs = ["RF", "LF"]
    pose, params = _stack(z, legs), _params(lib, z, legs)
    for chunk in (0, -1):
        out = lib.solve_seq(pose, params, want_fk=True, frame_chunk=chunk)
        for kind in ("seq", 0):
            fk = lib.forward_kinematics(out["angles"], params, kind=kind, pose=pose)["fk"]
            assert np.array_equal(fk, out["fk"]), (chunk, kind)


@pytest.mark.gpu
def test_gpu_fk_equals_solver_fk_on_a_synthetic_batch(lib):
    """A million leg-frames of the benchmark's workload (six legs, 64-frame recordings), sequential chain; and a smaller
    batch through the generic solver."""
    from seqikpy_amd import data, synthetic, utils
    legs = data.LEGS
    body = utils.calculate_body_size(data.TEMPLATE_NMF_LOCOMOTION, legs)
    params = [lib.make_leg_params(l, data.BOUNDS_LOCOMOTION, body, data.INITIAL_ANGLES_LOCOMOTION) for l in legs]
    S, N = 2731, 64
    assert S * len(legs) * N >= 1_000_000
    pose = synthetic.synthetic_pose(S, N, legs, data.BOUNDS_LOCOMOTION, body, data.TEMPLATE_NMF_LOCOMOTION,
                                    variant="iid", seed=11)
    out = lib.solve_seq(pose, params, want_fk=True)
    res = lib.forward_kinematics(out["angles"], params, kind="seq", pose=pose, want_dist=True)
    assert np.array_equal(res["fk"], out["fk"])
    ref = np.linalg.norm(out["fk"][..., [4, 6, 7, 8], :] - pose[..., 1:, :], axis=-1)
    assert np.array_equal(np.isnan(res["dist"]), np.isnan(ref))
    assert np.abs(res["dist"] - ref).max() <= 1e-15 * max(1.0, np.abs(ref).max())
    # the generic chain is seeded positionally in its own link order (roll, yaw, pitch, ...): mid-range seeds
    gparams = []
    for l in legs:
        b = np.array([data.BOUNDS_LOCOMOTION[f"{l}_{d}"] for d in DOFS])
        seeds = np.zeros(27)
        seeds[19:26] = b[[2, 0, 1, 3, 4, 5, 6]].mean(axis=1)
        gparams.append(lib.leg_params_from_arrays([body[f"{l}_{s}"] for s in data.SEGMENTS], b, seeds))
    gen = lib.solve_generic(pose[:64], gparams)
    fk = lib.forward_kinematics(gen["angles"], gparams, kind="generic", pose=pose[:64])["fk"]
    assert np.array_equal(fk, gen["fk"])


@pytest.mark.gpu
def test_gpu_fk_equals_solve_generic_fk(lib):
    for name in ("generic_rf_100", "df3d_100"):
        z = load_golden(name)
        legs = [str(l) for l in z["legs"]]
        pose, params = _stack(z, legs), (_params if name == "generic_rf_100" else _generic_params)(lib, z, legs)
        out = lib.solve_generic(pose, params)
        fk = lib.forward_kinematics(out["angles"], params, kind="generic", pose=pose)["fk"]
        assert np.array_equal(fk, out["fk"]), name


@pytest.mark.gpu
def test_gpu_fk_fused_alignment_origin_is_template_coxa(lib):
    """Fused alignment (SeqikAffine): the solvers' origin is template_coxa -- passed as `origin`, broadcast per leg."""
    from seqikpy_amd import data
    from seqikpy_amd.alignment import AlignPose
    z = load_golden("df3d_1000")
    legs = [str(l) for l in z["legs"]]
    raw = {f"{l}_leg": z[f"{l}_raw"] for l in legs}
    al = AlignPose(raw, legs, body_template=data.TEMPLATE_NMF_LOCOMOTION, log_level="ERROR")
    aff = [al.leg_affine(raw[f"{l}_leg"], l) for l in legs]
    params = _params(lib, z, legs)
    pose_raw = np.stack([raw[f"{l}_leg"] for l in legs])[None]
    tc = np.stack([a[2] for a in aff])[None, :, None, :]
    out = lib.solve_seq(pose_raw, params, want_fk=True, affine=[lib.make_affine(*a) for a in aff])
    assert np.array_equal(lib.forward_kinematics(out["angles"], params, origin=tc)["fk"], out["fk"])
    gparams = _generic_params(lib, z, legs)
    gen = lib.solve_generic(pose_raw[:, :, :100], gparams, affine=[lib.make_affine(*a) for a in aff])
    assert np.array_equal(lib.forward_kinematics(gen["angles"], gparams, kind="generic", origin=tc)["fk"], gen["fk"])


@pytest.mark.gpu
def test_gpu_fk_device_entry_point_on_a_torch_stream(lib):
    import torch
    z = load_golden("df3d_1000")
    legs = [str(l) for l in z["legs"]]
    params = _params(lib, z, legs)
    ang = np.stack([z[f"{l}_angles"] for l in legs])[None]
    pose = _stack(z, legs)
    host = lib.forward_kinematics(ang, params, pose=pose, want_dist=True)
    d_ang, d_pose = torch.from_numpy(ang).cuda(), torch.from_numpy(pose).cuda()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_fk = torch.full((1, 6, 1000, 9, 3), float("nan"), dtype=torch.float64, device="cuda")
        d_dist = torch.full((1, 6, 1000, 4), float("nan"), dtype=torch.float64, device="cuda")
        lib.forward_kinematics_device(d_ang.data_ptr(), 1, 6, 1000, params, d_fk.data_ptr(), kind="seq",
                                      d_pose=d_pose.data_ptr(), d_dist=d_dist.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(d_fk.cpu().numpy(), host["fk"])
    assert np.array_equal(d_dist.cpu().numpy(), host["dist"])
    # both kernel variants (LDS-staged, the default, and per lane; SEQIK_FK_STAGED is read per call), including a range
    # that ends in a partial wavefront
    for staged in ("0", "1"):
        with switches(SEQIK_FK_STAGED=staged):
            v = lib.forward_kinematics(ang[:, :, :997], params, pose=pose[:, :, :997], want_dist=True)
        assert np.array_equal(v["fk"], host["fk"][:, :, :997]) and np.array_equal(v["dist"], host["dist"][:, :, :997])
    for kind in ("seq", "generic"):
        ref = lib.forward_kinematics(ang, params, kind=kind, origin=pose[..., 0, :])["fk"]
        d_org = torch.from_numpy(np.ascontiguousarray(pose[..., 0, :])).cuda()
        out = torch.empty((1, 6, 1000, 9, 3), dtype=torch.float64, device="cuda")
        lib.forward_kinematics_device(d_ang.data_ptr(), 1, 6, 1000, params, out.data_ptr(), kind=kind,
                                      d_origin=d_org.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), ref), kind


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1])
def test_gpu_fk_block_sizes_and_a_capped_grid(lib, fk_harness, kind):
    """SEQIK_FK_GRID = 3 at 2 * 3 * block + 37 leg-frames: every workgroup makes two full trips of the grid-stride loop and
    the third is ragged -- whole wavefronts, then a partial one on the per-lane path.  SEQIK_FK_BLOCK 64 and 256 with both
    kernels, 1024 per lane (seven legs: the trips straddle leg seams), two sequences of three legs, and once with pose
    and dist.  Bit for bit against the host-run rule, guard records around every output."""
    import torch
    runs = [(1, 1, 2 * 3 * b + 37, st, b, False) for st in ("0", "1") for b in (64, 256)]
    runs += [(1, 7, (2 * 3 * 1024 + 37) // 7, "0", 1024, False), (1, 1, 2 * 3 * 256 + 37, "1", 256, True)]
    runs += [(2, 3, 71, st, 64, True) for st in ("0", "1")]
    assert 7 * runs[4][2] == 2 * 3 * 1024 + 37 and 2 * 3 * 71 > 2 * 3 * 64 + 37
    for S, L, N, staged, block, with_pose in runs:
        ang, segs, org = made_up_batch(S, L, N, 40 + block)
        pose = np.random.default_rng(block).standard_normal((S, L, N, 5, 3))
        src = dict(pose=pose) if with_pose else dict(origin=org)
        ref = [fk_harness.fk(ang[:, l].reshape(-1, 7), segs[l], kind, want_dist=with_pose,
                             **{k: v[:, l].reshape((S * N,) + v.shape[3:]) for k, v in src.items()}) for l in range(L)]
        d_ang, d_src = torch.from_numpy(ang).cuda(), torch.from_numpy(pose if with_pose else org).cuda()
        (fk, p_fk), (dist, p_dist) = guarded(S * L * N, 27), guarded(S * L * N, 4)
        params = [lib.leg_params_from_arrays(s, np.zeros((7, 2)), np.zeros(27)) for s in segs]
        with switches(SEQIK_FK_STAGED=staged, SEQIK_FK_BLOCK=str(block), SEQIK_FK_GRID="3"):
            lib.forward_kinematics_device(d_ang, S, L, N, params, p_fk, kind=kind, d_dist=p_dist if with_pose else 0,
                                          stream=torch.cuda.current_stream().cuda_stream,
                                          **{"d_pose" if with_pose else "d_origin": d_src})
            torch.cuda.synchronize()
        got_fk, got_dist = unguarded(fk, 27).reshape(S, L, N, 9, 3), unguarded(dist, 4).reshape(S, L, N, 4)
        for l in range(L):
            assert same_bits(got_fk[:, l].reshape(-1, 9, 3), ref[l][0]), (kind, S, L, N, staged, block, with_pose, l)
            if with_pose:
                assert same_bits(got_dist[:, l].reshape(-1, 4), ref[l][1]), (kind, S, L, N, staged, block, l)
        assert with_pose or (got_dist == SENTINEL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["seq", "generic"])
def test_gpu_fk_segment_lengths_are_invariant_at_config3_size(lib, kind):
    """Independent of any implementation: for random in-bounds angles (6 legs x 1 M frames, as 15625 recordings of 64
    frames) the distances between rows 0->4, 4->6, 6->7, 7->8 are the segment lengths."""
    import torch
    from seqikpy_amd import data, utils
    legs = data.LEGS
    body = utils.calculate_body_size(data.TEMPLATE_NMF_LOCOMOTION, legs)
    params = [lib.make_leg_params(l, data.BOUNDS_LOCOMOTION, body, data.INITIAL_ANGLES_LOCOMOTION) for l in legs]
    S, L, N = 15625, 6, 64
    lb = torch.tensor([[data.BOUNDS_LOCOMOTION[f"{l}_{d}"][0] for d in DOFS] for l in legs], dtype=torch.float64)
    ub = torch.tensor([[data.BOUNDS_LOCOMOTION[f"{l}_{d}"][1] for d in DOFS] for l in legs], dtype=torch.float64)
    g = torch.Generator(device="cuda").manual_seed(5)
    u = torch.rand((S, L, N, 7), dtype=torch.float64, device="cuda", generator=g)
    ang = (lb.cuda()[None, :, None] + u * (ub - lb).cuda()[None, :, None]).contiguous()
    org = torch.randn((S, L, N, 3), dtype=torch.float64, device="cuda", generator=g)
    fk = torch.empty((S, L, N, 9, 3), dtype=torch.float64, device="cuda")
    lib.forward_kinematics_device(ang.data_ptr(), S, L, N, params, fk.data_ptr(), kind=kind, d_origin=org.data_ptr(),
                                  stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(fk[:, :, :, 0], org)
    seg = torch.tensor([[body[f"{l}_{s}"] for s in data.SEGMENTS] for l in legs], dtype=torch.float64).cuda()
    rows = [0, 4, 6, 7, 8]
    for k in range(4):
        d = torch.linalg.vector_norm(fk[:, :, :, rows[k + 1]] - fk[:, :, :, rows[k]], dim=-1)
        rel = ((d - seg[None, :, None, k]).abs() / seg[None, :, None, k]).max().item()
        assert rel <= 1e-12, (kind, k, rel)


@pytest.mark.gpu
def test_gpu_fk_nan_angle_and_empty_inputs(lib):
    z = load_golden("df3d_100")
    legs = [str(l) for l in z["legs"]]
    params = _params(lib, z, legs)
    ang = np.stack([z[f"{l}_angles"] for l in legs])[None]
    pose = _stack(z, legs)
    clean = lib.forward_kinematics(ang, params, pose=pose, want_dist=True)
    bad = ang.copy()
    bad[0, 2, 40, 3] = np.nan
    bad[0, 4, 99, 0] = np.inf
    out = lib.forward_kinematics(bad, params, pose=pose, want_dist=True)
    hit = np.zeros(ang.shape[:3], bool)
    hit[0, 2, 40] = hit[0, 4, 99] = True
    assert np.isnan(out["fk"][hit]).all() and np.isnan(out["dist"][hit]).all()
    assert out["fk"][~hit].tobytes() == clean["fk"][~hit].tobytes()
    assert out["dist"][~hit].tobytes() == clean["dist"][~hit].tobytes()
    assert lib.forward_kinematics(ang[:, :, :0], params, pose=pose[:, :, :0])["fk"].shape == (1, 6, 0, 9, 3)
    assert lib.forward_kinematics(ang[:0], params, want_dist=True, pose=pose[:0])["dist"].shape == (0, 6, 100, 4)
    # a tail that is not a whole wavefront, one leg-frame alone
    one = lib.forward_kinematics(ang[:, :1, 7:8], params[:1], pose=pose[:, :1, 7:8])["fk"]
    assert np.array_equal(one[0, 0, 0], clean["fk"][0, 0, 7])


@pytest.mark.gpu
def test_gpu_leg_inv_kin_run_fk_and_fit_error(lib, tmp_path):
    from seqikpy_amd.data import BOUNDS, INITIAL_ANGLES
    from seqikpy_amd.kinematic_chain import KinematicChainGeneric, KinematicChainSeq
    from seqikpy_amd.leg_inverse_kinematics import LegInvKinGeneric, LegInvKinSeq
    za = load_golden("anipose_shipped")
    aligned = {"RF_leg": za["RF_pose"][:500], "LF_leg": za["LF_pose"][:500]}
    ik = LegInvKinSeq(aligned, KinematicChainSeq(BOUNDS, ["RF", "LF"]), INITIAL_ANGLES, log_level="ERROR")
    ang, fk = ik.run_ik_and_fk()
    again = ik.run_fk(export_path=tmp_path)
    assert list(again) == list(fk)
    for k in fk:
        assert again[k].dtype == fk[k].dtype and again[k].shape == fk[k].shape
        assert np.array_equal(again[k], fk[k]), k
    with open(tmp_path / "forward_kinematics.pkl", "rb") as f:
        saved = pickle.load(f)
    assert all(np.array_equal(saved[k], fk[k]) for k in fk)
    assert not (tmp_path / "leg_joint_angles.pkl").exists()
    # explicit angles (a copy of the dict), an explicit origin
    assert np.array_equal(ik.run_fk(dict(ang))["RF_leg"], fk["RF_leg"])
    o = ik.run_fk(origin=np.zeros(3))
    assert np.abs(o["LF_leg"] + za["LF_pose"][:500, :1] - fk["LF_leg"]).max() < 1e-14
    per_frame = ik.run_fk(origin=za["RF_pose"][:500, 0])
    assert np.array_equal(per_frame["RF_leg"], fk["RF_leg"])
    err = ik.fit_error()
    assert list(err) == ["RF_leg", "LF_leg"] and err["RF_leg"].shape == (500, 4)
    ref = np.linalg.norm(fk["RF_leg"][:, [4, 6, 7, 8]] - za["RF_pose"][:500, 1:5], axis=-1)
    assert np.abs(err["RF_leg"] - ref).max() <= 1e-15 * max(1.0, ref.max())
    # errors
    missing = {k: v for k, v in ang.items() if k != "Angle_LF_CTr_roll"}
    with pytest.raises(ValueError, match="Angle_LF_CTr_roll"):
        ik.run_fk(missing)
    short = {k: v[:400] for k, v in ang.items()}
    with pytest.raises(ValueError, match="400.*500"):
        ik.run_fk(short)
    assert ik.run_fk(short, origin=np.zeros(3))["RF_leg"].shape == (400, 9, 3)
    with pytest.raises(ValueError, match="origin must have shape"):
        ik.run_fk(origin=np.zeros((7, 3)))
    # the generic chain: its own kind
    gen = LegInvKinGeneric({"RF_leg": za["RF_pose"][:100]}, KinematicChainGeneric(BOUNDS, ["RF"]), INITIAL_ANGLES,
                           log_level="ERROR")
    gang, gfk = gen.run_ik_and_fk()
    gagain = gen.run_fk()
    assert np.array_equal(gagain["RF_leg"], gfk["RF_leg"])
    assert gen.fit_error()["RF_leg"].shape == (100, 4)
    assert np.abs(gen.fit_error()["RF_leg"][:, 3]).max() < 1e-3  # the generic chain fits the claw only


@pytest.mark.gpu
def test_gpu_leg_inv_kin_run_fk_with_fused_alignment(lib):
    from seqikpy_amd import data
    from seqikpy_amd.alignment import AlignPose
    from seqikpy_amd.kinematic_chain import KinematicChainSeq
    from seqikpy_amd.leg_inverse_kinematics import LegInvKinSeq
    from seqikpy_amd.utils import calculate_body_size
    z = load_golden("df3d_1000")
    legs = [str(l) for l in z["legs"]]
    raw = {f"{l}_leg": z[f"{l}_raw"][:200] for l in legs}
    al = AlignPose(raw, legs, body_template=data.TEMPLATE_NMF_LOCOMOTION, log_level="ERROR")
    body = calculate_body_size(data.TEMPLATE_NMF_LOCOMOTION, legs)
    ik = LegInvKinSeq(raw, KinematicChainSeq(data.BOUNDS_LOCOMOTION, legs, body), data.INITIAL_ANGLES_LOCOMOTION,
                      log_level="ERROR", leg_affine=al.leg_affines())
    _, fk = ik.run_ik_and_fk()
    again = ik.run_fk()
    for k in fk:
        assert np.array_equal(again[k], fk[k]), k
    assert np.isfinite(ik.fit_error()["RM_leg"]).all()
