"""Skip mode for missing key points (include/seqik_gaps.h, csrc/seqik_gaps.hpp / seqik_gaps.hip).

CPU tier: the header and exports, the per-frame rules run on the host against a numpy construction, the whole contract
on the host (compact -> host-run solver -> expand == the solver on the recording with the gap frames deleted), Python
argument handling.  GPU tier (`-m gpu`): the host entry points against the solver on deleted / compacted-and-padded
recordings (serial, chunked, fused alignment, generic, an all-missing leg), the device building blocks on torch tensors,
and the LegInvKin* dictionaries."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, leg_arrays, load_golden
from gaps_model import (inject_gaps, load_gaps_harness, np_compact, np_compact_batch, np_expand, np_expand_batch,
                        np_missing, rows_read)

GAPS_SYMBOLS = ["seqik_gaps_compact_device", "seqik_gaps_expand_device", "seqik_solve_seq_gaps",
                "seqik_solve_generic_gaps"]
MISSING = -100


@pytest.fixture(scope="module")
def gaps_harness():
    h = load_gaps_harness()
    if h is None:
        pytest.skip("hipcc not available")
    return h


# ---------------------------------------------------------------------------------------------------------------------
# CPU tier
# ---------------------------------------------------------------------------------------------------------------------

def test_gaps_header_declares_exactly_the_new_entry_points(hiplib):
    text = open(os.path.join(ROOT, "include", "seqik_gaps.h")).read()
    assert re.search(r"#define SEQIK_STATUS_MISSING \(-100\)", text)
    assert hiplib.STATUS_MISSING == MISSING and MISSING not in range(-1, 5)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(seqik_[a-z_]+)\s*\(", text)))
    assert declared == sorted(GAPS_SYMBOLS)
    assert sorted(hiplib.GAPS_EXPORTED_SYMBOLS) == declared
    assert not set(declared) & set(hiplib.EXPORTED_SYMBOLS)
    assert not set(declared) & set(hiplib.FK_EXPORTED_SYMBOLS)
    lib = hiplib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.seqik_abi_version() == 7 == hiplib.ABI_VERSION
    assert "seqik_gaps.hip" in hiplib.COMPILE_UNITS
    assert {"seqik_gaps.hip", "seqik_gaps.hpp"} <= set(hiplib.SOURCES)
    assert "seqik_gaps.h" in open(os.path.join(ROOT, "setup.py")).read()


def _mask_cases(rng, n):
    none = np.zeros(n, bool)
    every = np.ones(n, bool)
    first = none.copy(); first[0] = True
    last = none.copy(); last[-1] = True
    block = none.copy(); block[20:70] = True
    rand = rng.random(n) < 0.3
    return dict(none=none, all=every, first=first, last=last, block=block, random=rand)


@pytest.mark.parametrize("kind,affine", [("seq", False), ("seq", True), ("generic", False), ("generic", True)])
def test_host_compact_and_expand_equal_numpy(gaps_harness, kind, affine):
    rng = np.random.default_rng(7)
    n = 150
    seg = rng.uniform(0.2, 0.8, 4)
    base = rng.normal(size=(n, 5, 3))
    for name, mask in _mask_cases(rng, n).items():
        for value in (np.nan, np.inf, -np.inf):
            pose = base.copy()
            for t in np.flatnonzero(mask):
                pose[t, rng.choice(rows_read(kind, affine)), rng.integers(0, 3)] = value
            # a non-finite value in a row the solver does not read leaves the frame in
            unread = [r for r in range(5) if r not in rows_read(kind, affine)]
            if unread:
                pose[5, unread[0], 1] = np.nan
            cpose, mp, nv = gaps_harness.compact(pose, seg, kind, affine)
            ref_c, ref_m, ref_nv = np_compact(pose, seg, kind, affine)
            assert nv == ref_nv, (name, value)
            assert np.array_equal(mp, ref_m), (name, value)
            assert np.array_equal(cpose, ref_c, equal_nan=True), (name, value)
            if unread and not mask[5]:
                assert mp[5] >= 0
            # expansion: angles-like doubles and status-like ints
            ang = rng.normal(size=(n, 7))
            st = rng.integers(-1, 5, size=(n, 4)).astype(np.int32)
            assert np.array_equal(gaps_harness.expand(mp, ang), np_expand(mp, ang, np.nan), equal_nan=True)
            assert np.array_equal(gaps_harness.expand(mp, st, MISSING), np_expand(mp, st, MISSING))


def test_host_contract_equals_solver_on_deleted_recording(host_harness, gaps_harness):
    """Host compact -> the solver's device code run on the host -> host expand == the same solver on the recording with
    the missing frames deleted, bit for bit (serial walk); missing frames are NaN / SEQIK_STATUS_MISSING / 0."""
    z = load_golden("df3d_1000")
    rng = np.random.default_rng(3)
    for leg in ["RF", "LH"]:
        pose, seg, b, seeds = leg_arrays(z, leg)
        gp = inject_gaps(pose[:300], rng, blocks=((40, 90), (299, 300)), values=(np.nan, np.inf, -np.inf))
        miss = np_missing(gp)
        cpose, mp, nv = gaps_harness.compact(gp, seg)
        assert nv == (~miss).sum()
        solved = host_harness.run(cpose, seg, b, seeds, diag=True)
        ang = gaps_harness.expand(mp, solved["angles"])
        fk = gaps_harness.expand(mp, solved["fk"])
        st = gaps_harness.expand(mp, solved["status"], MISSING)
        nf = gaps_harness.expand(mp, solved["nfev"], 0)
        ref = host_harness.run(gp[~miss], seg, b, seeds, diag=True)
        assert np.array_equal(ang[~miss], ref["angles"]), leg
        assert np.array_equal(fk[~miss], ref["fk"]), leg
        assert np.array_equal(st[~miss], ref["status"]) and np.array_equal(nf[~miss], ref["nfev"]), leg
        assert np.isnan(ang[miss]).all() and np.isnan(fk[miss]).all()
        assert (st[miss] == MISSING).all() and (nf[miss] == 0).all()


def test_host_contract_generic(host_harness, gaps_harness):
    z = load_golden("generic_rf_100")
    rng = np.random.default_rng(5)
    pose, seg, b, seeds = leg_arrays(z, "RF")
    gp = inject_gaps(pose, rng, frac=0.1, blocks=((30, 40),), rows=(0, 4))
    t = int(np.flatnonzero(~np_missing(gp, "generic"))[20])
    gp[t, 2] = np.nan  # row 2 is not read by the generic chain
    miss = np_missing(gp, "generic")
    assert not miss[t]
    cpose, mp, nv = gaps_harness.compact(gp, seg, "generic")
    solved = host_harness.run_generic(cpose, seg, b, seeds)
    ref = host_harness.run_generic(gp[~miss], seg, b, seeds)
    assert np.array_equal(gaps_harness.expand(mp, solved["angles"])[~miss], ref["angles"])
    assert np.array_equal(gaps_harness.expand(mp, solved["fk"])[~miss], ref["fk"])


def test_python_argument_handling(hiplib):
    from seqikpy_amd.kinematic_chain import KinematicChainSeq
    from seqikpy_amd.leg_inverse_kinematics import LegInvKinSeq
    from seqikpy_amd.data import BOUNDS
    z = load_golden("df3d_100")
    pose = z["RF_pose"][:8].copy()
    pose[3, 2, 0] = np.nan
    lp = hiplib.leg_params_from_arrays(z["RF_seg"], z["RF_bounds"], z["RF_seeds"])
    with pytest.raises(ValueError, match="Residuals are not finite"):
        hiplib.solve_seq(pose[None, None], [lp])
    with pytest.raises(ValueError, match="Residuals are not finite"):
        hiplib.solve_generic(pose[None, None], [lp])
    with pytest.raises(ValueError, match="missing"):
        hiplib.solve_seq(pose[None, None], [lp], missing="interpolate")
    with pytest.raises(ValueError, match="four stages"):
        hiplib.solve_seq(pose[None, None], [lp], 1, 2, missing="skip")
    ik = LegInvKinSeq({"RF_leg": pose}, KinematicChainSeq(BOUNDS, ["RF"]), log_level="ERROR")
    with pytest.raises(ValueError, match="missing key points"):
        ik.run_ik_and_fk(missing_key_points="fill")
    with pytest.raises(ValueError, match="stages"):
        ik.run_ik_and_fk(missing_key_points="skip", stages=[1, 2])
    with pytest.raises(ValueError, match="Residuals are not finite"):
        ik.run_ik_and_fk()


def test_gaps_c_abi_argument_errors(hiplib):
    lib = hiplib.load()
    lp = (hiplib.SeqikLegParams * 1)()
    for i in range(4):
        lp[0].seg[i] = 0.5
    buf = ctypes.c_void_p(16)  # never dereferenced: every call below fails its checks before any launch
    cases = [
        (dict(flags=4), "unknown flags"),
        (dict(n_legs=0), "n_legs"),
        (dict(n_frames=-1), "negative"),
        (dict(n_frames=2 ** 31), "2^31"),
        (dict(pose=None), "must not be null"),
    ]
    for over, msg in cases:
        a = dict(pose=buf, n_seq=1, n_legs=1, n_frames=4, flags=0)
        a.update(over)
        rc = lib.seqik_gaps_compact_device(a["pose"], a["n_seq"], a["n_legs"], a["n_frames"], a["flags"], lp, buf, buf,
                                           buf, None)
        assert rc == hiplib.ERR_ARG, over
        assert msg in lib.seqik_last_error().decode(), (over, lib.seqik_last_error())
    rc = lib.seqik_gaps_expand_device(buf, 1, 1, 4, 0, buf, buf, None, None, buf, None, None, None, None)
    assert rc == hiplib.ERR_ARG and b"pairs" in lib.seqik_last_error()
    # no leg-frames: OK without a launch (no GPU needed)
    assert lib.seqik_gaps_compact_device(buf, 0, 1, 4, 0, lp, buf, buf, buf, None) == 0
    assert lib.seqik_gaps_expand_device(buf, 1, 1, 0, 0, buf, None, None, None, buf, None, None, None, None) == 0
    dp = ctypes.POINTER(ctypes.c_double)
    pose = np.zeros((1, 1, 4, 5, 3))
    ang = np.zeros((1, 1, 4, 7))
    rc = lib.seqik_solve_seq_gaps(pose.ctypes.data_as(dp), 1, 1, 4, lp, 1, 3, ang.ctypes.data_as(dp), None, None, None,
                                  None, None, None, None)
    assert rc == hiplib.ERR_ARG and b"four stages" in lib.seqik_last_error()
    opt = hiplib.SeqikOptions()
    opt.frame_lead = 8
    rc = lib.seqik_solve_seq_gaps(pose.ctypes.data_as(dp), 1, 1, 4, lp, 1, 4, ang.ctypes.data_as(dp), None, None, None,
                                  None, None, ctypes.byref(opt), None)
    assert rc == hiplib.ERR_ARG and b"not supported" in lib.seqik_last_error()
    assert lib.seqik_solve_generic_gaps(pose.ctypes.data_as(dp), 1, 1, 0, lp, ang.ctypes.data_as(dp), None, None, None,
                                        None, None, None, None) == 0


def test_align_pose_skip_mode(hiplib):
    from seqikpy_amd.alignment import AlignPose
    z = load_golden("anipose_shipped")
    rng = np.random.default_rng(11)
    legs = ["RF", "LF"]
    pose = {f"{l}_leg": np.array(z[f"{l}_pose"][:2000], copy=True) for l in legs}
    # finite data: skip mode is the default bit for bit
    a = AlignPose(pose, legs_list=legs, log_level="ERROR").align_pose()
    b = AlignPose(pose, legs_list=legs, log_level="ERROR", missing_key_points="skip").align_pose()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    with pytest.raises(ValueError, match="missing key points"):
        AlignPose(pose, legs_list=legs, missing_key_points="drop")
    gapped = {k: inject_gaps(v, rng, frac=0.05, blocks=((100, 160),)) for k, v in pose.items()}
    al = AlignPose(gapped, legs_list=legs, log_level="ERROR", missing_key_points="skip")
    out = al.align_pose()
    for l in legs:
        raw = gapped[f"{l}_leg"]
        miss = ~np.isfinite(raw[:, 1:]).all(axis=(1, 2))    # row 0 becomes the template's coxa
        fixed, scale, template = al.leg_affine(raw, l)
        assert np.isfinite(fixed).all() and np.isfinite(scale)
        mq = lambda v: 0.5 * (np.nanquantile(v, 0.45) + np.nanquantile(v, 0.55))
        assert np.array_equal(fixed, np.array([mq(raw[:, 0, i]) for i in range(3)]))
        # aligned frames with a missing key point stay non-finite, the others are finite
        assert (~np.isfinite(out[f"{l}_leg"]).all(axis=(1, 2)) == miss).all()
    # a leg that was never triangulated: NaN constants (np.nanquantile of an all-NaN series), every frame missing
    never = dict(gapped, LF_leg=np.full_like(gapped["LF_leg"], np.nan))
    al = AlignPose(never, legs_list=legs, log_level="ERROR", missing_key_points="skip")
    fixed, scale, _ = al.leg_affine(never["LF_leg"], "LF")
    assert np.isnan(fixed).all() and np.isnan(scale)
    out = al.align_pose()
    assert np.isnan(out["LF_leg"][:, 1:]).all()
    assert np.array_equal(out["RF_leg"], AlignPose(gapped, legs_list=legs, log_level="ERROR",
                                                   missing_key_points="skip").align_pose()["RF_leg"], equal_nan=True)
    # the default still propagates the NaN into the statistics
    d = AlignPose(gapped, legs_list=legs, log_level="ERROR")
    assert not np.isfinite(d.leg_affine(gapped["RF_leg"], "RF")[1])


# ---------------------------------------------------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------------------------------------------------

def _params(hiplib, z, legs):
    return [hiplib.leg_params_from_arrays(z[f"{l}_seg"], z[f"{l}_bounds"], z[f"{l}_seeds"]) for l in legs]


def _anipose_df3d_cases():
    rng = np.random.default_rng(2024)
    out = []
    a = load_golden("anipose_shipped")
    out.append(("anipose", ["RF", "LF"], np.stack([inject_gaps(a[f"{l}_pose"], rng, blocks=((500, 560), (5990, 6000)))
                                                   for l in ["RF", "LF"]])))
    d = load_golden("df3d_1000")
    legs = ["RF", "RM", "RH", "LF", "LM", "LH"]
    out.append(("df3d", legs, np.stack([inject_gaps(d[f"{l}_pose"], rng, blocks=((0, 3), (400, 470))) for l in legs])))
    return out, a, d


@pytest.mark.gpu
def test_serial_skip_equals_solve_of_deleted_recording(hiplib):
    cases, a, d = _anipose_df3d_cases()
    for name, legs, pose in cases:
        z = a if name == "anipose" else d
        params = _params(hiplib, z, legs)
        out = hiplib.solve_seq(pose[None], params, want_diag=True, missing="skip")
        miss = np_missing(pose)
        assert np.array_equal(out["n_valid"][0], (~miss).sum(axis=1))
        for li, leg in enumerate(legs):
            keep = ~miss[li]
            ref = hiplib.solve_seq(pose[li][keep][None, None], [params[li]], want_diag=True)
            assert np.array_equal(out["angles"][0, li][keep], ref["angles"][0, 0]), (name, leg)
            assert np.array_equal(out["fk"][0, li][keep], ref["fk"][0, 0]), (name, leg)
            assert np.array_equal(out["status"][0, li][keep], ref["status"][0, 0]), (name, leg)
            assert np.array_equal(out["nfev"][0, li][keep], ref["nfev"][0, 0]), (name, leg)
            assert np.isnan(out["angles"][0, li][~keep]).all() and np.isnan(out["fk"][0, li][~keep]).all()
            assert (out["status"][0, li][~keep] == MISSING).all() and (out["nfev"][0, li][~keep] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [-1, 16])
def test_chunked_skip_equals_solve_of_compacted_and_padded(hiplib, chunk):
    cases, a, d = _anipose_df3d_cases()
    for name, legs, pose in cases:
        z = a if name == "anipose" else d
        params = _params(hiplib, z, legs)
        out = hiplib.solve_seq(pose[None], params, frame_chunk=chunk, missing="skip")
        padded = np.stack([np_compact(pose[li], z[f"{l}_seg"])[0] for li, l in enumerate(legs)])
        ref = hiplib.solve_seq(padded[None], params, frame_chunk=chunk)
        assert out["chunk_stats"] == ref["chunk_stats"]
        miss = np_missing(pose)
        for li in range(len(legs)):
            mp = np_compact(pose[li], z[f"{legs[li]}_seg"])[1]
            assert np.array_equal(out["angles"][0, li], np_expand(mp, ref["angles"][0, li], np.nan), equal_nan=True)
            assert np.array_equal(out["fk"][0, li], np_expand(mp, ref["fk"][0, li], np.nan), equal_nan=True)
            assert np.isnan(out["angles"][0, li][miss[li]]).all()


@pytest.mark.gpu
def test_skip_on_finite_input_equals_default(hiplib):
    z = load_golden("df3d_1000")
    legs = ["RF", "RM", "RH", "LF", "LM", "LH"]
    pose = np.stack([z[f"{l}_pose"] for l in legs])[None]
    params = _params(hiplib, z, legs)
    for fc in (0, -1):
        a = hiplib.solve_seq(pose, params, frame_chunk=fc)
        b = hiplib.solve_seq(pose, params, frame_chunk=fc, missing="skip")
        assert np.array_equal(a["angles"], b["angles"]) and np.array_equal(a["fk"], b["fk"]), fc
        assert (b["n_valid"] == 1000).all()


@pytest.mark.gpu
def test_fused_affine_ignores_row_0(hiplib):
    z = load_golden("df3d_1000")
    legs = ["RF", "LF"]
    raw = np.stack([z[f"{l}_pose"][:200] for l in legs])
    params = _params(hiplib, z, legs)
    aff = [hiplib.make_affine(raw[li, :, 0].mean(axis=0), 1.1, [0.1 * li, 0.2, -0.3]) for li in range(2)]
    gp = raw.copy()
    gp[0, 10, 0, 1] = np.nan            # row 0 only: read neither with the fused alignment
    gp[1, 20:25, 0, :] = np.inf
    out = hiplib.solve_seq(gp[None], params, affine=aff, missing="skip")
    plain = hiplib.solve_seq(raw[None], params, affine=aff)
    assert (out["n_valid"] == 200).all()
    assert np.array_equal(out["angles"], plain["angles"]) and np.array_equal(out["fk"], plain["fk"])
    gp[0, 30, 2, 0] = np.nan            # row 2 is read: that frame is missing
    out = hiplib.solve_seq(gp[None], params, affine=aff, missing="skip")
    assert out["n_valid"][0, 0] == 199 and np.isnan(out["angles"][0, 0, 30]).all()
    keep = np.arange(200) != 30
    ref = hiplib.solve_seq(raw[0][keep][None, None], params[:1], affine=aff[:1])
    assert np.array_equal(out["angles"][0, 0][keep], ref["angles"][0, 0])


@pytest.mark.gpu
def test_all_missing_leg_is_nan_and_leaves_the_others_alone(hiplib):
    z = load_golden("df3d_1000")
    legs = ["RF", "RM", "RH"]
    pose = np.stack([z[f"{l}_pose"][:300] for l in legs])
    params = _params(hiplib, z, legs)
    pose[1, :, 3, 2] = np.nan
    out = hiplib.solve_seq(pose[None], params, want_diag=True, missing="skip")
    assert out["n_valid"][0].tolist() == [300, 0, 300]
    assert np.isnan(out["angles"][0, 1]).all() and np.isnan(out["fk"][0, 1]).all()
    assert (out["status"][0, 1] == MISSING).all() and (out["nfev"][0, 1] == 0).all()
    for li in (0, 2):
        ref = hiplib.solve_seq(pose[li][None, None], [params[li]], want_diag=True)
        assert np.array_equal(out["angles"][0, li], ref["angles"][0, 0])
        assert np.array_equal(out["status"][0, li], ref["status"][0, 0])


@pytest.mark.gpu
def test_generic_skip_equals_solve_of_deleted_recording(hiplib):
    from seqikpy_amd.kinematic_chain import KinematicChainGeneric
    from seqikpy_amd.leg_inverse_kinematics import LegInvKinGeneric
    from seqikpy_amd.data import BOUNDS, INITIAL_ANGLES
    z = load_golden("generic_rf_100")
    rng = np.random.default_rng(9)
    legs = ["RF", "LF"]
    gapped = {f"{l}_leg": inject_gaps(z[f"{l}_pose"], rng, frac=0.1, blocks=((40, 55),), rows=(0, 4)) for l in legs}
    ik = LegInvKinGeneric(gapped, KinematicChainGeneric(BOUNDS, legs), INITIAL_ANGLES, log_level="ERROR")
    ja, fk = ik.run_ik_and_fk(missing_key_points="skip")
    for l in legs:
        miss = np_missing(gapped[f"{l}_leg"], "generic")
        assert np.array_equal(ik.missing_frames[l], miss)
        ref_ik = LegInvKinGeneric({f"{l}_leg": gapped[f"{l}_leg"][~miss]}, KinematicChainGeneric(BOUNDS, [l]),
                                  INITIAL_ANGLES, log_level="ERROR")
        ref_ja, ref_fk = ref_ik.run_ik_and_fk()
        for k, v in ref_ja.items():
            assert np.array_equal(ja[k][~miss], v), k
            assert np.isnan(ja[k][miss]).all()
        assert np.array_equal(fk[f"{l}_leg"][~miss], ref_fk[f"{l}_leg"])


def _torch_cases():
    rng = np.random.default_rng(77)
    short = rng.normal(size=(2000, 6, 64, 5, 3))
    short[rng.random((2000, 6, 64)) < 0.05, rng.integers(0, 5), 1] = np.nan
    short[5, 2] = np.nan                     # a chain without any frame
    long = rng.normal(size=(1, 6, 200_000, 5, 3))
    long[rng.random((1, 6, 200_000)) < 0.5, 4, 2] = np.inf
    long[0, 3, 199_000:] = np.nan            # the chain ends in a gap
    return [short, long]


@pytest.mark.gpu
def test_device_building_blocks_equal_numpy(hiplib):
    import torch
    seg = [0.4, 0.6, 0.5, 0.3]
    legs = [hiplib.leg_params_from_arrays(seg, np.zeros((7, 2)), np.zeros(27))] * 6
    for pose in _torch_cases():
        S, L, N = pose.shape[:3]
        dev = torch.device("cuda:0")
        d_pose = torch.from_numpy(pose).to(dev)
        d_cpose = torch.empty_like(d_pose)
        d_map = torch.empty((S, L, N), dtype=torch.int32, device=dev)
        d_nv = torch.empty((S, L), dtype=torch.int32, device=dev)
        hiplib.gaps_compact_device(d_pose, S, L, N, legs, d_cpose, d_map, d_nv)
        cangles = torch.from_numpy(np.random.default_rng(1).normal(size=(S, L, N, 7))).to(dev)
        cstatus = torch.from_numpy(np.random.default_rng(2).integers(-1, 5, (S, L, N, 4)).astype(np.int32)).to(dev)
        angles = torch.empty_like(cangles)
        status = torch.empty_like(cstatus)
        hiplib.gaps_expand_device(d_map, S, L, N, cangles, angles, d_cstatus=cstatus, d_status=status)
        torch.cuda.synchronize()
        cp, mp, nv, ang, st = (x.cpu().numpy() for x in (d_cpose, d_map, d_nv, angles, status))
        ca, cs = cangles.cpu().numpy(), cstatus.cpu().numpy()
        for s in list(range(min(S, 40))) + [S - 1]:
            for l in range(L):
                rc, rm, rn = np_compact(pose[s, l], seg)
                assert nv[s, l] == rn and np.array_equal(mp[s, l], rm), (s, l)
                assert np.array_equal(cp[s, l], rc), (s, l)
                assert np.array_equal(ang[s, l], np_expand(rm, ca[s, l], np.nan), equal_nan=True)
                assert np.array_equal(st[s, l], np_expand(rm, cs[s, l], MISSING))
        assert np.array_equal(nv, (~np_missing(pose)).sum(axis=-1))
        # every chain of every sequence, with the vectorised form of the same construction
        rc, rm, rn = np_compact_batch(pose, seg)
        assert np.array_equal(nv, rn) and np.array_equal(mp, rm)
        assert np.array_equal(cp, rc)
        assert np.array_equal(ang, np_expand_batch(rm, ca, np.nan), equal_nan=True)
        assert np.array_equal(st, np_expand_batch(rm, cs, MISSING))


@pytest.mark.gpu
def test_solve_seq_gaps_device_equals_host_entry(hiplib):
    import torch
    cases, a, d = _anipose_df3d_cases()
    name, legs, pose = cases[1]
    params = _params(hiplib, d, legs)
    host = hiplib.solve_seq(pose[None], params, want_diag=True, missing="skip")
    dev = torch.device("cuda:0")
    S, L, N = 1, len(legs), pose.shape[1]
    t = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=dev)
    d_pose = torch.from_numpy(pose[None].copy()).to(dev)
    bufs = dict(d_angles=t((S, L, N, 7)), d_cpose=t((S, L, N, 5, 3)), d_map=t((S, L, N), torch.int32),
                d_n_valid=t((S, L), torch.int32), d_cangles=t((S, L, N, 7)), d_fk=t((S, L, N, 9, 3)),
                d_cfk=t((S, L, N, 9, 3)), d_status=t((S, L, N, 4), torch.int32), d_cstatus=t((S, L, N, 4), torch.int32),
                d_nfev=t((S, L, N, 4), torch.int32), d_cnfev=t((S, L, N, 4), torch.int32))
    hiplib.solve_seq_gaps_device(d_pose, S, L, N, params, stream=torch.cuda.current_stream(), **bufs)
    torch.cuda.synchronize()
    assert np.array_equal(bufs["d_angles"].cpu().numpy(), host["angles"], equal_nan=True)
    assert np.array_equal(bufs["d_fk"].cpu().numpy(), host["fk"], equal_nan=True)
    assert np.array_equal(bufs["d_status"].cpu().numpy(), host["status"])
    assert np.array_equal(bufs["d_nfev"].cpu().numpy(), host["nfev"])
    assert np.array_equal(bufs["d_n_valid"].cpu().numpy(), host["n_valid"])


@pytest.mark.gpu
def test_leg_inv_kin_seq_skip_dicts_and_run_fk(hiplib):
    from seqikpy_amd.kinematic_chain import KinematicChainSeq
    from seqikpy_amd.leg_inverse_kinematics import LegInvKinSeq
    from seqikpy_amd.data import BOUNDS, INITIAL_ANGLES
    z = load_golden("df3d_1000")
    rng = np.random.default_rng(12)
    legs = ["RF", "LF"]
    gapped = {f"{l}_leg": inject_gaps(z[f"{l}_pose"], rng, blocks=((100, 130),)) for l in legs}
    for fp in (False, "auto", {"chunk": 32}):
        ik = LegInvKinSeq(gapped, KinematicChainSeq(BOUNDS, legs), INITIAL_ANGLES, log_level="ERROR")
        ja, fk = ik.run_ik_and_fk(missing_key_points="skip", frame_parallel=fp, diagnostics=fp is False)
        for l in legs:
            miss = np_missing(gapped[f"{l}_leg"])
            assert np.array_equal(ik.missing_frames[l], miss)
            for k in [k for k in ja if k.startswith(f"Angle_{l}_")]:
                assert np.isnan(ja[k][miss]).all() and np.isfinite(ja[k][~miss]).all(), k
            assert np.isnan(fk[f"{l}_leg"][miss]).all() and np.isfinite(fk[f"{l}_leg"][~miss]).all()
            if fp is False:
                assert (ik.solver_status[l][miss] == MISSING).all() and (ik.solver_nfev[l][miss] == 0).all()
        again = ik.run_fk(ja)
        for k in fk:
            assert np.array_equal(again[k], fk[k], equal_nan=True), (fp, k)


@pytest.mark.gpu
def test_run_ik_and_fk_many_skip_equals_single_recordings(hiplib):
    from seqikpy_amd.batch import run_ik_and_fk_many
    from seqikpy_amd.kinematic_chain import KinematicChainSeq
    from seqikpy_amd.leg_inverse_kinematics import LegInvKinSeq
    from seqikpy_amd.data import BOUNDS, INITIAL_ANGLES
    z = load_golden("df3d_1000")
    rng = np.random.default_rng(21)
    legs = ["RF", "LF"]
    recs = [{f"{l}_leg": inject_gaps(z[f"{l}_pose"][a:a + 200], rng, blocks=((20, 40),)) for l in legs}
            for a in (0, 300)]
    many = run_ik_and_fk_many(recs, KinematicChainSeq(BOUNDS, legs), INITIAL_ANGLES, frame_parallel=False,
                              missing_key_points="skip")
    for rec, (ja, fk) in zip(recs, many):
        ik = LegInvKinSeq(rec, KinematicChainSeq(BOUNDS, legs), INITIAL_ANGLES, log_level="ERROR")
        ref_ja, ref_fk = ik.run_ik_and_fk(missing_key_points="skip", frame_parallel=False)
        for k in ref_ja:
            assert np.array_equal(ja[k], ref_ja[k], equal_nan=True), k
        for k in ref_fk:
            assert np.array_equal(fk[k], ref_fk[k], equal_nan=True), k


@pytest.mark.gpu
def test_run_body_ik_skip_legs_equal_leg_inv_kin_and_head_is_unchanged(hiplib):
    """pipeline.run_body_ik(missing_key_points="skip"): the legs are LegInvKinSeq.run_ik_and_fk(missing_key_points="skip")
    bit for bit (serial and chunked); head and antenna angles are those of the default run."""
    from seqikpy_amd.data import BOUNDS, INITIAL_ANGLES, NMF_TEMPLATE
    from seqikpy_amd.kinematic_chain import KinematicChainSeq
    from seqikpy_amd.leg_inverse_kinematics import LegInvKinSeq
    from seqikpy_amd.pipeline import run_body_ik
    z = load_golden("anipose_raw_cut")
    rng = np.random.default_rng(31)
    aligned = {k: z[f"aligned_{k}"] for k in ("R_head", "L_head", "Neck", "RF_leg", "LF_leg")}
    gapped = dict(aligned)
    for k in ("RF_leg", "LF_leg"):
        gapped[k] = inject_gaps(aligned[k], rng, blocks=((5, 12),))
    kc = KinematicChainSeq(BOUNDS, ["RF", "LF"])
    with pytest.raises(ValueError, match="Residuals are not finite"):
        run_body_ik(gapped, kc, NMF_TEMPLATE, INITIAL_ANGLES)
    head_ref, _ = run_body_ik(aligned, kc, NMF_TEMPLATE, INITIAL_ANGLES)
    for fp in (False, "auto"):
        body, fk = run_body_ik(gapped, kc, NMF_TEMPLATE, INITIAL_ANGLES, frame_parallel=fp, missing_key_points="skip")
        ik = LegInvKinSeq(gapped, kc, INITIAL_ANGLES, log_level="ERROR")
        legs, fk_ref = ik.run_ik_and_fk(missing_key_points="skip", frame_parallel=fp)
        assert ik.missing_frames["RF"].any() and ik.missing_frames["LF"].any()
        for k, v in legs.items():
            assert np.array_equal(body[k], v, equal_nan=True), (fp, k)
        for k in fk_ref:
            assert np.array_equal(fk[k], fk_ref[k], equal_nan=True), (fp, k)
        for k in head_ref:
            if not k.startswith(("Angle_RF_", "Angle_LF_")):
                assert np.array_equal(body[k], head_ref[k], equal_nan=True), k


def test_device_wrappers_check_tensors_before_enqueueing(hiplib):
    torch = pytest.importorskip("torch")
    seg = [0.4, 0.6, 0.5, 0.3]
    legs = [hiplib.leg_params_from_arrays(seg, np.zeros((7, 2)), np.zeros(27))]
    S, L, N = 1, 1, 8
    pose = torch.zeros((S, L, N, 5, 3), dtype=torch.float64)   # CPU tensor: refused before any launch
    with pytest.raises(ValueError, match="GPU tensor"):
        hiplib.gaps_compact_device(pose, S, L, N, legs, pose, 0, 0)
    with pytest.raises(ValueError, match="float64"):
        hiplib.gaps_compact_device(pose.float(), S, L, N, legs, pose, 0, 0)
    with pytest.raises(ValueError, match="int32"):
        hiplib.gaps_expand_device(torch.zeros((S, L, N), dtype=torch.int64), S, L, N, 0, 0)
    with pytest.raises(ValueError, match="elements"):
        hiplib.gaps_expand_device(torch.zeros((S, L, N + 1), dtype=torch.int32), S, L, N, 0, 0)
    with pytest.raises(ValueError, match="pair"):
        hiplib.solve_seq_gaps_device(1, S, L, N, legs, 1, 1, 1, 1, 1, d_fk=1)
