"""Leg Jacobians, stage conditioning and key-point velocities (include/seqik_jacobian.h, csrc/seqik_jacobian.hpp /
seqik_jacobian.hip).

CPU tier: the header and exports; every SEQIK_ERR_BAD_ARG case through the C ABI without a GPU; the device rule run on
the host (tests/harness/jacobian_harness.hip): structural zeros by bits, the stage blocks of sigma, np.cross of the link
frames bit for bit, central differences of the host FK rule, origin-free FK differences, the staged re-enactment, and
the conditioning of the shipped recording.  GPU tier (`-m gpu`): the kernel against the host-run rule bit for bit over
kinds, staged / per-lane, every subset of the outputs, sizes around the wavefront and the 16-record pass, block sizes
and a capped grid, with guard records; the device entry point on a torch stream; the LegInvKin* methods.

The accuracy of the rule (a 200-bit yardstick, hard inputs, the domain rules) is tests/test_jacobian_accuracy.py."""
import ctypes
import itertools
import os
import pickle
import re
import sys

import numpy as np
import pytest

from angle_map_support import gpu_lib, same_bits, switches
from conftest import DOFS, ROOT, LegParamsC, load_golden
from harness_build import build_harness
from test_capi_symbols import assert_same_class, header_prototypes
from test_forward_kinematics import fk_harness, _lp  # noqa: F401  (fixture: the FK rule run on the host)
from test_link_frames import frames_harness  # noqa: F401  (fixture: the frames rule run on the host)

JAC_SYMBOLS = ["seqik_leg_jacobians", "seqik_leg_jacobians_device"]
KEY_LINKS = (4, 6, 7, 8)
# row k by column DOF, as include/seqik_jacobian.h prints it
PATTERN = {0: ["1100000", "1111000", "1111110", "1111111"], 1: ["1110000", "1111000", "1111110", "1111111"]}
STAGE_DOFS = [(0, 1), (2, 3), (4, 5), (6,)]
# (link, axis) of every DOF per kind, from the link order of include/seqik_frames.h
DOF_LINK = {0: [(1, 0), (2, 1), (3, 2), (4, 1), (5, 2), (6, 1), (7, 1)],
            1: [(2, 0), (3, 1), (1, 2), (4, 1), (5, 2), (6, 1), (7, 1)]}


def nonzero_mask(kind):
    return np.array([[c == "1" for c in row] for row in PATTERN[kind]])   # (4, 7)


class JacHarness:
    def __init__(self, so):
        self.lib = ctypes.CDLL(so)
        dp, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(LegParamsC)
        for name, args in (("harness_leg_jacobians", [dp, ctypes.c_int64, lp, ctypes.c_int32, dp, dp, dp, dp]),
                           ("harness_leg_jacobians_reduce_only", [dp, ctypes.c_int64, lp, ctypes.c_int32, dp, dp, dp]),
                           ("harness_leg_jacobians_staged", [dp, ctypes.c_int64, lp, ctypes.c_int32, dp])):
            getattr(self.lib, name).restype = ctypes.c_int
            getattr(self.lib, name).argtypes = args
        self.lib.harness_jacobi_sweeps.restype = ctypes.c_int

    def run(self, angles, seg, kind, qdot=None, reduce_only=False):
        """(n, 7) angles -> jac (n, 4, 3, 7), sigma (n, 8), vel (n, 4, 3) or None, as the library stores them."""
        dp = ctypes.POINTER(ctypes.c_double)
        angles = np.ascontiguousarray(angles, dtype=np.float64)
        n = angles.shape[0]
        q = None if qdot is None else np.ascontiguousarray(qdot, dtype=np.float64)
        jac, sigma = np.full((n, 4, 3, 7), 7.0), np.full((n, 8), 7.0)
        vel = None if q is None else np.full((n, 4, 3), 7.0)
        lp = _lp(seg)
        ptr = lambda a: a.ctypes.data_as(dp) if a is not None else None  # noqa: E731
        if reduce_only:
            rc = self.lib.harness_leg_jacobians_reduce_only(ptr(angles), n, ctypes.byref(lp), kind, ptr(q), ptr(sigma), ptr(vel))
            jac = None
        else:
            rc = self.lib.harness_leg_jacobians(ptr(angles), n, ctypes.byref(lp), kind, ptr(q), ptr(jac), ptr(sigma), ptr(vel))
        assert rc == 0
        return jac, sigma, vel

    def staged(self, angles, seg, kind):
        dp = ctypes.POINTER(ctypes.c_double)
        angles = np.ascontiguousarray(angles, dtype=np.float64)
        jac = np.full((angles.shape[0], 4, 3, 7), 7.0)
        lp = _lp(seg)
        assert self.lib.harness_leg_jacobians_staged(angles.ctypes.data_as(dp), angles.shape[0], ctypes.byref(lp), kind,
                                                     jac.ctypes.data_as(dp)) == 0
        return jac


@pytest.fixture(scope="module")
def jac_harness():
    return JacHarness(build_harness(os.path.join(ROOT, "tests", "harness", "jacobian_harness.hip")))


def host_batch(jh, ang, segs, kind, qdot=None):
    """The host-run rule over a (S, L, N, 7) batch, leg by leg -> jac, sigma (S, L, N, 8), vel or None."""
    S, L, N = ang.shape[:3]
    jac, sigma = np.empty((S, L, N, 4, 3, 7)), np.empty((S, L, N, 8))
    vel = None if qdot is None else np.empty((S, L, N, 4, 3))
    for li in range(L):
        q = None if qdot is None else np.ascontiguousarray(qdot[:, li]).reshape(-1, 7)
        j, s, v = jh.run(np.ascontiguousarray(ang[:, li]).reshape(-1, 7), segs[li], kind, q)
        jac[:, li], sigma[:, li] = j.reshape(S, N, 4, 3, 7), s.reshape(S, N, 8)
        if v is not None:
            vel[:, li] = v.reshape(S, N, 4, 3)
    return jac, sigma, vel


def numpy_jacobian(frames, kind):
    """a_j x (p_k - o_j) with np.cross from leg-local link frames (n, 9, 3, 4) -> (n, 4, 3, 7): every entry of a joint in
    front of or in the key point is computed; a joint behind the key point does not move it (0)."""
    n = frames.shape[0]
    jac = np.zeros((n, 4, 3, 7))
    for d, (link, axis) in enumerate(DOF_LINK[kind]):
        for k, kl in enumerate(KEY_LINKS):
            if link <= kl:
                jac[:, k, :, d] = np.cross(frames[:, link, :, axis], frames[:, kl, :, 3] - frames[:, link, :, 3])
    return jac


def made_up(seed, n, lo=-np.pi, hi=np.pi):
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, (n, 7)), rng.uniform(0.15, 1.8, 4), rng.standard_normal((n, 7))


# ---------------------------------------------------------------------------------------------------------------------
# CPU tier
# ---------------------------------------------------------------------------------------------------------------------

def test_jacobian_header_declares_exactly_the_new_entry_points(hiplib):
    text = open(os.path.join(ROOT, "include", "seqik_jacobian.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(seqik_[a-z_]+)\s*\(", text)))
    assert declared == sorted(JAC_SYMBOLS)
    assert sorted(hiplib.JACOBIAN_SIGNATURES) == ["seqik_jacobian.h"]
    assert hiplib.JACOBIAN_EXPORTED_SYMBOLS == [s[0] for s in hiplib.JACOBIAN_SIGNATURES["seqik_jacobian.h"]]
    assert sorted(hiplib.JACOBIAN_EXPORTED_SYMBOLS) == declared
    others = [s[0] for table in (hiplib.SIGNATURES, hiplib.EXTENSION_SIGNATURES, hiplib.STREAM_GAPS_SIGNATURES)
              for sigs in table.values() for s in sigs]
    assert not set(declared) & set(others)
    assert "seqik_jacobian.h" not in hiplib.SIGNATURES and "seqik_jacobian.h" not in hiplib.EXTENSION_SIGNATURES
    assert len(hiplib.EXPORTED_SYMBOLS) == 42
    lib = hiplib.load()
    assert lib.seqik_abi_version() == 7 == hiplib.ABI_VERSION
    assert "seqik_jacobian.hip" in hiplib.COMPILE_UNITS and "seqik_jacobian.hpp" in hiplib.CSRC_HEADERS
    assert "seqik_jacobian" not in " ".join(hiplib.KERNEL_SOURCES + hiplib.LATENCY_SOURCES)
    assert '"seqik_jacobian.h"' in open(os.path.join(ROOT, "setup.py")).read()
    # the table against the prototypes: count and class, and what the loaded library is bound with
    protos = header_prototypes("seqik_jacobian.h")
    table = {sig[0]: sig[1:] for sig in hiplib.JACOBIAN_SIGNATURES["seqik_jacobian.h"]}
    assert sorted(table) == sorted(protos) == declared
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name][0], list(table[name][1:])
        assert len(argtypes) == len(params) == 11, (name, params)
        assert_same_class(ret, restype, False, name)
        for p, a in zip(params, argtypes):
            assert_same_class(p, a, True, name)
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_bad_arguments_are_refused_before_anything_touches_hip(hiplib):
    """Every SEQIK_ERR_BAD_ARG case of the header, raised on a machine without a GPU, by both entry points; a call
    with no leg-frames returns OK without a launch."""
    lib = hiplib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    ang = np.zeros((1, 2, 3, 7))
    out = np.zeros((1, 2, 3, 84))
    a, o = ang.ctypes.data_as(dp), out.ctypes.data_as(dp)
    good = (hiplib.SeqikLegParams * 2)()
    for l in range(2):
        for i in range(4):
            good[l].seg[i] = 0.5
    bad_seg = (hiplib.SeqikLegParams * 2)()
    bad_seg[1].seg[2] = np.inf
    nan_seg = (hiplib.SeqikLegParams * 2)()
    nan_seg[0].seg[0] = np.nan
    huge = 2 ** 63 // (8 * 84) + 1   # leg-frames that 672 B each cannot be addressed for (27 doubles each still can)
    assert huge * 8 * 27 < 2 ** 63
    cases = [("n_legs", (a, 1, 0, 3, good, 0, None, o, None, None)), ("n_legs", (a, 1, 9, 3, good, 0, None, o, None, None)),
             ("negative", (a, -1, 2, 3, good, 0, None, o, None, None)), ("negative", (a, 1, 2, -3, good, 0, None, o, None, None)),
             ("angles", (None, 1, 2, 3, good, 0, None, o, None, None)), ("legs", (a, 1, 2, 3, None, 0, None, o, None, None)),
             ("no output", (a, 1, 2, 3, good, 0, None, None, None, None)), ("no output", (a, 1, 2, 3, good, 0, a, None, None, None)),
             ("vel needs qdot", (a, 1, 2, 3, good, 0, None, o, None, o)), ("vel needs qdot", (a, 1, 2, 3, good, 1, None, None, None, o)),
             ("kind", (a, 1, 2, 3, good, 2, None, o, None, None)), ("kind", (a, 1, 2, 3, good, -1, None, o, None, None)),
             ("segment", (a, 1, 2, 3, bad_seg, 0, None, o, None, None)), ("segment", (a, 1, 2, 3, nan_seg, 1, None, None, o, None)),
             ("too many", (a, huge, 1, 1, good, 0, None, o, None, None)), ("too many", (a, 1, 1, huge, good, 0, None, None, o, None)),
             ("too many", (a, 2 ** 40, 2, 2 ** 40, good, 0, None, o, None, None))]
    for what, args in cases:
        for fn, last in ((lib.seqik_leg_jacobians, -1), (lib.seqik_leg_jacobians_device, None)):
            assert fn(*args, last) == hiplib.ERR_ARG, (what, fn.__name__)
            msg = lib.seqik_last_error().decode()
            assert msg.startswith("seqik_leg_jacobians: ") and what.split()[0] in msg, (what, msg)
    for args in ((a, 0, 2, 3, good, 0, None, o, None, None), (a, 1, 2, 0, good, 1, a, o, o, o)):
        assert lib.seqik_leg_jacobians(*args, -1) == 0 and lib.seqik_leg_jacobians_device(*args, None) == 0
    assert not out.any()
    # the Python wrappers: shapes and arguments
    params = [hiplib.leg_params_from_arrays(np.full(4, 0.5), np.zeros((7, 2)), np.zeros(27))] * 2
    with pytest.raises(ValueError, match="no output"):
        hiplib.leg_jacobians(ang, params, want_jac=False, want_sigma=False)
    with pytest.raises(ValueError, match="qdot must have the shape"):
        hiplib.leg_jacobians(ang, params, qdot=np.zeros((1, 2, 3, 6)))
    with pytest.raises(ValueError, match="kind must be one of"):
        hiplib.leg_jacobians(ang, params, kind="stage")
    with pytest.raises(ValueError, match=r"shape \(S, L, N, 7\)"):
        hiplib.leg_jacobians(ang[0], params)


@pytest.mark.parametrize("kind", [0, 1])
def test_host_structure_zeros_blocks_and_velocities(jac_harness, frames_harness, kind):  # noqa: F811
    ang, seg, qdot = made_up(11 + kind, 200)
    jac, sigma, vel = jac_harness.run(ang, seg, kind, qdot)
    nz = nonzero_mask(kind)
    # structural zeros are +0.0 by bits; every other column was computed and is not zero at random angles (single
    # components can be: the first joint's axis is a base axis)
    assert (jac.view(np.uint64)[:, ~nz[:, None, :].repeat(3, 1)] == 0).all()
    assert (np.abs(jac).max(axis=2)[:, nz] > 1e-6).all()
    # every entry the rule computes is np.cross of the columns of the link frames it names, bit for bit
    fr = frames_harness.frames(ang, seg, kind)
    want = numpy_jacobian(fr, kind)
    full = np.broadcast_to(nz[None, :, None, :], jac.shape)
    assert same_bits(jac[full], want[full])
    # ... and what it does not compute is zero up to the rounding of the frames
    assert 0 < np.abs(want[~full]).max() < 1e-14 * seg.sum()
    # the velocities: the nonzero pattern only, DOFs ascending
    acc = np.zeros((200, 4, 3))
    for k in range(4):
        for d in range(7):
            if nz[k, d]:
                acc[:, k] = jac[:, k, :, d] * qdot[:, None, d] if d == 0 else acc[:, k] + jac[:, k, :, d] * qdot[:, None, d]
    assert same_bits(vel, acc)
    # sigma: the stage blocks are the entries the header names
    if kind == 0:
        for s, dofs in enumerate(STAGE_DOFS):
            sv = np.linalg.svd(jac[:, s][:, :, list(dofs)], compute_uv=False)
            assert np.abs(sigma[:, 2 * s] - sv[:, 0]).max() < 1e-14 * seg.sum()
            assert np.abs(sigma[:, 2 * s + 1] - sv[:, -1]).max() < 1e-14 * seg.sum()
        assert same_bits(sigma[:, 6], sigma[:, 7])
        u = jac[:, 3, :, 6]
        assert same_bits(sigma[:, 6], np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]))
    else:
        sv = np.linalg.svd(jac[:, 3], compute_uv=False)
        assert np.abs(sigma[:, :3] - sv).max() < 1e-14 * seg.sum()
        assert (np.diff(sigma[:, :3], axis=1) <= 0).all() and np.isnan(sigma[:, 3:]).all()
    # no record: the reduction alone gives the same sigma and vel; without qdot the other outputs are the same
    _, s2, v2 = jac_harness.run(ang, seg, kind, qdot, reduce_only=True)
    assert same_bits(s2, sigma) and same_bits(v2, vel)
    j3, s3, v3 = jac_harness.run(ang, seg, kind)
    assert v3 is None and same_bits(j3, jac) and same_bits(s3, sigma)
    assert jac_harness.lib.harness_jacobi_sweeps() == 6
    assert "6 sweeps" in open(os.path.join(ROOT, "include", "seqik_jacobian.h")).read()


@pytest.mark.parametrize("kind", [0, 1])
def test_host_central_differences_of_the_fk_rule_and_origin_free(jac_harness, fk_harness, kind):  # noqa: F811
    """(FK(x + h e_d) - FK(x - h e_d)) / 2h of rows 4, 6, 7, 8 at h = 1e-6 agrees with jac to 1e-7 -- with and without an
    origin added to FK: the differences are origin-free, so there is one Jacobian."""
    ang, seg, _ = made_up(23 + kind, 120)
    jac, _, _ = jac_harness.run(ang, seg, kind)
    origin = np.random.default_rng(5).standard_normal((120, 3))
    h = 1e-6
    for org in (None, origin):
        fd = np.empty_like(jac)
        for d in range(7):
            step = np.zeros(7)
            step[d] = h
            hi = fk_harness.fk(ang + step, seg, kind, origin=org)[0][:, KEY_LINKS]
            lo = fk_harness.fk(ang - step, seg, kind, origin=org)[0][:, KEY_LINKS]
            fd[..., d] = (hi - lo) / (2 * h)
        assert np.abs(fd - jac).max() <= 1e-7, (kind, org is None, np.abs(fd - jac).max())


@pytest.mark.parametrize("kind", [0, 1])
def test_host_staged_re_enactment_equals_the_per_record_rule(jac_harness, kind):
    ang, seg, _ = made_up(37 + kind, 16 * 9)
    ang[5, 2], ang[77, 6], ang[143, 0] = np.nan, 2.0 ** 31, -np.inf
    jac, _, _ = jac_harness.run(ang, seg, kind)
    assert same_bits(jac_harness.staged(ang, seg, kind), jac)
    assert np.isnan(jac[[5, 77, 143]]).all() and np.isnan(jac).sum() == 3 * 84


def _shim_frames(seg, ang, kind):
    """Leg-local frames (n, 9, 3, 4) of the IKPy stand-in (oracle/shim/ikpy), float64 numpy."""
    from test_fk_accuracy import restatement
    fam = dict(name="shim", ang=np.asarray(ang)[None], seg=np.asarray(seg)[None], pose=np.zeros((1, len(ang), 5, 3)))
    return restatement(fam, kind)[0]


def test_host_conditioning_of_the_shipped_recording(jac_harness):
    """The evidence the conditioning output was built for (EXPERIMENTS.md, "Leg Jacobians"): on the 6000 shipped frames RF
    is well conditioned throughout, and the frames of LF whose stage-2 / stage-3 sigma_min falls below 5 % of the stage
    median are the hand-masked episode around frame 290 and a second one near 3348 -- the same sets the numpy restatement
    (IKPy stand-in frames, np.cross, np.linalg.svd) gives."""
    z = load_golden("anipose_shipped")
    sig, ref = {}, {}
    for leg in ("RF", "LF"):
        ang, seg = z[f"{leg}_angles"], z[f"{leg}_seg"]
        assert ang.shape == (6000, 7)
        sig[leg] = jac_harness.run(ang, seg, 0)[1].reshape(6000, 4, 2)
        J = numpy_jacobian(_shim_frames(seg, ang, 0), 0)
        ref[leg] = np.stack([np.linalg.svd(J[:, s][:, :, list(dofs)], compute_uv=False)[:, -1]
                             for s, dofs in enumerate(STAGE_DOFS)], 1)
    assert sig["RF"][:, :, 1].min() > 0.1
    below = lambda smin: set(np.flatnonzero(smin < 0.05 * np.median(smin)).tolist())  # noqa: E731
    stage2, stage3 = set(range(280, 288)) | set(range(3347, 3351)), {297, 298, 299}
    assert below(sig["LF"][:, 1, 1]) == stage2 == below(ref["LF"][:, 1])
    assert below(sig["LF"][:, 2, 1]) == stage3 == below(ref["LF"][:, 2])
    for s in range(4):
        assert below(sig["RF"][:, s, 1]) == below(ref["RF"][:, s]) == set()
    print("\n[jacobians] shipped recording, sigma_min (smallest / median) per stage: " + "; ".join(
        f"{leg} " + " / ".join(f"{sig[leg][:, s, 1].min():.3g}" for s in range(4)) + " | " +
        " / ".join(f"{np.median(sig[leg][:, s, 1]):.3g}" for s in range(4)) for leg in ("RF", "LF")))


# ---------------------------------------------------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(hiplib):
    return gpu_lib(hiplib)


SENTINEL = -12345.678
WIDTH = dict(jac=84, sigma=8, vel=12)
SUBSETS = [c for r in (1, 2, 3) for c in itertools.combinations(("jac", "sigma", "vel"), r)]


def _segs(n_legs):
    return np.random.default_rng(3).uniform(0.15, 1.8, (8, 4))[:n_legs]


def _params_of(lib, segs):
    return [lib.leg_params_from_arrays(s, np.zeros((7, 2)), np.zeros(27)) for s in segs]


def device_run(lib, ang, qdot, segs, kind, want, env=None):
    """The device entry point on torch tensors with one guard record on each side of every output, all filled with a
    sentinel -> {name: (S, L, N, width)} of the outputs asked for; asserts that the guards and the outputs not asked for
    are untouched."""
    import torch
    S, L, N = ang.shape[:3]
    n = S * L * N
    d_ang, d_q = torch.from_numpy(np.ascontiguousarray(ang)).cuda(), torch.from_numpy(np.ascontiguousarray(qdot)).cuda()
    bufs = {k: torch.full(((n + 2) * w,), SENTINEL, dtype=torch.float64, device="cuda") for k, w in WIDTH.items()}
    ptr = {k: (bufs[k].data_ptr() + 8 * WIDTH[k] if k in want else 0) for k in WIDTH}
    with switches(**(env or {})):
        lib.leg_jacobians_device(d_ang.data_ptr(), S, L, N, _params_of(lib, segs), kind=kind, d_qdot=d_q.data_ptr(),
                                 d_jac=ptr["jac"], d_sigma=ptr["sigma"], d_vel=ptr["vel"],
                                 stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    out = {}
    for k, w in WIDTH.items():
        got = bufs[k].cpu().numpy()
        assert (got[:w] == SENTINEL).all() and (got[-w:] == SENTINEL).all(), (k, "guard", want, env)
        if k in want:
            out[k] = got[w:-w].reshape(S, L, N, w)
        else:
            assert (got == SENTINEL).all(), (k, "not requested", want, env)
    return out


def _inputs(S, L, N, seed):
    rng = np.random.default_rng(seed)
    ang = rng.uniform(-np.pi, np.pi, (S, L, N, 7))
    qdot = rng.standard_normal((S, L, N, 7))
    flat_a, flat_q = ang.reshape(-1, 7), qdot.reshape(-1, 7)
    n = flat_a.shape[0]
    if n >= 15:   # records whose neighbours in the four-lane group and the 16-record pass must keep their bits
        flat_a[n // 3, 4] = np.nan
        flat_a[n - 1, 0] = 1e300
        flat_q[n // 2, 6] = np.inf
        flat_a[7, 5] = 0.0   # a singular stage 3
    return ang, qdot


def check_against_host(lib, jh, S, L, N, kind, staged, want, seed, extra_env=None):
    ang, qdot = _inputs(S, L, N, seed)
    segs = _segs(L)
    ref = dict(zip(("jac", "sigma", "vel"), host_batch(jh, ang, segs, kind, qdot)))
    env = dict(SEQIK_JAC_STAGED=staged, **(extra_env or {}))
    got = device_run(lib, ang, qdot, segs, kind, want, env)
    for k in want:
        assert same_bits(got[k], ref[k].reshape(S, L, N, -1)), (k, (S, L, N), kind, staged, want, extra_env)


SIZES = [(1, 1, 1), (1, 1, 15), (1, 1, 16), (1, 1, 17), (1, 1, 63), (1, 1, 64), (1, 1, 65), (1, 1, 127), (1, 1, 128),
         (1, 1, 129), (1, 2, 72), (2, 3, 21)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("staged", ["0", "1"])
def test_gpu_kernel_equals_the_host_rule_bit_for_bit(lib, jac_harness, kind, staged):
    """Total leg-frames 1 .. 129, 144 and 2 x 3 x 21 (three different segment sets: wavefronts and 16-record passes
    straddle leg and sequence seams), every subset of the three outputs, guards around every buffer."""
    for i, (S, L, N) in enumerate(SIZES):
        for want in SUBSETS:
            check_against_host(lib, jac_harness, S, L, N, kind, staged, want, seed=100 + i)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1])
def test_gpu_block_sizes_and_a_capped_grid(lib, jac_harness, kind):
    """SEQIK_JAC_BLOCK 64 and 256 at sizes around the workgroup; SEQIK_JAC_GRID = 3 at 2 * 3 * 256 + 37 leg-frames, so that
    every workgroup makes more than one trip of the grid-stride loop and the last trip is ragged."""
    for block in ("64", "256"):
        for staged in ("0", "1"):
            for S, L, N in ((1, 1, 129), (2, 3, 21), (1, 3, 171)):
                check_against_host(lib, jac_harness, S, L, N, kind, staged, ("jac", "sigma", "vel"), 7,
                                   dict(SEQIK_JAC_BLOCK=block))
    n = 2 * 3 * 256 + 37
    for staged in ("0", "1"):
        for want in (("jac",), ("sigma", "vel"), ("jac", "sigma", "vel")):
            check_against_host(lib, jac_harness, 1, 1, n, kind, staged, want, 9, dict(SEQIK_JAC_GRID="3"))
        check_against_host(lib, jac_harness, 1, 1, n, kind, staged, ("jac", "vel"), 9,
                           dict(SEQIK_JAC_GRID="3", SEQIK_JAC_BLOCK="64"))


@pytest.mark.gpu
def test_gpu_device_entry_point_on_a_torch_stream_equals_the_host_entry_point(lib, jac_harness):
    import torch
    S, L, N = 2, 3, 150
    ang, qdot = _inputs(S, L, N, 55)
    segs = _segs(L)
    params = _params_of(lib, segs)
    for kind in ("seq", "generic"):
        host = lib.leg_jacobians(ang, params, kind=kind, qdot=qdot)
        k = lib.FK_KINDS[kind]
        assert host["jac"].shape == (S, L, N, 4, 3, 7) and host["vel"].shape == (S, L, N, 4, 3)
        assert host["sigma"].shape == ((S, L, N, 4, 2) if k == 0 else (S, L, N, 3))
        ref_j, ref_s, ref_v = host_batch(jac_harness, ang, segs, k, qdot)
        assert same_bits(host["jac"], ref_j) and same_bits(host["vel"], ref_v)
        assert same_bits(host["sigma"].reshape(S, L, N, -1), ref_s[..., :8 if k == 0 else 3])
        d_ang, d_q = torch.from_numpy(ang).cuda(), torch.from_numpy(qdot).cuda()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            d_j = torch.full((S, L, N, 4, 3, 7), 7.0, dtype=torch.float64, device="cuda")
            d_s = torch.full((S, L, N, 8), 7.0, dtype=torch.float64, device="cuda")
            d_v = torch.full((S, L, N, 4, 3), 7.0, dtype=torch.float64, device="cuda")
            lib.leg_jacobians_device(d_ang, S, L, N, params, kind=kind, d_qdot=d_q, d_jac=d_j, d_sigma=d_s, d_vel=d_v,
                                     stream=s)
        s.synchronize()
        assert same_bits(d_j.cpu().numpy(), ref_j) and same_bits(d_s.cpu().numpy(), ref_s)
        assert same_bits(d_v.cpu().numpy(), ref_v)
        # requests: sigma alone, and without qdot no velocities
        only = lib.leg_jacobians(ang, params, kind=kind, want_jac=False)
        assert only["jac"] is None and only["vel"] is None and same_bits(only["sigma"], host["sigma"])
        with pytest.raises(ValueError, match="expected 7200 elements"):
            lib.leg_jacobians_device(d_ang, S, L, N, params, kind=kind, d_sigma=d_v)
    # empty input: no launch, the output is not touched
    keep = d_j.clone()
    lib.leg_jacobians_device(d_ang.data_ptr(), 0, L, N, params, d_jac=d_j.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(keep.view(torch.int64), d_j.view(torch.int64))   # by bits: the records hold NaN leg-frames


def _vel_bound(jac_shape_segs, qdot):
    """K_v u S_k sum |qdot_j| of tests/test_jacobian_accuracy.py for (N, 7) rates -> (N, 4, 1)"""
    from test_jacobian_accuracy import K_V, U
    S_k = np.cumsum(np.abs(jac_shape_segs))
    return K_V * U * S_k[None, :, None] * np.abs(qdot).sum(-1)[:, None, None]


@pytest.mark.gpu
def test_gpu_leg_inv_kin_methods(lib, jac_harness, tmp_path):
    from seqikpy_amd.data import BOUNDS, INITIAL_ANGLES
    from seqikpy_amd.kinematic_chain import KinematicChainGeneric, KinematicChainSeq
    from seqikpy_amd.leg_inverse_kinematics import LegInvKinGeneric, LegInvKinSeq
    from seqikpy_amd.data import SEGMENTS
    z = load_golden("df3d_100")
    legs = ["RF", "LF"]
    ik = LegInvKinSeq({f"{l}_leg": z[f"{l}_pose"] for l in legs}, KinematicChainSeq(BOUNDS, legs), INITIAL_ANGLES,
                      log_level="ERROR")
    ja, fk = ik.run_ik_and_fk()
    jac, cond = ik.run_jacobians(export_path=tmp_path), ik.conditioning()
    kpv = ik.run_key_point_velocities(1e-2, 1e-2)
    qd = ik.run_joint_velocities(1e-2)
    assert list(jac) == list(cond) == list(kpv) == list(fk) == ["RF_leg", "LF_leg"]
    with open(tmp_path / "leg_jacobians.pkl", "rb") as f:
        saved = pickle.load(f)
    for l in legs:
        name = f"{l}_leg"
        assert jac[name].shape == (100, 4, 3, 7) and cond[name].shape == (100, 4, 2) and kpv[name].shape == (100, 4, 3)
        assert same_bits(saved[name], jac[name])
        seg = [ik.kinematic_chain_class.body_size[f"{l}_{s}"] for s in SEGMENTS]
        ang = np.stack([ja[f"Angle_{l}_{d}"] for d in DOFS], 1)
        ref_j, ref_s, _ = jac_harness.run(ang, seg, 0)
        assert same_bits(jac[name], ref_j) and same_bits(cond[name], ref_s.reshape(100, 4, 2))
        q = np.stack([qd[f"Angle_{l}_{d}"] for d in DOFS], 1)
        assert np.isfinite(kpv[name]).all()
        assert (np.abs(kpv[name] - np.einsum("nkcd,nd->nkc", jac[name], q)) <= _vel_bound(seg, q)).all()
    assert ik.run_key_point_velocities(1e-2, 4e-3)["RF_leg"].shape == (lib.resample_count(100, 1e-2, 4e-3), 4, 3)
    assert same_bits(ik.run_key_point_velocities(1e-2)["LF_leg"], kpv["LF_leg"])
    # the generic chain
    zg = load_golden("generic_rf_100")
    gen = LegInvKinGeneric({"RF_leg": zg["RF_pose"]}, KinematicChainGeneric(BOUNDS, ["RF"]), INITIAL_ANGLES, log_level="ERROR")
    gja, _ = gen.run_ik_and_fk()
    gj, gc, gv = gen.run_jacobians(), gen.conditioning(), gen.run_key_point_velocities(1e-2, 1e-2)
    n = gj["RF_leg"].shape[0]
    assert gj["RF_leg"].shape == (n, 4, 3, 7) and gc["RF_leg"].shape == (n, 3) and gv["RF_leg"].shape == (n, 4, 3)
    seg = [gen.kinematic_chain_class.body_size[f"RF_{s}"] for s in SEGMENTS]
    gang = np.stack([gja[f"Angle_RF_{d}"] for d in DOFS], 1)
    ref_j, ref_s, _ = jac_harness.run(gang, seg, 1)
    assert same_bits(gj["RF_leg"], ref_j) and same_bits(gc["RF_leg"], ref_s[:, :3])
    gq = np.stack([gen.run_joint_velocities(1e-2)[f"Angle_RF_{d}"] for d in DOFS], 1)
    assert (np.abs(gv["RF_leg"] - np.einsum("nkcd,nd->nkc", gj["RF_leg"], gq)) <= _vel_bound(seg, gq)).all()


@pytest.mark.gpu
def test_gpu_nan_rows_of_skip_mode_give_nan_records_and_clean_bits_elsewhere(lib, jac_harness):
    from seqikpy_amd.data import BOUNDS, INITIAL_ANGLES, SEGMENTS
    from seqikpy_amd.kinematic_chain import KinematicChainSeq
    from seqikpy_amd.leg_inverse_kinematics import LegInvKinSeq
    z = load_golden("df3d_100")
    pose = np.array(z["RF_pose"], dtype=np.float64, copy=True)
    hit = np.zeros(100, bool)
    hit[[3, 40, 41, 42, 64, 98]] = True
    pose[hit, 2, :] = np.nan
    ik = LegInvKinSeq({"RF_leg": pose}, KinematicChainSeq(BOUNDS, ["RF"]), INITIAL_ANGLES, log_level="ERROR")
    ja, _ = ik.run_ik_and_fk(missing_key_points="skip")
    ang = np.stack([ja[f"Angle_RF_{d}"] for d in DOFS], 1)
    assert np.array_equal(np.isnan(ang).any(1), hit)
    jac, cond = ik.run_jacobians()["RF_leg"], ik.conditioning()["RF_leg"]
    assert np.isnan(jac[hit]).all() and np.isnan(cond[hit]).all()
    seg = [ik.kinematic_chain_class.body_size[f"RF_{s}"] for s in SEGMENTS]
    ref_j, ref_s, _ = jac_harness.run(ang[~hit], seg, 0)
    assert same_bits(jac[~hit], ref_j) and same_bits(cond[~hit], ref_s.reshape(-1, 4, 2))
    with pytest.raises(ValueError, match="finite"):
        ik.run_key_point_velocities(1e-2)
    vel = ik.run_key_point_velocities(1e-2, missing="bridge", max_gap=0)["RF_leg"]
    assert np.isnan(vel[hit]).all() and np.isfinite(vel[~hit]).all()
