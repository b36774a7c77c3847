"""Link frames from joint angles (include/seqik_frames.h, csrc/seqik_frames.hpp / seqik_frames.hip) and the IKPy-shaped
methods of ``Chain`` / ``Link``.

CPU tier: the header and exports; the device function run on the host against the forward kinematics (bit for bit),
against the IKPy stand-in of the build (oracle/shim/ikpy, 1e-12) and its own invariants; ``Link.get_link_frame_matrix`` /
``Chain.forward_kinematics`` against the stand-in; the reference's own chains where the reference is present; argument
errors through the C ABI.  GPU tier (`-m gpu`): the kernel against the host-run rule (bit for bit), against the solvers'
FK, the device entry point, ``run_link_frames`` and ``Chain.inverse_kinematics`` / ``forward_kinematics_many``.

The bar of every comparison that is not bit for bit is 1e-12 absolute, the bar of kernel FK against host numpy in
tests/test_gpu_parity.py: positions are of order 1, a frame is a product of at most nine matrices with entries <= ~2, so
two correctly rounded evaluation orders differ by a few 1e-16 per product."""
import ctypes
import os
import pickle
import re
import sys

import numpy as np
import pytest

from angle_map_support import (_generic_params, _params, _stack, gpu_lib, guarded, made_up_batch, same_bits, switches,
                               unguarded)
from conftest import DOFS, ROOT, LegParamsC, load_golden
from harness_build import build_harness
from test_forward_kinematics import fk_harness, _lp  # noqa: F401  (fixture: the FK rule run on the host)

sys.path.insert(0, os.path.join(ROOT, "oracle"))
from ref_import import import_reference, reference_available  # noqa: E402

FRAMES_SYMBOLS = ["seqik_link_frames", "seqik_link_frames_device"]
TOL = 1e-12
SEGMENTS = ["Coxa", "Femur", "Tibia", "Tarsus"]


class FramesHarness:
    def __init__(self, so):
        self.lib = ctypes.CDLL(so)
        dp = ctypes.POINTER(ctypes.c_double)
        self.lib.harness_link_frames.restype = ctypes.c_int
        self.lib.harness_link_frames.argtypes = [dp, ctypes.c_int64, ctypes.POINTER(LegParamsC), ctypes.c_int32, dp, dp]
        self.lib.harness_link_frames_staged.restype = ctypes.c_int
        self.lib.harness_link_frames_staged.argtypes = self.lib.harness_link_frames.argtypes

    def frames(self, angles, seg, kind, origin=None, staged=False):
        """(n, 7) angles -> (n, 9, 3, 4), as the library stores them.  ``staged``: through the host re-enactment of the
        kernel's staged pass (four lanes per record) instead of the per-record rule."""
        dp = ctypes.POINTER(ctypes.c_double)
        angles = np.ascontiguousarray(angles, dtype=np.float64)
        n = angles.shape[0]
        org = None if origin is None else np.ascontiguousarray(np.broadcast_to(origin, (n, 3)), dtype=np.float64)
        out = np.full((n, 9, 3, 4), np.nan)
        lp = _lp(seg)
        fn = self.lib.harness_link_frames_staged if staged else self.lib.harness_link_frames
        rc = fn(angles.ctypes.data_as(dp), n, ctypes.byref(lp), kind, org.ctypes.data_as(dp) if org is not None else None,
                out.ctypes.data_as(dp))
        assert rc == 0
        return out


@pytest.fixture(scope="module")
def frames_harness():
    return FramesHarness(build_harness(os.path.join(ROOT, "tests", "harness", "frames_harness.hip")))


# -- the IKPy stand-in (oracle/shim/ikpy/link.py; its chain.py:25-35 is the product below) -----------------------------

def _shim_links(chain):
    sys.path.insert(0, os.path.join(ROOT, "oracle", "shim"))
    try:
        from ikpy.link import OriginLink, URDFLink
    finally:
        sys.path.pop(0)
    out = []
    for l in chain.links:
        if l.name == "Base link":
            out.append(OriginLink())
        else:
            out.append(URDFLink(name=l.name, origin_translation=l.origin_translation, origin_orientation=l.origin_orientation,
                                rotation=l.rotation, joint_type=l.joint_type, bounds=l.bounds))
    return out


def _shim_fk(links, joints):
    frame, frames = np.eye(4), []
    for link, theta in zip(links, joints):
        frame = np.dot(frame, link.get_link_frame_matrix(theta))
        frames.append(frame)
    return np.stack(frames)


def _factory(z, leg, generic=False):
    """Chain factory holding the fixture's own limits and segment lengths for `leg`."""
    from seqikpy_amd.kinematic_chain import KinematicChainGeneric, KinematicChainSeq
    bounds = {f"{leg}_{d}": tuple(z[f"{leg}_bounds"][i]) for i, d in enumerate(DOFS)}
    body = {f"{leg}_{s}": float(z[f"{leg}_seg"][i]) for i, s in enumerate(SEGMENTS)}
    return (KinematicChainGeneric if generic else KinematicChainSeq)(bounds, [leg], body)


def _angle_dict(leg, ang):
    return {f"Angle_{leg}_{d}": np.asarray(ang)[:, i] for i, d in enumerate(DOFS)}


def _made_up_angles(z, leg, n, seed):
    b = z[f"{leg}_bounds"]
    return b[:, 0] + np.random.default_rng(seed).random((n, 7)) * (b[:, 1] - b[:, 0])


# ---------------------------------------------------------------------------------------------------------------------
# CPU tier
# ---------------------------------------------------------------------------------------------------------------------

def test_frames_header_declares_exactly_the_new_entry_points(hiplib):
    text = open(os.path.join(ROOT, "include", "seqik_frames.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(seqik_[a-z_]+)\s*\(", text)))
    assert declared == sorted(FRAMES_SYMBOLS)
    assert sorted(hiplib.FRAMES_EXPORTED_SYMBOLS) == declared
    for other in (hiplib.EXPORTED_SYMBOLS, hiplib.FK_EXPORTED_SYMBOLS, hiplib.GAPS_EXPORTED_SYMBOLS,
                  hiplib.RESAMPLE_EXPORTED_SYMBOLS):
        assert not set(declared) & set(other)
    assert len(hiplib.EXPORTED_SYMBOLS) == 42
    lib = hiplib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.seqik_abi_version() == 7 == hiplib.ABI_VERSION
    assert "seqik_frames.hip" in hiplib.COMPILE_UNITS
    assert {"seqik_frames.hip", "seqik_frames.hpp"} <= set(hiplib.SOURCES)
    assert "seqik_frames" not in " ".join(hiplib.KERNEL_SOURCES)
    assert '"seqik_frames.h"' in open(os.path.join(ROOT, "setup.py")).read()


@pytest.mark.parametrize("name,kind", [("df3d_100", 0), ("df3d_1000", 0), ("generic_rf_100", 1), ("anipose_shipped", 0)])
def test_host_frames_translation_column_equals_fk_bit_for_bit(frames_harness, fk_harness, name, kind):  # noqa: F811
    z = load_golden(name)
    for leg in [str(l) for l in z["legs"]]:
        ang, seg, org = z[f"{leg}_angles"], z[f"{leg}_seg"], z[f"{leg}_pose"][:, 0]
        fr = frames_harness.frames(ang, seg, kind, origin=org)
        assert np.array_equal(fr[..., :, 3], fk_harness.fk(ang, seg, kind, origin=org)[0]), leg
        local = frames_harness.frames(ang, seg, kind)
        assert np.array_equal(local[..., :, 3], fk_harness.fk(ang, seg, kind)[0]), leg
        # the origin moves the column only
        assert np.array_equal(local[..., :3], fr[..., :3]), leg


def test_host_frames_against_the_ikpy_stand_in(frames_harness):
    """All nine 4 x 4 frames against oracle/shim/ikpy links built from our Link descriptions, leg-local.
    Largest difference seen (printed): 4.4e-16."""
    worst = 0.0
    for name, generic in (("df3d_100", False), ("anipose_shipped", False), ("generic_rf_100", True)):
        z = load_golden(name)
        for leg in [str(l) for l in z["legs"]]:
            ang = z[f"{leg}_angles"][:: max(1, len(z[f"{leg}_angles"]) // 100)]
            fr = frames_harness.frames(ang, z[f"{leg}_seg"], int(generic))
            kc = _factory(z, leg, generic)
            for t in range(len(ang)):
                if generic:
                    chain = kc.create_leg_chain(leg)
                    q = np.concatenate([[0.0], ang[t][[2, 0, 1, 3, 4, 5, 6]], [0.0]])
                else:
                    chain = kc.create_leg_chain(leg, stage=4, angles=_angle_dict(leg, ang), t=t)
                    q = np.concatenate([[0.0], ang[t], [0.0]])
                ref = _shim_fk(_shim_links(chain), q)
                worst = max(worst, np.abs(fr[t] - ref[:, :3, :]).max())
                assert (ref[:, 3] == (0, 0, 0, 1)).all()
    print(f"host rule vs IKPy stand-in: max |diff| = {worst:.3g}")
    assert worst <= TOL


@pytest.mark.parametrize("kind", [0, 1])
def test_host_frames_properties_at_volume(frames_harness, kind):
    z = load_golden("df3d_100")
    n = 200_000
    ang = _made_up_angles(z, "RF", n, 3 + kind)
    fr = frames_harness.frames(ang, z["RF_seg"], kind)
    R = fr[..., :3]
    ortho = np.abs(R @ np.swapaxes(R, -1, -2) - np.eye(3)).max()
    det = np.abs(np.linalg.det(R) - 1.0).max()
    print(f"kind {kind}: |R R^T - I| = {ortho:.3g}, |det R - 1| = {det:.3g}")
    assert ortho <= TOL and det <= TOL
    other = frames_harness.frames(ang[:1000], z["RF_seg"], 1 - kind)
    assert not np.allclose(other, fr[:1000])
    bad = ang[:100].copy()
    bad[7, 6] = np.nan
    bad[50, 0] = np.inf
    out = frames_harness.frames(bad, z["RF_seg"], kind)
    hit = np.zeros(100, bool)
    hit[[7, 50]] = True
    assert np.isnan(out[hit]).all() and np.isnan(out[hit]).sum() == 2 * 108
    assert np.array_equal(out[~hit], fr[:100][~hit])
    # the kernel's staged pass, re-enacted on the host, lays the same bits out in the same places
    org = np.random.default_rng(5).standard_normal((1600, 3))
    bad16 = np.concatenate([bad, ang[100:1600]])
    assert np.array_equal(frames_harness.frames(bad16, z["RF_seg"], kind, origin=org, staged=True),
                          frames_harness.frames(bad16, z["RF_seg"], kind, origin=org), equal_nan=True)


def _frozen_link_matrix(link, theta):
    """The arithmetic calculate_fk had before the Chain / Link methods existed, kept here to pin its bits."""
    def rot(axis, a):
        c, s = np.cos(a), np.sin(a)
        x, y, z = axis
        return np.array([[x * x + (1 - x * x) * c, x * y * (1 - c) - z * s, x * z * (1 - c) + y * s],
                         [x * y * (1 - c) + z * s, y * y + (1 - y * y) * c, y * z * (1 - c) - x * s],
                         [x * z * (1 - c) - y * s, y * z * (1 - c) + x * s, z * z + (1 - z * z) * c]])
    m = np.eye(4)
    m[:3, 3] = link.origin_translation
    r, p, y = link.origin_orientation
    m[:3, :3] = rot((0, 0, 1), y) @ rot((0, 1, 0), p) @ rot((1, 0, 0), r)
    if link.has_rotation:
        h = np.eye(4)
        h[:3, :3] = rot(tuple(link.rotation), theta)
        m = m @ h
    return m


def _all_chains(z, leg, t=3):
    ang = _angle_dict(leg, z[f"{leg}_angles"])
    kc = _factory(z, leg)
    chains = [kc.create_leg_chain(leg, stage=s, angles=ang, t=t) for s in (1, 2, 3, 4)]
    return chains + [_factory(z, leg, generic=True).create_leg_chain(leg)]


def test_link_and_chain_methods_against_the_ikpy_stand_in():
    from seqikpy_amd.leg_inverse_kinematics import LegInvKinSeq
    z = load_golden("df3d_100")
    rng = np.random.default_rng(17)
    ik = LegInvKinSeq({}, _factory(z, "RF"), log_level="ERROR")
    worst = 0.0
    for leg in ("RF", "LH"):
        for chain in _all_chains(z, leg):
            shim = _shim_links(chain)
            assert chain.active_links_mask.dtype == bool and chain.active_links_mask.all()
            assert len(chain.active_links_mask) == len(chain.links) == len(chain)
            for trial in range(20):
                q = rng.uniform(-2.0, 2.0, len(chain.links))
                if trial % 2 == 0:
                    q[0] = 0.0
                    if chain.links[-1].name.endswith("Claw"):
                        q[-1] = 0.0  # odd trials keep a non-zero claw variable: the zero-axis Rodrigues block is cos . I
                for link, sl, th in zip(chain.links, shim, q):
                    m = link.get_link_frame_matrix(th)
                    assert m.shape == (4, 4)
                    worst = max(worst, np.abs(m - sl.get_link_frame_matrix(th)).max())
                ref = _shim_fk(shim, q)
                full = chain.forward_kinematics(q, full_kinematics=True)
                assert isinstance(full, list) and len(full) == len(chain.links)
                worst = max(worst, np.abs(np.stack(full) - ref).max())
                last = chain.forward_kinematics(q)
                assert last.shape == (4, 4) and np.array_equal(last, full[-1])
                # calculate_fk on the new methods: the bits it had before
                frame, frozen = np.eye(4), np.zeros((len(chain.links), 3))
                for i, (link, th) in enumerate(zip(chain.links, q)):
                    frame = frame @ _frozen_link_matrix(link, th)
                    frozen[i] = frame[:3, 3]
                assert np.array_equal(ik.calculate_fk(chain, q), frozen)
            n = len(chain.links)
            msg = f"Your joints vector length is {n + 1} but you have {n} links"
            with pytest.raises(ValueError, match=msg):
                chain.forward_kinematics(np.zeros(n + 1))
            with pytest.raises(ValueError, match=msg):
                ik.calculate_fk(chain, np.zeros(n + 1))
    assert chain.links[0].get_link_frame_matrix(1.3).tolist() == np.eye(4).tolist()
    print(f"Link / Chain methods vs IKPy stand-in: max |diff| = {worst:.3g}")
    assert worst <= TOL


def test_chain_methods_on_a_chain_assembled_by_hand():
    from seqikpy_amd.kinematic_chain import Chain, Link, OriginLink
    links = [OriginLink(), Link("a", (0.1, 0.2, -0.5), (0.3, -0.2, 0.1), (0, 0, 1), "revolute", (-1, 1)),
             Link("b", (0, 0, -0.7), (0, 0.4, 0), None, "fixed"), Link("c", (0, 0, -0.2), (0, 0, 0), (1, 0, 0), "revolute")]
    chain = Chain("hand", links)
    q = np.array([[0.0, 0.4, 9.0, -0.3], [0.5, -0.4, 0.0, 1.3]])
    many = chain.forward_kinematics_many(q)  # no factory spec: the host loop, no library needed
    assert many.shape == (2, 4, 4, 4)
    for t in range(2):
        assert np.abs(many[t] - _shim_fk(_shim_links(chain), q[t])).max() <= TOL
    with pytest.raises(ValueError, match="Your joints vector length is 3 but you have 4 links"):
        chain.forward_kinematics_many(np.zeros((5, 3)))
    with pytest.raises(ValueError, match="calculate_ik needs a chain made by"):
        chain.inverse_kinematics(target_position=np.zeros(3))
    with pytest.raises(TypeError, match="target_orientation"):
        chain.inverse_kinematics(target_position=np.zeros(3), target_orientation=np.eye(3))
    assert chain.device == -1


@pytest.mark.skipif(not reference_available(), reason="reference checkout not present")
def test_reference_chains_over_the_stand_in_give_the_same_frames():
    """The reference's own create_leg_chain (over oracle/shim/ikpy) against ours, every leg and stage, full kinematics."""
    import_reference()
    from seqikpy.kinematic_chain import KinematicChainGeneric as RefGeneric, KinematicChainSeq as RefSeq
    from seqikpy_amd import data, utils
    from seqikpy_amd.kinematic_chain import KinematicChainGeneric, KinematicChainSeq, LEG_NAMES
    BOUNDS = data.BOUNDS_LOCOMOTION  # limits and a template that know all six legs
    body = utils.calculate_body_size(data.TEMPLATE_NMF_LOCOMOTION, LEG_NAMES)
    rng = np.random.default_rng(23)
    worst = 0.0
    for leg in LEG_NAMES:
        ang = {f"Angle_{leg}_{d}": rng.uniform(-1.5, 1.5, 4) for d in DOFS}
        pairs = [(KinematicChainSeq(BOUNDS, [leg], body).create_leg_chain(leg, stage=s, angles=ang, t=2),
                  RefSeq(BOUNDS, [leg], body).create_leg_chain(leg, stage=s, angles=ang, t=2)) for s in (1, 2, 3, 4)]
        pairs.append((KinematicChainGeneric(BOUNDS, [leg], body).create_leg_chain(leg),
                      RefGeneric(BOUNDS, [leg], body).create_leg_chain(leg)))
        for mine, ref in pairs:
            q = rng.uniform(-1.5, 1.5, len(ref.links))
            a = mine.forward_kinematics(q, full_kinematics=True)
            b = ref.forward_kinematics(q, full_kinematics=True)
            worst = max(worst, np.abs(np.stack(a) - np.stack(b)).max())
            assert np.abs(mine.forward_kinematics(q) - ref.forward_kinematics(q)).max() <= TOL
            # what the reference's two call sites touch (leg_inverse_kinematics.py:62-77)
            for attr in ("forward_kinematics", "inverse_kinematics", "links", "name", "active_links_mask"):
                assert hasattr(mine, attr), attr
            assert np.array_equal(mine.active_links_mask, ref.active_links_mask)
    print(f"reference chains vs ours: max |diff| = {worst:.3g}")
    assert worst <= TOL


def _call(lib, fn, angles, n_seq, n_legs, n_frames, legs, kind, origin, frames):
    dp = ctypes.POINTER(ctypes.c_double)
    p = lambda a: a.ctypes.data_as(dp) if a is not None else None  # noqa: E731
    if fn == "host":
        return lib.seqik_link_frames(p(angles), n_seq, n_legs, n_frames, legs, kind, p(origin), p(frames), -1)
    v = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None  # noqa: E731
    return lib.seqik_link_frames_device(v(angles), n_seq, n_legs, n_frames, legs, kind, v(origin), v(frames), None)


@pytest.mark.parametrize("fn", ["host", "device"])
def test_frames_argument_errors_through_the_c_abi(hiplib, fn):
    """Every SEQIK_ERR_BAD_ARG case with its message, before anything touches HIP; the empty call returns SEQIK_OK."""
    lib = hiplib.load()
    z = load_golden("df3d_100")
    one = hiplib.leg_params_from_arrays(z["RF_seg"], z["RF_bounds"], z["RF_seeds"])
    legs = (hiplib.SeqikLegParams * 8)(*[one] * 8)
    ang, fr, org = np.zeros((1, 1, 4, 7)), np.zeros((1, 1, 4, 9, 3, 4)), np.zeros((1, 1, 4, 3))
    bad_seg = (hiplib.SeqikLegParams * 1)(hiplib.leg_params_from_arrays(z["RF_seg"], z["RF_bounds"], z["RF_seeds"]))
    bad_seg[0].seg[2] = float("inf")
    cases = [
        (dict(n_legs=0), "n_legs must lie in 1..8"),
        (dict(n_legs=9), "n_legs must lie in 1..8"),
        (dict(n_seq=-1), "negative n_seq or n_frames"),
        (dict(n_frames=-4), "negative n_seq or n_frames"),
        (dict(angles=None), "angles and frames must not be null"),
        (dict(frames=None), "angles and frames must not be null"),
        (dict(legs=None), "legs must not be null"),
        (dict(kind=2), "kind must be 0"),
        (dict(kind=-1), "kind must be 0"),
        (dict(legs=bad_seg), "non-finite segment length"),
        (dict(n_seq=1 << 40, n_frames=1 << 20), "too many leg-frames"),
        (dict(n_seq=1 << 30, n_frames=1 << 24), "too many leg-frames"),  # fits 27 doubles per leg-frame, not 108
    ]
    for kw, msg in cases:
        a = dict(angles=ang, n_seq=1, n_legs=1, n_frames=4, legs=legs, kind=0, origin=org, frames=fr)
        a.update(kw)
        rc = _call(lib, fn, **a)
        assert rc == hiplib.ERR_ARG, (kw, rc)
        assert "seqik_link_frames: " + msg in lib.seqik_last_error().decode(), (kw, lib.seqik_last_error())
    for kw in (dict(n_seq=0), dict(n_frames=0)):
        a = dict(angles=ang, n_seq=1, n_legs=1, n_frames=4, legs=legs, kind=1, origin=None, frames=fr)
        a.update(kw)
        assert _call(lib, fn, **a) == hiplib.SEQIK_OK


def test_frames_python_argument_errors(hiplib):
    z = load_golden("df3d_100")
    lp = [hiplib.leg_params_from_arrays(z["RF_seg"], z["RF_bounds"], z["RF_seeds"])]
    ang = z["RF_angles"][None, None]
    with pytest.raises(ValueError, match="shape"):
        hiplib.link_frames(ang[0], lp)
    with pytest.raises(ValueError, match="kind"):
        hiplib.link_frames(ang, lp, kind="ikpy")
    with pytest.raises(ValueError, match="one SeqikLegParams per leg"):
        hiplib.link_frames(ang, lp * 2)
    assert hiplib.link_frames(ang[:, :, :0], lp)["frames"].shape == (1, 1, 0, 9, 4, 4)
    assert hiplib.link_frames(ang[:0], lp, rows3=True)["frames"].shape == (0, 1, 100, 9, 3, 4)


# ---------------------------------------------------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(hiplib):
    return gpu_lib(hiplib)


def _host_batch(frames_harness, ang, segs, kind, origin=None):
    """The host-run rule over a (S, L, N, 7) batch, leg by leg."""
    S, L, N = ang.shape[:3]
    out = np.empty((S, L, N, 9, 3, 4))
    for li in range(L):
        org = None if origin is None else np.ascontiguousarray(origin[:, li]).reshape(-1, 3)
        out[:, li] = frames_harness.frames(np.ascontiguousarray(ang[:, li]).reshape(-1, 7), segs[li], kind,
                                           origin=org).reshape(S, N, 9, 3, 4)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", [("df3d_100", "seq"), ("df3d_1000", "seq"), ("generic_rf_100", "generic"),
                                       ("anipose_shipped", "seq")])
def test_gpu_frames_equal_the_host_rule_bit_for_bit(lib, frames_harness, name, kind):
    z = load_golden(name)
    legs = [str(l) for l in z["legs"]]
    params, segs = _params(lib, z, legs), [z[f"{l}_seg"] for l in legs]
    ang, org = _stack(z, legs, "angles"), _stack(z, legs)[..., 0, :]
    k = lib.FK_KINDS[kind]
    for o in (org, None):
        ref = _host_batch(frames_harness, ang, segs, k, o)
        got = lib.link_frames(ang, params, kind=kind, origin=o, rows3=True)["frames"]
        assert np.array_equal(got, ref), (name, o is None)
    full = lib.link_frames(ang, params, kind=kind, origin=org)["frames"]
    assert full.shape == ang.shape[:3] + (9, 4, 4)
    assert np.array_equal(full[..., :3, :], _host_batch(frames_harness, ang, segs, k, org))
    assert (full[..., 3, :] == (0.0, 0.0, 0.0, 1.0)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["seq", "generic"])
def test_gpu_frames_equal_the_host_rule_at_config3_size_and_on_tails(lib, frames_harness, kind):
    """15 625 x 6 x 64 made-up leg-frames inside the shipped limits, NaN / inf angles included; then frame counts that
    are not a multiple of the staging tile, with the staged and the per-lane kernel."""
    from seqikpy_amd import data, utils
    legs = data.LEGS
    body = utils.calculate_body_size(data.TEMPLATE_NMF_LOCOMOTION, legs)
    params = [lib.make_leg_params(l, data.BOUNDS_LOCOMOTION, body, data.INITIAL_ANGLES_LOCOMOTION) for l in legs]
    segs = [[body[f"{l}_{s}"] for s in SEGMENTS] for l in legs]
    S, L, N = 15625, 6, 64
    rng = np.random.default_rng(31)
    lb = np.array([[data.BOUNDS_LOCOMOTION[f"{l}_{d}"][0] for d in DOFS] for l in legs])
    ub = np.array([[data.BOUNDS_LOCOMOTION[f"{l}_{d}"][1] for d in DOFS] for l in legs])
    ang = lb[None, :, None] + rng.random((S, L, N, 7)) * (ub - lb)[None, :, None]
    ang[5, 2, 40, 3] = np.nan
    ang[77, 4, 63, 0] = np.inf
    org = rng.standard_normal((S, L, N, 3))
    k = lib.FK_KINDS[kind]
    for o in (org, None):
        got = lib.link_frames(ang, params, kind=kind, origin=o, rows3=True)["frames"]
        for li in range(L):  # leg by leg: a sixth of the 5 GB reference at a time
            ref = _host_batch(frames_harness, ang[:, li:li + 1], segs[li:li + 1], k, None if o is None else o[:, li:li + 1])
            assert np.array_equal(got[:, li:li + 1], ref, equal_nan=True), (kind, o is None, li)
            del ref
        assert np.isnan(got[5, 2, 40]).all() and np.isnan(got[77, 4, 63]).all()
        assert np.isnan(got).sum() == 2 * 108
        del got
    for n in (1, 63, 65, 1000):
        a = np.ascontiguousarray(np.resize(ang[:40], (1, 6, n, 7)))
        o = np.ascontiguousarray(np.resize(org[:40], (1, 6, n, 3)))
        ref = _host_batch(frames_harness, a, segs, k, o)
        for staged in ("0", "1"):
            with switches(SEQIK_FRAMES_STAGED=staged):
                got = lib.link_frames(a, params, kind=kind, origin=o, rows3=True)["frames"]
            assert np.array_equal(got, ref, equal_nan=True), (kind, n, staged)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1])
def test_gpu_frames_block_sizes_and_a_capped_grid(lib, frames_harness, kind):
    """SEQIK_FRAMES_GRID = 3 at 2 * 3 * block + 37 leg-frames: every workgroup makes two full trips of the grid-stride loop
    and the third is ragged -- whole wavefronts, then a partial one on the per-lane path.  SEQIK_FRAMES_BLOCK 64 and 256
    with both kernels, and two sequences of three legs, whose trips straddle leg and sequence seams.  Bit for bit against
    the host-run rule, guard records around the output."""
    import torch
    runs = [(1, 1, 2 * 3 * b + 37, st, b) for st in ("0", "1") for b in (64, 256)] + [(2, 3, 71, st, 64) for st in ("0", "1")]
    for S, L, N, staged, block in runs:
        ang, segs, org = made_up_batch(S, L, N, 60 + block)
        ref = _host_batch(frames_harness, ang, segs, kind, org)
        out, p_out = guarded(S * L * N, 108)
        params = [lib.leg_params_from_arrays(s, np.zeros((7, 2)), np.zeros(27)) for s in segs]
        with switches(SEQIK_FRAMES_STAGED=staged, SEQIK_FRAMES_BLOCK=str(block), SEQIK_FRAMES_GRID="3"):
            lib.link_frames_device(torch.from_numpy(ang).cuda(), S, L, N, params, p_out, kind=kind,
                                   d_origin=torch.from_numpy(org).cuda(), stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        assert same_bits(unguarded(out, 108).reshape(ref.shape), ref), (kind, S, L, N, staged, block)


@pytest.mark.gpu
def test_gpu_frames_translation_column_equals_the_solvers_fk(lib):
    z = load_golden("df3d_1000")
    legs = [str(l) for l in z["legs"]]
    pose, params = _stack(z, legs), _params(lib, z, legs)
    for chunk in (0, -1):
        out = lib.solve_seq(pose, params, want_fk=True, frame_chunk=chunk)
        fr = lib.link_frames(out["angles"], params, kind="seq", origin=pose[..., 0, :])["frames"]
        assert np.array_equal(fr[..., :3, 3], out["fk"]), chunk
    for name in ("generic_rf_100", "df3d_100"):
        zg = load_golden(name)
        lg = [str(l) for l in zg["legs"]]
        pg, gp = _stack(zg, lg), (_params if name == "generic_rf_100" else _generic_params)(lib, zg, lg)
        gen = lib.solve_generic(pg, gp)
        fr = lib.link_frames(gen["angles"], gp, kind="generic", origin=pg[..., 0, :])["frames"]
        assert np.array_equal(fr[..., :3, 3], gen["fk"]), name
    # fused alignment: the solvers' origin is template_coxa
    from seqikpy_amd import data
    from seqikpy_amd.alignment import AlignPose
    raw = {f"{l}_leg": z[f"{l}_raw"] for l in legs}
    al = AlignPose(raw, legs, body_template=data.TEMPLATE_NMF_LOCOMOTION, log_level="ERROR")
    aff = [al.leg_affine(raw[f"{l}_leg"], l) for l in legs]
    pose_raw = np.stack([raw[f"{l}_leg"] for l in legs])[None]
    tc = np.stack([a[2] for a in aff])[None, :, None, :]
    out = lib.solve_seq(pose_raw, params, want_fk=True, affine=[lib.make_affine(*a) for a in aff])
    assert np.array_equal(lib.link_frames(out["angles"], params, origin=tc)["frames"][..., :3, 3], out["fk"])


@pytest.mark.gpu
def test_gpu_frames_device_entry_point_on_a_torch_stream(lib):
    import torch
    z = load_golden("df3d_1000")
    legs = [str(l) for l in z["legs"]]
    params = _params(lib, z, legs)
    ang, org = _stack(z, legs, "angles"), np.ascontiguousarray(_stack(z, legs)[..., 0, :])
    host = lib.link_frames(ang, params, origin=org, rows3=True)["frames"]
    d_ang, d_org = torch.from_numpy(ang).cuda(), torch.from_numpy(org).cuda()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_fr = torch.full((1, 6, 1000, 9, 3, 4), float("nan"), dtype=torch.float64, device="cuda")
        lib.link_frames_device(d_ang.data_ptr(), 1, 6, 1000, params, d_fr.data_ptr(), kind="seq",
                               d_origin=d_org.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(d_fr.cpu().numpy(), host)
    # behind the resampling on the same stream, from the buffer it wrote: no host round trip
    L, N = 6, 1000
    n_out = lib.resample_count(N, 0.01, 0.004)
    d_res = torch.empty((L, n_out, 7), dtype=torch.float64, device="cuda")
    d_out = torch.empty((L, n_out, 9, 3, 4), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    lib.resample_pchip_device(d_ang.data_ptr(), L, N, 7, 0.01, 0.004, d_res.data_ptr(), stream=stream)
    lib.link_frames_device(d_res.data_ptr(), 1, L, n_out, params, d_out.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    ref = lib.link_frames(d_res.cpu().numpy()[None], params, rows3=True)["frames"][0]
    assert np.array_equal(d_out.cpu().numpy(), ref)
    # empty input: no launch, the output is not touched
    keep = d_out.clone()
    lib.link_frames_device(d_res.data_ptr(), 1, L, 0, params, d_out.data_ptr(), stream=stream)
    lib.link_frames_device(d_res.data_ptr(), 0, L, n_out, params, d_out.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert torch.equal(keep, d_out)


@pytest.mark.gpu
def test_gpu_run_link_frames_after_run_ik_and_fk(lib, tmp_path):
    from seqikpy_amd.data import BOUNDS, INITIAL_ANGLES
    from seqikpy_amd.kinematic_chain import KinematicChainGeneric, KinematicChainSeq
    from seqikpy_amd.leg_inverse_kinematics import LegInvKinGeneric, LegInvKinSeq
    za = load_golden("anipose_shipped")
    aligned = {"RF_leg": za["RF_pose"][:500], "LF_leg": za["LF_pose"][:500]}
    ik = LegInvKinSeq(aligned, KinematicChainSeq(BOUNDS, ["RF", "LF"]), INITIAL_ANGLES, log_level="ERROR")
    ang, fk = ik.run_ik_and_fk()
    fr = ik.run_link_frames(export_path=tmp_path)
    assert list(fr) == list(fk)
    for k in fk:
        assert fr[k].shape == (500, 9, 4, 4)
        assert np.array_equal(fr[k][..., :3, 3], fk[k]), k
        R = fr[k][..., :3, :3]
        assert np.abs(R @ np.swapaxes(R, -1, -2) - np.eye(3)).max() <= TOL
    with open(tmp_path / "link_frames.pkl", "rb") as f:
        saved = pickle.load(f)
    assert all(np.array_equal(saved[k], fr[k]) for k in fr)
    local = ik.run_link_frames(dict(ang), origin=np.zeros(3))
    assert np.array_equal(local["RF_leg"][..., :3, :3], fr["RF_leg"][..., :3, :3])
    # one frame against the stage-4 chain object of the same angles
    chain = ik.kinematic_chain_class.create_leg_chain("RF", stage=4, angles=ang, t=11)
    q = np.concatenate([[0.0], [ang[f"Angle_RF_{d}"][11] for d in DOFS], [0.0]])
    assert np.abs(np.stack(chain.forward_kinematics(q, full_kinematics=True)) - local["RF_leg"][11]).max() <= TOL
    gen = LegInvKinGeneric({"RF_leg": za["RF_pose"][:100]}, KinematicChainGeneric(BOUNDS, ["RF"]), INITIAL_ANGLES,
                           log_level="ERROR")
    gang, gfk = gen.run_ik_and_fk()
    gfr = gen.run_link_frames()
    assert np.array_equal(gfr["RF_leg"][..., :3, 3], gfk["RF_leg"])
    gchain = gen.kinematic_chain_class.create_leg_chain("RF")
    q = np.concatenate([[0.0], [gang[f"Angle_RF_{d}"][5] for d in ["ThC_roll", "ThC_yaw", "ThC_pitch"] + DOFS[3:]], [0.0]])
    kind1 = np.stack(gchain.forward_kinematics(q, full_kinematics=True))
    assert np.abs(kind1[:, :3, :3] - gfr["RF_leg"][5][:, :3, :3]).max() <= TOL


@pytest.mark.gpu
def test_gpu_chain_inverse_kinematics_and_forward_kinematics_many(lib):
    from seqikpy_amd.leg_inverse_kinematics import LegInvKinGeneric, LegInvKinSeq
    z = load_golden("df3d_100")
    worst_ang = 0.0
    for leg in [str(l) for l in z["legs"]]:
        kc = _factory(z, leg)
        ik = LegInvKinSeq({}, kc, log_level="ERROR")
        pose, seeds = z[f"{leg}_pose"], z[f"{leg}_seeds"]
        seed = {1: seeds[0:4], 2: seeds[4:10], 3: seeds[10:18], 4: seeds[18:27]}
        found = {}
        for stage in (1, 2, 3, 4):
            chain = kc.create_leg_chain(leg, stage=stage, angles=found, t=0)
            target = pose[0, stage] - pose[0, 0]
            x = chain.inverse_kinematics(target_position=target, initial_position=seed[stage])
            assert x.shape == (len(chain.links),)
            assert np.array_equal(x, ik.calculate_ik(chain, target, seed[stage])), (leg, stage)
            names = [l.name for l in chain.links]
            for dof in {1: DOFS[0:2], 2: DOFS[2:4], 3: DOFS[4:6], 4: DOFS[6:7]}[stage]:
                found[f"Angle_{leg}_{dof}"] = np.array([x[names.index(f"{leg}_{dof}")]])
            # forward_kinematics_many through the GPU == the host loop
            q = np.random.default_rng(stage).uniform(-1.0, 1.0, (130, len(chain.links)))
            q[:, 0] = 0.0
            if stage == 4:
                q[:, -1] = 0.0
            gpu = chain.forward_kinematics_many(q)
            assert chain._whole_leg_angles(q) is not None
            host = np.stack([np.stack(chain.forward_kinematics(r, full_kinematics=True)) for r in q])
            assert gpu.shape == host.shape == (130, len(chain.links), 4, 4)
            assert np.abs(gpu - host).max() <= TOL, (leg, stage)
        got = np.array([found[f"Angle_{leg}_{d}"][0] for d in DOFS])
        worst_ang = max(worst_ang, np.abs(got - z[f"{leg}_angles"][0]).max())
    print(f"chain.inverse_kinematics stage by stage vs the reference's frame 0: max |diff| = {worst_ang:.3g} rad")
    assert worst_ang <= 1e-4
    # a non-zero claw variable takes the host loop and agrees with it by construction; the route is what is checked
    q4 = np.zeros((3, 9))
    q4[:, -1] = 0.2
    assert chain._whole_leg_angles(q4) is None and chain.forward_kinematics_many(q4).shape == (3, 9, 4, 4)
    # the generic chain: the same launch as calculate_ik, the claw of the reference's run
    zg = load_golden("generic_rf_100")
    gkc = _factory(zg, "RF", generic=True)
    gchain = gkc.create_leg_chain("RF")
    gik = LegInvKinGeneric({}, gkc, log_level="ERROR")
    target = zg["RF_pose"][0, 4] - zg["RF_pose"][0, 0]
    x = gchain.inverse_kinematics(target_position=target, initial_position=zg["RF_seeds"][18:27])
    assert np.array_equal(x, gik.calculate_ik(gchain, target, zg["RF_seeds"][18:27]))
    claw = gchain.forward_kinematics(x)[:3, 3] + zg["RF_pose"][0, 0]
    assert np.abs(claw - zg["RF_fk"][0, 8]).max() < 1e-6
    q = np.random.default_rng(9).uniform(-1.0, 1.0, (70, 9))
    q[:, [0, -1]] = 0.0
    host = np.stack([np.stack(gchain.forward_kinematics(r, full_kinematics=True)) for r in q])
    assert np.abs(gchain.forward_kinematics_many(q) - host).max() <= TOL
