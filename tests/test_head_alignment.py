"""Antenna alignment on the GPU (include/seqik_head_align.h, csrc/seqik_head_align.hpp / .hip): the whole-recording
statistics of ``AlignPose.align_head`` and its per-frame map fused into the head / antenna angle kernel.

Every comparison here is equality of bits.  The yardsticks are the reference's own aligned output in
tests/golden/anipose_raw_cut.npz and numpy on the host, never the new code.

CPU tier: header and exports; the per-element rules run on the host (tests/harness/head_align_harness.hip) against
numpy; ``head_affine`` / ``align_head`` against the golden; the fused rule against the plain head rule on the golden's
aligned points; the launch plan of the head kernels; argument handling.  GPU tier (`-m gpu`): ``head_affines(on_gpu=True)`` against the host constants, the
fused kernel against ``head_angles`` on host-aligned points, ``run_body_ik`` on raw key points, the example's flag."""
import ctypes
import importlib.util
import json
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
from harness_build import build_harness

HEAD_ALIGN_SYMBOLS = ["seqik_head_align_stats_open", "seqik_head_align_stats_select", "seqik_head_align_stats_pick",
                      "seqik_head_align_stats_close", "seqik_head_angles_raw", "seqik_head_angles_raw_device"]
N_STAT_FIXTURE = {"R": 975, "L": 928}   # counted with numpy on the fixture when the feature was specified
THRESHOLD = 5e-5


class HeadAffineC(ctypes.Structure):
    _fields_ = [("origin", ctypes.c_double * 3), ("scale_base", ctypes.c_double), ("scale_tip", ctypes.c_double),
                ("template_base", ctypes.c_double * 3)]


def _affine_c(pair):
    arr = (HeadAffineC * 2)()
    for i, (origin, sb, st, tmpl) in enumerate(pair):
        for a in range(3):
            arr[i].origin[a], arr[i].template_base[a] = float(origin[a]), float(tmpl[a])
        arr[i].scale_base, arr[i].scale_tip = float(sb), float(st)
    return arr


class HeadAlignHarness:
    def __init__(self, so):
        self.lib = ctypes.CDLL(so)
        dp, vp = ctypes.POINTER(ctypes.c_double), ctypes.c_void_p
        self.lib.harness_head_align_series.restype = ctypes.c_int64
        self.lib.harness_head_align_series.argtypes = [dp, dp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                                       ctypes.c_double, dp, dp, vp]
        self.lib.harness_head_angles_raw.restype = None
        self.lib.harness_head_angles_raw.argtypes = [dp, dp, ctypes.c_int64, ctypes.c_int32, dp, ctypes.c_int64,
                                                     ctypes.c_double, ctypes.c_double, ctypes.c_int32, dp,
                                                     ctypes.POINTER(HeadAffineC), dp, dp, dp]
        self.lib.harness_head_angles_plain.restype = None
        self.lib.harness_head_angles_plain.argtypes = [dp, dp, ctypes.c_int64, ctypes.c_int32, dp, ctypes.c_int64,
                                                       ctypes.c_double, ctypes.c_double, ctypes.c_int32, dp, dp]

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if a is not None else None

    def series(self, head, thorax, threshold=THRESHOLD):
        head, thorax = (np.ascontiguousarray(a, dtype=np.float64) for a in (head, thorax))
        n = head.shape[0]
        d, ln, mask = np.full(n, np.nan), np.full(n, np.nan), np.zeros(n, dtype=np.uint8)
        count = self.lib.harness_head_align_series(self._p(head), self._p(thorax), n, head.shape[1], thorax.shape[1],
                                                   threshold, self._p(d), self._p(ln), mask.ctypes.data)
        return d, ln, mask.astype(bool), int(count)

    def angles_raw(self, r, l, neck, rest, affine, compute_ant=True, roll=None):
        r, l = (np.ascontiguousarray(a, dtype=np.float64) for a in (r, l))
        n, k = r.shape[:2]
        neck = np.ascontiguousarray(neck, dtype=np.float64).reshape(-1, 3)
        out = np.full((7 if compute_ant else 3, n), np.nan)
        ra, la = np.full((n, min(k, 2), 3), np.nan), np.full((n, min(k, 2), 3), np.nan)
        roll = None if roll is None else np.ascontiguousarray(roll, dtype=np.float64)
        self.lib.harness_head_angles_raw(self._p(r), self._p(l), n, k, self._p(neck), 3 if len(neck) == n and n > 1 else 0,
                                         rest[0], rest[1], int(compute_ant), self._p(roll), _affine_c(affine),
                                         self._p(out), self._p(ra), self._p(la))
        return out, ra, la

    def angles_plain(self, r, l, neck, rest, compute_ant=True, roll=None):
        r, l = (np.ascontiguousarray(a, dtype=np.float64) for a in (r, l))
        n, k = r.shape[:2]
        neck = np.ascontiguousarray(neck, dtype=np.float64).reshape(-1, 3)
        out = np.full((7 if compute_ant else 3, n), np.nan)
        roll = None if roll is None else np.ascontiguousarray(roll, dtype=np.float64)
        self.lib.harness_head_angles_plain(self._p(r), self._p(l), n, k, self._p(neck), 3 if len(neck) == n and n > 1 else 0,
                                           rest[0], rest[1], int(compute_ant), self._p(roll), self._p(out))
        return out


@pytest.fixture(scope="module")
def head_align_harness():
    return HeadAlignHarness(build_harness(os.path.join(ROOT, "tests", "harness", "head_align_harness.hip")))


# -- numpy restatement of what AlignPose.align_head reduces (the yardstick) ---------------------------------------------

def np_series(head, thorax, threshold=THRESHOLD):
    mid = 0.5 * (thorax[:, 0, :] + thorax[:, -1, :])
    d = np.linalg.norm(head[:, 0, :] - mid, axis=1)
    ln = np.linalg.norm(np.diff(head, axis=1), axis=2)[:, 0]
    mask = np.zeros(len(d), dtype=bool)
    mask[np.where(np.diff(np.diff(d)) < threshold)[0]] = True
    return d, ln, mask


def fixture_raw():
    z = load_golden("anipose_raw_cut")
    return z, {str(k): z[f"raw_{k}"] for k in z["segments"]}


def aligner(pose):
    from seqikpy_amd.alignment import AlignPose
    from seqikpy_amd.data import NMF_TEMPLATE
    return AlignPose(pose, legs_list=["RF", "LF"], include_claw=False, body_template=NMF_TEMPLATE, log_level="ERROR")


def rest_pitches():
    from seqikpy_amd.data import NMF_TEMPLATE
    from seqikpy_amd.head_inverse_kinematics import HeadInverseKinematics
    z = load_golden("anipose_raw_cut")
    hk = HeadInverseKinematics({k: z[f"aligned_{k}"] for k in ("R_head", "L_head", "Neck")}, NMF_TEMPLATE, log_level="ERROR")
    return hk.rest_head_pitch, hk.rest_antenna_pitch


def synthetic(n, seed, ties_at_threshold=True):
    """A recording whose antenna base moves along x over a fixed thorax at the origin, with positions that are exact
    binary fractions: d is then exact and its second difference too, so frames can be put ON the threshold (a power of
    two here) on purpose, next to frames just above and below it and seeded noise."""
    rng = np.random.default_rng(seed)
    thr = 2.0 ** -14
    thorax = np.zeros((n, 3, 3))
    steps = rng.choice([0.0, thr, 2 * thr, -thr, 0.5 * thr, 1.5 * thr, 3 * thr], size=n)
    x = 1.0 + np.cumsum(np.cumsum(steps))   # second difference of x = steps (exact: multiples of 2^-15 near 1)
    head = np.zeros((n, 2, 3))
    head[:, 0, 0] = x
    head[:, 1, :] = head[:, 0, :] + rng.uniform(0.1, 0.2, size=(n, 3))
    if not ties_at_threshold:
        head[:, 0, 1:] = rng.normal(scale=1e-3, size=(n, 2))
    return head, thorax, thr


# ======================================================= CPU tier =======================================================

def test_header_declares_and_library_exports_the_entry_points(hiplib):
    text = open(os.path.join(ROOT, "include", "seqik_head_align.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(seqik_[a-z_]+)\s*\(", text))) == sorted(HEAD_ALIGN_SYMBOLS)
    assert sorted(hiplib.HEAD_ALIGN_EXPORTED_SYMBOLS) == sorted(HEAD_ALIGN_SYMBOLS)
    lib = hiplib.load()
    for name in HEAD_ALIGN_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.seqik_abi_version() == 7 == hiplib.ABI_VERSION
    assert not set(HEAD_ALIGN_SYMBOLS) & set(hiplib.EXPORTED_SYMBOLS)
    assert ctypes.sizeof(hiplib.SeqikHeadAffine) == 64 == ctypes.sizeof(HeadAffineC)
    assert "seqik_head_align.hip" in hiplib.COMPILE_UNITS and "seqik_head_align.hpp" in hiplib.SOURCES


@pytest.mark.parametrize("side", ["R", "L"])
def test_host_run_rules_equal_numpy_on_the_fixture(head_align_harness, side):
    z, raw = fixture_raw()
    d, ln, mask, count = head_align_harness.series(raw[f"{side}_head"], raw["Thorax"])
    want_d, want_len, want_mask = np_series(raw[f"{side}_head"], raw["Thorax"])
    assert np.array_equal(d, want_d) and np.array_equal(ln, want_len)
    assert np.array_equal(mask, want_mask)
    assert count == int(want_mask.sum()) == N_STAT_FIXTURE[side]


@pytest.mark.parametrize("n", [3, 4, 5, 64, 1000])
def test_host_run_rules_equal_numpy_on_synthetic_recordings(head_align_harness, n):
    for seed in range(4):
        head, thorax, thr = synthetic(n, seed)
        want_d, want_len, want_mask = np_series(head, thorax, thr)
        d, ln, mask, count = head_align_harness.series(head, thorax, thr)
        assert np.array_equal(d, want_d) and np.array_equal(ln, want_len) and np.array_equal(mask, want_mask)
        assert count == int(want_mask.sum())
        second = np.diff(np.diff(want_d))
        assert not mask[-2:].any() and not mask[:-2][second == thr].any()   # the comparison is strict
        if n >= 64:
            assert (second == thr).any() and (second < thr).any() and (second > thr).any()
        head2, thorax2, _ = synthetic(n, seed, ties_at_threshold=False)        # irrational distances
        w = np_series(head2, thorax2)
        g = head_align_harness.series(head2, thorax2)
        assert all(np.array_equal(a, b) for a, b in zip(g[:3], w))


def test_head_affine_and_align_head_reproduce_the_reference(hiplib):
    from seqikpy_amd.alignment import AlignPose
    z, raw = fixture_raw()
    al = aligner(raw)
    consts = al.head_affines()
    assert list(consts) == ["R", "L"]
    for side in "RL":
        head = raw[f"{side}_head"]
        one = al.head_affine(head, side)
        assert all(np.array_equal(a, b) for a, b in zip(one, consts[side]))
        assert np.array_equal(AlignPose.apply_head_affine(head, one), z[f"aligned_{side}_head"]), side
        assert np.array_equal(al.align_head(head, side), z[f"aligned_{side}_head"]), side
    aligned = al.align_pose()
    for k in ("R_head", "L_head", "Neck", "RF_leg", "LF_leg"):
        assert np.array_equal(aligned[k], z[f"aligned_{k}"]), k


@pytest.mark.parametrize("n_points", [1, 2])
def test_host_run_fused_rule_equals_head_rule_on_the_reference_aligned_points(head_align_harness, n_points):
    z, raw = fixture_raw()
    consts = aligner(raw).head_affines()
    pair = (consts["R"], consts["L"])
    rest = rest_pitches()
    neck = z["aligned_Neck"][:, 0]
    r_raw, l_raw = raw["R_head"][:, :n_points], raw["L_head"][:, :n_points]
    r_al, l_al = z["aligned_R_head"][:, :n_points], z["aligned_L_head"][:, :n_points]
    ant = n_points == 2
    got, ra, la = head_align_harness.angles_raw(r_raw, l_raw, neck, rest, pair, compute_ant=ant)
    want = head_align_harness.angles_plain(r_al, l_al, neck, rest, compute_ant=ant)
    assert got.shape == want.shape == ((7 if ant else 3), 1500) and np.isfinite(want).all()
    assert np.array_equal(got, want)
    assert np.array_equal(ra, r_al) and np.array_equal(la, l_al)
    if ant:   # a supplied head roll: all seven rows again
        roll = np.linspace(-0.4, 0.4, 1500)
        got, ra, la = head_align_harness.angles_raw(r_raw, l_raw, neck, rest, pair, roll=roll)
        want = head_align_harness.angles_plain(r_al, l_al, neck, rest, roll=roll)
        assert np.array_equal(got, want) and not np.array_equal(got[3:], head_align_harness.angles_plain(r_al, l_al, neck, rest)[3:])
        assert np.array_equal(ra, r_al) and np.array_equal(la, l_al)
        per_frame_neck = np.repeat(neck, 1500, axis=0) + np.linspace(0, 1e-3, 1500)[:, None]
        got, _, _ = head_align_harness.angles_raw(r_raw, l_raw, per_frame_neck, rest, pair)
        assert np.array_equal(got, head_align_harness.angles_plain(r_al, l_al, per_frame_neck, rest))


_PLAN_CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
lib.harness_head_plan.restype = None
lib.harness_head_plan.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32] + [ctypes.c_void_p] * 5 + [
    ctypes.POINTER(ctypes.c_int64)]
out = (ctypes.c_int64 * 2)()
plans = []
for case in json.loads(sys.argv[2]):
    lib.harness_head_plan(*case, out)
    plans.append(list(out))
print(json.dumps(plans))
"""


def _head_plans(so, cases, blocks_per_cu):
    """plan_head for every case (n_frames, n_points, compute_ant, r_head, l_head, head_roll, r_aligned, l_aligned; the
    pointers as addresses, 0 = null) in a child process, because SEQIK_HEAD_BLOCKS_PER_CU is read once per process
    -> [(workgroups, variant)]."""
    env = {k: v for k, v in os.environ.items() if k != "SEQIK_HEAD_BLOCKS_PER_CU"}
    if blocks_per_cu is not None:
        env["SEQIK_HEAD_BLOCKS_PER_CU"] = str(blocks_per_cu)
    run = subprocess.run([sys.executable, "-c", _PLAN_CHILD, so, json.dumps(cases)], env=env, capture_output=True,
                         text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    return [tuple(p) for p in json.loads(run.stdout)]


def test_head_launch_plan_grid_staging_and_kernel_choice(head_align_harness):
    """The launch plan both head units share (csrc/seqik_head_launch.hpp), with the numbers each unit's own launch code
    gave before it was shared: ceil(n / 256) workgroups, at most 256 * SEQIK_HEAD_BLOCKS_PER_CU (64 when unset); the
    staged kernel only with compute_ant, two points per side and every array that takes part 16-byte aligned (an
    aligned output that is not asked for is aligned); a given roll takes the per-lane + roll kernel whatever the rest."""
    so = head_align_harness.lib._name
    GIVEN_ROLL, STAGED, PER_LANE = 0, 1, 2
    a, odd = 1 << 20, (1 << 20) + 8          # a 16-byte aligned address and one that is only 8-byte aligned
    plain = lambda n, k=2, ant=1, r=a, l=a + 4800, roll=0, ra=0, la=0: [n, k, ant, r, l, roll, ra, la]  # noqa: E731
    # the grid: one workgroup per CU at most, so that the cap of 256 is reached at 65 537 frames
    sizes = [0, 1, 256, 257, 65536, 65537, 10_000_000]
    got = _head_plans(so, [plain(n) for n in sizes], blocks_per_cu=1)
    assert [g[0] for g in got] == [0, 1, 1, 2, 256, 256, 256] and {g[1] for g in got} == {STAGED}
    # ... and the default of 64 per CU
    full = 256 * 64 * 256
    got = _head_plans(so, [plain(n) for n in (257, full - 256, full, full + 1, 6_000_000_000)], blocks_per_cu=None)
    assert [g[0] for g in got] == [2, 256 * 64 - 1, 256 * 64, 256 * 64, 256 * 64]
    # the choice of kernel
    cases = {
        "aligned, no outputs": (plain(1000), STAGED),
        "aligned, both outputs": (plain(1000, ra=a + 9600, la=a + 19200), STAGED),
        "aligned, one output": (plain(1000, la=a + 9600), STAGED),
        "head angles only": (plain(1000, ant=0), PER_LANE),
        "single-point records": (plain(1000, k=1, ant=0), PER_LANE),
        "three points per side": (plain(1000, k=3), PER_LANE),
        "r_head misaligned": (plain(1000, r=odd), PER_LANE),
        "l_head misaligned": (plain(1000, l=odd), PER_LANE),
        "r_aligned alone misaligned": (plain(1000, ra=odd, la=a + 9600), PER_LANE),
        "l_aligned alone misaligned": (plain(1000, la=odd), PER_LANE),
        "given roll, all aligned": (plain(1000, roll=a + 9600), GIVEN_ROLL),
        "given roll, outputs": (plain(1000, roll=a + 9600, ra=a + 19200, la=a + 28800), GIVEN_ROLL),
        "given roll, misaligned input": (plain(1000, roll=odd, r=odd), GIVEN_ROLL),
        "given roll, misaligned output": (plain(1000, roll=a + 9600, ra=odd), GIVEN_ROLL),
        "given roll without antenna angles": (plain(1000, ant=0, roll=a + 9600), PER_LANE),   # the roll is not read
    }
    got = _head_plans(so, [c for c, _ in cases.values()], blocks_per_cu=1)
    assert {k: g for k, g in zip(cases, got)} == {k: (4, want) for k, (_, want) in cases.items()}


def test_argument_handling(hiplib, monkeypatch):
    from seqikpy_amd.data import NMF_TEMPLATE
    from seqikpy_amd.head_inverse_kinematics import HeadInverseKinematics
    z, raw = fixture_raw()
    no_thorax = {k: v for k, v in raw.items() if k != "Thorax"}
    for on_gpu in (False, True):
        with pytest.raises(ValueError, match="Thorax"):
            aligner(no_thorax).head_affines(on_gpu=on_gpu)
        with pytest.raises(ValueError, match="at least 3 frames"):
            aligner({k: v[:2] for k, v in raw.items()}).head_affines(on_gpu=on_gpu)
    with pytest.raises(ValueError, match="Thorax"):
        aligner(no_thorax).align_head(raw["R_head"], "R")
    with pytest.raises(ValueError, match=r"threshold -1000(\.0)?"):
        aligner(raw).head_affines(threshold=-1000.0)
    with pytest.raises(ValueError, match="both R_head and L_head"):
        aligner({k: v for k, v in raw.items() if k != "L_head"}).head_affines(on_gpu=True)
    # what the GPU statistics report decides the path: non-finite input -> host path (NaN constants, as the reference);
    # nothing selected -> the ValueError that names the threshold.  (No GPU here: the report is put in the call's place.)
    al = aligner(raw)
    host = al.head_affines()
    calls = []

    def fake_stats(r, l, thorax, ranks_for, threshold, device):
        calls.append(threshold)
        return fake_stats.result
    monkeypatch.setattr(hiplib, "head_align_stats", fake_stats)
    fake_stats.result = dict(n_stat=np.array([975, 928]), n_nonfinite=3, order=None)
    got = al.head_affines(on_gpu=True)
    assert calls == [5e-5] and all(np.array_equal(a, b) for s in "RL" for a, b in zip(got[s], host[s]))
    fake_stats.result = dict(n_stat=np.array([975, 0]), n_nonfinite=0, order=None)
    with pytest.raises(ValueError, match=r"L_head.*threshold 1e-09"):
        al.head_affines(on_gpu=True, threshold=1e-9)
    monkeypatch.undo()
    # the C ABI refuses before anything touches the GPU
    lib, dp = hiplib.load(), ctypes.POINTER(ctypes.c_double)
    r = np.ascontiguousarray(raw["R_head"][:8, :1])
    out, aff = np.zeros((7, 8)), hiplib._head_affine_pair(host)
    rc = lib.seqik_head_angles_raw(r.ctypes.data_as(dp), r.ctypes.data_as(dp), 8, 1, np.zeros(3).ctypes.data_as(dp), 0, 0.0,
                                   0.0, 1, None, aff, out.ctypes.data_as(dp), None, None, None)
    assert rc == hiplib.ERR_ARG and b"two key points" in lib.seqik_last_error()
    rc = lib.seqik_head_angles_raw_device(r.ctypes.data, r.ctypes.data, 8, 1, r.ctypes.data, 0, 0.0, 0.0, 1, None, aff,
                                          out.ctypes.data, None, None, None)
    assert rc == hiplib.ERR_ARG and b"two key points" in lib.seqik_last_error()
    with pytest.raises(IndexError, match="antenna"):
        hiplib.head_angles_raw(raw["R_head"][:, :1], raw["L_head"][:, :1], np.zeros(3), 0.0, 0.0, host, compute_ant=True)
    with pytest.raises(ValueError, match="at least 3 frames"):
        hiplib.head_align_stats(raw["R_head"][:2], raw["L_head"][:2], raw["Thorax"][:2], lambda n: [0])
    with pytest.raises(ValueError, match="both sides"):
        HeadInverseKinematics.from_raw(raw, NMF_TEMPLATE, {"R": host["R"]})
    # from_raw maps the aligned points on the host when they are asked for (no GPU needed for the array helpers)
    hk = HeadInverseKinematics.from_raw(raw, NMF_TEMPLATE, host, log_level="ERROR")
    ref = HeadInverseKinematics({k: z[f"aligned_{k}"] for k in ("R_head", "L_head", "Neck")}, NMF_TEMPLATE, log_level="ERROR")
    assert "aligned_pos" not in hk.__dict__
    for side in "RL":
        assert np.array_equal(hk.get_ant_vector(side), ref.get_ant_vector(side))
        assert np.array_equal(hk.get_head_vector(side), ref.get_head_vector(side))
    assert np.array_equal(hk.head_vector_mid, ref.head_vector_mid)
    assert np.array_equal(hk.head_vector_horizontal, ref.head_vector_horizontal)
    assert all(np.array_equal(hk.aligned_pos[k], z[f"aligned_{k}"]) for k in ("R_head", "L_head", "Neck"))
    assert (hk.rest_head_pitch, hk.rest_antenna_pitch) == (ref.rest_head_pitch, ref.rest_antenna_pitch)


def test_nan_input_gives_the_reference_constants_on_the_host_path():
    """Non-finite input is the host path's business, and that path does not change: a NaN in the antenna base makes the
    constants numpy's (NaN where numpy's quantile says so)."""
    _, raw = fixture_raw()
    bad = {k: v.copy() for k, v in raw.items()}
    bad["R_head"][700, 1, 2] = np.nan      # a tip: only scale_tip of R is touched
    got, clean = aligner(bad).head_affines(), aligner(raw).head_affines()
    assert np.isnan(got["R"][2]) and np.array_equal(got["R"][0], clean["R"][0]) and got["R"][1] == clean["R"][1]
    assert all(np.array_equal(a, b) for a, b in zip(got["L"], clean["L"]))


# ======================================================= GPU tier =======================================================

def _same_constants(got, want):
    assert list(got) == list(want)
    for side in want:
        for a, b in zip(got[side], want[side]):
            assert np.array_equal(np.asarray(a), np.asarray(b)), (side, a, b)


def _np_counts(pose, threshold=THRESHOLD):
    return [int(np_series(pose[f"{s}_head"], pose["Thorax"], threshold)[2].sum()) for s in "RL"]


@pytest.mark.gpu
def test_gpu_constants_equal_host_on_the_fixture(hiplib):
    from seqikpy_amd.alignment import _quantile_ranks
    _, raw = fixture_raw()
    al = aligner(raw)
    _same_constants(al.head_affines(on_gpu=True), al.head_affines())
    res = hiplib.head_align_stats(raw["R_head"], raw["L_head"], raw["Thorax"], lambda n: _quantile_ranks(n)[0])
    assert list(res["n_stat"]) == _np_counts(raw) == [975, 928] and res["n_nonfinite"] == 0
    # the order statistics themselves, against numpy's sort
    for i, side in enumerate("RL"):
        d, ln, mask = np_series(raw[f"{side}_head"], raw["Thorax"])
        series = [raw[f"{side}_head"][mask, 0, a] for a in range(3)] + [d[mask], ln]
        for j, v in enumerate(series):
            assert np.array_equal(res["order"][i, j], np.sort(v)[_quantile_ranks(len(v))[0]]), (side, j)
    # non-finite input is counted on the device and takes the host path
    bad = {k: v.copy() for k, v in raw.items()}
    bad["L_head"][3, 0, 1] = np.nan
    bad["Thorax"][9, 2, 0] = np.inf
    res = hiplib.head_align_stats(bad["R_head"], bad["L_head"], bad["Thorax"], lambda n: [0])
    assert res["n_nonfinite"] == 3 + 2 and res["order"] is None   # frame 3: base y, d and len of L; frame 9: d of R and of L
    alb = aligner(bad)
    got, want = alb.head_affines(on_gpu=True), alb.head_affines()
    for side in "RL":
        for a, b in zip(got[side], want[side]):
            assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
    with pytest.raises(ValueError, match="threshold -1000"):
        al.head_affines(on_gpu=True, threshold=-1000.0)


@pytest.mark.gpu
@pytest.mark.parametrize("noise", [True, False])
def test_gpu_constants_equal_host_on_a_million_frames(hiplib, noise):
    """The fixture tiled to ~1 M frames: with seeded noise, and WITHOUT, so that every value is tied ~700 times over."""
    _, raw = fixture_raw()
    reps = 700
    pose = {k: np.tile(raw[k], (reps, 1, 1)) for k in ("R_head", "L_head", "Thorax")}
    if noise:
        rng = np.random.default_rng(11)
        for k in pose:
            pose[k] = pose[k] + rng.normal(scale=1e-4, size=pose[k].shape)
    al = aligner(pose)
    res = hiplib.head_align_stats(pose["R_head"], pose["L_head"], pose["Thorax"], lambda n: [0])
    assert list(res["n_stat"]) == _np_counts(pose) and min(res["n_stat"]) > 0 and res["n_nonfinite"] == 0
    _same_constants(al.head_affines(on_gpu=True), al.head_affines())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 4, 5, 63, 64, 65, 257, 1025])
def test_gpu_constants_equal_host_at_wavefront_and_tile_seams(hiplib, n):
    _, raw = fixture_raw()
    for start in (0, 311):
        pose = {k: raw[k][start:start + n] for k in ("R_head", "L_head", "Thorax")}
        counts = _np_counts(pose)
        res = hiplib.head_align_stats(pose["R_head"], pose["L_head"], pose["Thorax"], lambda m: [0, m - 1])
        assert list(res["n_stat"]) == counts, (n, start)
        al = aligner(pose)
        if min(counts) == 0:
            with pytest.raises(ValueError, match="threshold"):
                al.head_affines(on_gpu=True)
            continue
        _same_constants(al.head_affines(on_gpu=True), al.head_affines())
    # frames ON the threshold, at every position relative to the seams
    head, thorax, thr = synthetic(n, seed=n)
    head_l, _, _ = synthetic(n, seed=n + 1)
    res = hiplib.head_align_stats(head, head_l, thorax, lambda m: [0], threshold=thr)
    assert list(res["n_stat"]) == [int(np_series(h, thorax, thr)[2].sum()) for h in (head, head_l)]


@pytest.mark.gpu
def test_fused_kernel_equals_head_kernel_on_host_aligned_points(hiplib):
    import torch
    z, raw = fixture_raw()
    al = aligner(raw)
    consts = al.head_affines()
    aligned = {s: al.align_head(raw[f"{s}_head"], s) for s in "RL"}
    assert all(np.array_equal(aligned[s], z[f"aligned_{s}_head"]) for s in "RL")
    rest, neck = rest_pitches(), z["aligned_Neck"][:, 0]
    n = 1500
    roll = np.linspace(-0.4, 0.4, n)
    per_frame_neck = np.repeat(neck, n, axis=0) + np.linspace(0, 1e-3, n)[:, None]
    for kw in (dict(), dict(compute_ant=False), dict(head_roll=roll)):
        for nk in (neck, per_frame_neck):
            want = hiplib.head_angles(aligned["R"], aligned["L"], nk, *rest, **kw)
            got = hiplib.head_angles_raw(raw["R_head"], raw["L_head"], nk, *rest, consts, **kw)
            assert np.array_equal(got, want), kw
            got, ra, la = hiplib.head_angles_raw(raw["R_head"], raw["L_head"], nk, *rest, consts, want_aligned=True, **kw)
            assert np.array_equal(got, want) and np.array_equal(ra, aligned["R"]) and np.array_equal(la, aligned["L"]), kw
    # lengths around the wavefront and workgroup seams (staged and per-lane paths in one launch), single-point records
    for m in (1, 63, 64, 65, 255, 257, 1499):
        want = hiplib.head_angles(aligned["R"][:m], aligned["L"][:m], neck, *rest)
        got, ra, la = hiplib.head_angles_raw(raw["R_head"][:m], raw["L_head"][:m], neck, *rest, consts, want_aligned=True)
        assert np.array_equal(got, want) and np.array_equal(ra, aligned["R"][:m]) and np.array_equal(la, aligned["L"][:m]), m
    want = hiplib.head_angles(aligned["R"][:, :1], aligned["L"][:, :1], neck, *rest, compute_ant=False)
    got, ra, la = hiplib.head_angles_raw(raw["R_head"][:, :1], raw["L_head"][:, :1], neck, *rest, consts, compute_ant=False,
                                         want_aligned=True)
    assert np.array_equal(got, want) and np.array_equal(ra, aligned["R"][:, :1]) and np.array_equal(la, aligned["L"][:, :1])
    # the device entry point on a stream of the caller's
    stream = torch.cuda.Stream()
    d_r, d_l = (torch.from_numpy(np.ascontiguousarray(raw[k])).cuda() for k in ("R_head", "L_head"))
    d_n = torch.from_numpy(np.ascontiguousarray(neck)).cuda()
    d_ang = torch.zeros((7, n), dtype=torch.float64, device="cuda")
    d_ra, d_la = (torch.zeros((n, 2, 3), dtype=torch.float64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    want = hiplib.head_angles(aligned["R"], aligned["L"], neck, *rest)
    for use_stream in (stream, 0):
        d_ang.zero_(), d_ra.zero_(), d_la.zero_()
        torch.cuda.synchronize()
        hiplib.head_angles_raw_device(d_r, d_l, n, 2, d_n, 0, *rest, consts, d_ang, d_r_aligned=d_ra, d_l_aligned=d_la,
                                      stream=use_stream)
        torch.cuda.synchronize()
        hiplib.check_faults()
        hiplib.check_faults(stream=stream.cuda_stream)
        assert np.array_equal(d_ang.cpu().numpy(), want)
        assert np.array_equal(d_ra.cpu().numpy(), aligned["R"]) and np.array_equal(d_la.cpu().numpy(), aligned["L"])
    d_ang.zero_()
    torch.cuda.synchronize()
    hiplib.head_angles_raw_device(d_r, d_l, n, 2, d_n, 0, *rest, consts, d_ang, stream=stream)   # no aligned outputs
    stream.synchronize()
    hiplib.check_faults()
    assert np.array_equal(d_ang.cpu().numpy(), want)


@pytest.mark.gpu
def test_head_inverse_kinematics_from_raw(hiplib, tmp_path):
    from seqikpy_amd.data import NMF_TEMPLATE
    from seqikpy_amd.head_inverse_kinematics import HeadInverseKinematics
    z, raw = fixture_raw()
    consts = aligner(raw).head_affines(on_gpu=True)
    ref = HeadInverseKinematics({k: z[f"aligned_{k}"] for k in ("R_head", "L_head", "Neck")}, NMF_TEMPLATE, log_level="ERROR")
    hk = HeadInverseKinematics.from_raw(raw, NMF_TEMPLATE, consts, log_level="ERROR")
    want, got = ref.compute_head_angles(), hk.compute_head_angles(export_path=tmp_path)
    assert list(got) == list(want) and all(np.array_equal(got[k], want[k]) for k in want)
    assert os.path.exists(tmp_path / "head_joint_angles.pkl")
    assert all(np.array_equal(hk.aligned_pos[k], z[f"aligned_{k}"]) for k in ("R_head", "L_head", "Neck"))
    roll = want["Angle_head_roll"] + 0.1
    for side in "RL":
        assert np.array_equal(hk.compute_antenna_pitch(side, roll), ref.compute_antenna_pitch(side, roll))
        assert np.array_equal(hk.compute_antenna_yaw(side, roll), ref.compute_antenna_yaw(side, roll))
        assert np.array_equal(hk.get_ant_vector(side), ref.get_ant_vector(side))
    assert np.array_equal(hk.compute_head_roll(), ref.compute_head_roll())
    assert np.array_equal(hk.compute_head_pitch(), ref.compute_head_pitch())
    assert np.array_equal(hk.compute_head_yaw(), ref.compute_head_yaw())
    three = HeadInverseKinematics.from_raw(raw, NMF_TEMPLATE, consts, log_level="ERROR").compute_head_angles(compute_ant_angles=False)
    assert list(three) == list(want)[:3] and all(np.array_equal(three[k], want[k]) for k in three)


@pytest.mark.gpu
@pytest.mark.parametrize("frame_parallel", [False, None])
def test_run_body_ik_from_raw_key_points(hiplib, frame_parallel):
    from seqikpy_amd.data import BOUNDS, INITIAL_ANGLES, NMF_TEMPLATE
    from seqikpy_amd.kinematic_chain import KinematicChainSeq
    from seqikpy_amd.pipeline import run_body_ik
    z, raw = fixture_raw()
    al = aligner(raw)
    host_aligned = al.align_pose()
    assert all(np.array_equal(host_aligned[k], z[f"aligned_{k}"]) for k in host_aligned)
    kc = KinematicChainSeq(BOUNDS, ["RF", "LF"])
    want_body, want_fk = run_body_ik(host_aligned, kc, NMF_TEMPLATE, INITIAL_ANGLES, frame_parallel=frame_parallel)
    aligned_head = {}
    body, fk = run_body_ik(raw, kc, NMF_TEMPLATE, INITIAL_ANGLES, frame_parallel=frame_parallel,
                           leg_affine=al.leg_affines(on_gpu=True), head_affine=al.head_affines(on_gpu=True),
                           aligned_head=aligned_head)
    assert list(body) == list(want_body) and len(body) == 21
    for k in want_body:
        assert np.array_equal(body[k], want_body[k]), k
    assert list(fk) == list(want_fk) and all(np.array_equal(fk[k], want_fk[k]) for k in fk)
    assert all(np.array_equal(aligned_head[k], z[f"aligned_{k}"]) for k in ("R_head", "L_head", "Neck"))
    # each half on its own: raw head with host-aligned legs, raw legs with the host-aligned head
    mixed = {**host_aligned, "R_head": raw["R_head"], "L_head": raw["L_head"]}
    body, _ = run_body_ik(mixed, kc, NMF_TEMPLATE, INITIAL_ANGLES, frame_parallel=frame_parallel, head_affine=al.head_affines())
    assert all(np.array_equal(body[k], want_body[k]) for k in want_body)
    mixed = {**host_aligned, "RF_leg": raw["RF_leg"], "LF_leg": raw["LF_leg"]}
    body, fk = run_body_ik(mixed, kc, NMF_TEMPLATE, INITIAL_ANGLES, frame_parallel=frame_parallel, leg_affine=al.leg_affines())
    assert all(np.array_equal(body[k], want_body[k]) for k in want_body) and all(np.array_equal(fk[k], want_fk[k]) for k in fk)


@pytest.mark.gpu
def test_example_flag_writes_the_files_of_the_default_run(hiplib, tmp_path, monkeypatch):
    _, raw = fixture_raw()
    spec = importlib.util.spec_from_file_location("entire_pipeline", os.path.join(ROOT, "examples", "entire_pipeline.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    files = ("pose3d_aligned.pkl", "head_joint_angles.pkl", "leg_joint_angles.pkl", "forward_kinematics.pkl",
             "body_joint_angles.pkl")
    loaded = {}
    for flags in ((), ("--gpu-alignment",)):
        d = tmp_path / ("fused" if flags else "default")
        d.mkdir()
        with open(d / "converted_dict.pkl", "wb") as f:
            pickle.dump(raw, f)
        monkeypatch.setattr(sys, "argv", ["entire_pipeline.py", "-p", str(d), *flags])
        mod.main()
        loaded[flags] = {name: pickle.load(open(d / name, "rb")) for name in files}
    for name in files:
        a, b = loaded[()][name], loaded[("--gpu-alignment",)][name]
        assert list(a) == list(b), name
        for k in a:
            assert np.array_equal(a[k], b[k]), (name, k)
