"""PCHIP resampling of joint angles (include/seqik_resample.h, csrc/seqik_resample.hpp / seqik_resample.hip).

CPU tier: the header and exports, the sample count against numpy, the per-sample rules run on the host against real
scipy (default and bridge mode), shape preservation, argument handling.  GPU tier (`-m gpu`): the kernels against the
host-run rules bit for bit (both paths, both modes, the neighbour tables of long chains), the LegInvKin* / utils layer,
streams.

Tolerance against scipy (set by the issue from an independent restatement, not from this code): per series
32 * 2^-52 * max(1, max|y|), 2.1e-14 on the shipped angles.  The host-run rules reach 1.4e-15 there (EXPERIMENTS.md 9.1,
profiles/resample_parity_r09.json)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden
from harness_build import build_harness

RESAMPLE_SYMBOLS = ["seqik_resample_count", "seqik_resample_workspace_bytes", "seqik_resample_pchip",
                    "seqik_resample_pchip_device"]
BRIDGE = 1
STEP_PAIRS = [(1e-2, 1e-4, 2000), (1e-2, 1e-3, 6000), (1e-2, 3e-3, 6000), (1e-2, 2.5e-2, 6000), (1 / 100, 1 / 30, 6000)]
_dp, _ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)


def bound_of(y):
    finite = np.abs(y[np.isfinite(y)])
    return 32 * 2.0 ** -52 * max(1.0, finite.max() if finite.size else 0.0)


def grid(n, ots, nts):
    """knots j * ots and samples i * nts (what np.arange(0, total, step) holds)"""
    u = np.arange(0, n * ots, nts)
    assert np.array_equal(u, np.arange(len(u)) * nts)
    return np.arange(n) * ots, u


class ResampleHarness:
    def __init__(self, so):
        self.lib = ctypes.CDLL(so)
        i32, i64, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_double
        self.lib.harness_resample_count.restype = f64
        self.lib.harness_resample_count.argtypes = [i64, f64, f64]
        self.lib.harness_resample_chain.restype = ctypes.c_int
        self.lib.harness_resample_chain.argtypes = [_dp, i32, i32, f64, f64, i32, i32, _dp, i32, _ip, _ip]
        self.lib.harness_resample_samples.restype = None
        self.lib.harness_resample_samples.argtypes = [_dp, i32, i32, f64, f64, i32, i32, _ip, _ip, i64, i64, i64, _dp]
        self.lib.harness_resample_tables.restype = None
        self.lib.harness_resample_tables.argtypes = [_dp, i32, i32, _ip, _ip]

    def chain(self, y, ots, nts, bridge=False, max_gap=None):
        """y (N,) or (N, W) -> (n_out,) or (n_out, W)"""
        y = np.ascontiguousarray(y, dtype=np.float64)
        y2 = y[:, None] if y.ndim == 1 else y
        y2 = np.ascontiguousarray(y2)
        n, w = y2.shape
        n_out = len(np.arange(0, n * ots, nts))
        out = np.full((n_out, w), 12345.0)
        rc = self.lib.harness_resample_chain(y2.ctypes.data_as(_dp), n, w, ots, nts, BRIDGE if bridge else 0,
                                             -1 if max_gap is None else max_gap, out.ctypes.data_as(_dp), n_out, None, None)
        assert rc == 0
        return out[:, 0] if y.ndim == 1 else out

    def chains(self, y, ots, nts, bridge=False, max_gap=None):
        """(..., N, W) -> (..., n_out, W), chain by chain"""
        y = np.asarray(y, dtype=np.float64)
        flat = y.reshape((-1,) + y.shape[-2:])
        res = np.stack([self.chain(c, ots, nts, bridge, max_gap) for c in flat])
        return res.reshape(y.shape[:-2] + res.shape[-2:])

    def tables(self, y):
        y = np.ascontiguousarray(y, dtype=np.float64)
        n, w = y.shape
        prev, nxt = np.empty(n, np.int32), np.empty(n, np.int32)
        self.lib.harness_resample_tables(y.ctypes.data_as(_dp), n, w, prev.ctypes.data_as(_ip), nxt.ctypes.data_as(_ip))
        return prev, nxt

    def samples(self, y, ots, nts, first, stride, count, bridge=False, max_gap=None, tables=None):
        y = np.ascontiguousarray(y, dtype=np.float64)
        n, w = y.shape
        prev, nxt = tables if tables is not None else (self.tables(y) if bridge else (None, None))
        out = np.full((count, w), 12345.0)
        self.lib.harness_resample_samples(y.ctypes.data_as(_dp), n, w, ots, nts, BRIDGE if bridge else 0,
                                          -1 if max_gap is None else max_gap,
                                          prev.ctypes.data_as(_ip) if prev is not None else None,
                                          nxt.ctypes.data_as(_ip) if nxt is not None else None, first, stride, count,
                                          out.ctypes.data_as(_dp))
        return out


@pytest.fixture(scope="module")
def rs_harness(hiplib):
    # the product library first: it lets torch's HIP runtime load before anything else that links one (_lib.load)
    hiplib.load()
    return ResampleHarness(build_harness(os.path.join(ROOT, "tests", "harness", "resample_harness.hip")))


def shipped_angles():
    z = load_golden("anipose_shipped")
    return {leg: np.array(z[f"{leg}_angles"], dtype=np.float64) for leg in ("RF", "LF")}


def gap_mask(n, seed, first=0, last=0):
    """about 10 % of the frames and the block 300..419; first / last frames missing as asked, else kept"""
    rng = np.random.default_rng(seed)
    m = rng.random(n) < 0.1
    m[300:420] = True
    m[0] = m[-1] = False
    m[:first] = True
    if last:
        m[-last:] = True
    return m


def with_gaps(y, mask, seed):
    """whole records made NaN / +-inf (one value of the record, or all of them)"""
    rng = np.random.default_rng(seed)
    out = np.array(y, dtype=np.float64, copy=True)
    vals = np.array([np.nan, np.inf, -np.inf])
    for t in np.flatnonzero(mask):
        if out.ndim == 1 or rng.random() < 0.5:
            out[t] = vals[rng.integers(0, 3)]
        else:
            out[t, rng.integers(0, out.shape[1])] = vals[rng.integers(0, 3)]
    return out


def scipy_bridge(y, mask, ots, nts):
    """pchip_interpolate(x[valid], y[valid], u) per column, NaN outside [x_first_valid, x_last_valid + ots)"""
    from scipy.interpolate import pchip_interpolate
    x, u = grid(y.shape[0], ots, nts)
    keep = ~mask
    ref = np.stack([pchip_interpolate(x[keep], y[keep, c], u) for c in range(y.shape[1])], axis=1)
    inside = (u >= x[keep][0]) & (u < x[keep][-1] + ots)
    ref[~inside] = np.nan
    return ref, inside


# ---------------------------------------------------------------------------------------------------------------------
# CPU tier
# ---------------------------------------------------------------------------------------------------------------------

def test_resample_header_declares_exactly_the_new_entry_points(hiplib):
    text = open(os.path.join(ROOT, "include", "seqik_resample.h")).read()
    assert re.search(r"#define SEQIK_RESAMPLE_BRIDGE 1\b", text)
    assert hiplib.RESAMPLE_BRIDGE == BRIDGE
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(seqik_[a-z_]+)\s*\(", text)))
    assert declared == sorted(RESAMPLE_SYMBOLS)
    assert sorted(hiplib.RESAMPLE_EXPORTED_SYMBOLS) == declared
    for other in (hiplib.EXPORTED_SYMBOLS, hiplib.FK_EXPORTED_SYMBOLS, hiplib.GAPS_EXPORTED_SYMBOLS):
        assert not set(declared) & set(other)
    assert len(hiplib.EXPORTED_SYMBOLS) == 42
    lib = hiplib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.seqik_abi_version() == 7 == hiplib.ABI_VERSION
    assert "seqik_resample.hip" in hiplib.COMPILE_UNITS
    assert {"seqik_resample.hip", "seqik_resample.hpp"} <= set(hiplib.SOURCES)
    assert "seqik_resample.h" in open(os.path.join(ROOT, "setup.py")).read()


def test_count_equals_numpy_arange(hiplib, rs_harness):
    steps = [(1e-2, 1e-4), (1e-2, 1e-3), (1e-2, 3e-3), (1e-2, 2.5e-2), (1 / 100, 1 / 30), (1 / 30, 1e-3), (0.1, 0.03),
             (1 / 30, 1 / 30), (1e-3, 1e-2), (0.005, 0.0007), (1.0, 0.5), (2.0, 3.0)]
    for n in (2, 3, 7, 63, 64, 65, 100, 999, 1000, 1001, 4096, 6000, 100003):
        for ots, nts in steps:
            want = len(np.arange(0, n * ots, nts))
            assert hiplib.resample_count(n, ots, nts) == want, (n, ots, nts)
            assert rs_harness.lib.harness_resample_count(n, ots, nts) == want
    lib = hiplib.load()
    for n, ots, nts in ((1, 1e-2, 1e-3), (0, 1e-2, 1e-3), (10, 0.0, 1e-3), (10, 1e-2, -1.0), (10, np.nan, 1e-3),
                        (10, 1e-2, np.inf), (10, 1.0, 1e-12)):
        assert lib.seqik_resample_count(n, ots, nts) == hiplib.ERR_ARG, (n, ots, nts)
        with pytest.raises(ValueError):
            hiplib.resample_count(n, ots, nts)


@pytest.mark.parametrize("n,ots", [(3, 0.1), (1000, 1 / 30)])
def test_knot_grid_longer_than_the_series_is_refused_only_where_the_reference_refuses(hiplib, n, ots):
    from seqikpy_amd import utils
    assert len(np.arange(0, n * ots, ots)) == n + 1      # np.arange's rounding, the reference's knot grid
    y = np.linspace(0.0, 1.0, n)
    with pytest.raises(ValueError, match="equal in length"):
        utils.interpolate_signal(y, ots, ots / 10, on_gpu=True)
    with pytest.raises(ValueError, match="equal in length"):
        utils.interpolate_joint_angles({"a": y, "b": y.copy()}, original_ts=ots, new_ts=ots / 10, on_gpu=True)
    # the knots of _lib.resample_pchip are j * ots by definition: the same arguments pass its checks
    assert hiplib.resample_count(n, ots, ots / 10) == len(np.arange(0, n * ots, ots / 10))
    assert _c_call(hiplib, n_frames=n, ots=ots, nts=ots / 10, launchable=False) == "passed the checks"


@pytest.mark.parametrize("leg", ["RF", "LF"])
@pytest.mark.parametrize("width", [1, 7])
def test_host_rules_equal_scipy(rs_harness, leg, width):
    from scipy.interpolate import pchip_interpolate
    Y = shipped_angles()[leg]
    assert Y.shape == (6000, 7)
    for ots, nts, nf in STEP_PAIRS:
        y = Y[:nf]
        x, u = grid(nf, ots, nts)
        assert u[-1] > x[-1] or nts > ots                      # the tail behind the last knot is part of the comparison
        ref = np.stack([pchip_interpolate(x, y[:, c], u) for c in range(7)], axis=1)
        got = rs_harness.chain(y, ots, nts) if width == 7 else \
            np.stack([rs_harness.chain(y[:, c], ots, nts) for c in range(7)], axis=1)
        assert got.shape == ref.shape
        for c in range(7):
            err = np.abs(got[:, c] - ref[:, c]).max()
            print(f"{leg} width {width} {ots:g}->{nts:g} col {c}: max |host - scipy| = {err:.3g} (bound {bound_of(y[:, c]):.3g})")
            assert err <= bound_of(y[:, c]), (ots, nts, c, err)


@pytest.mark.parametrize("leg", ["RF", "LF"])
def test_shape_preservation(rs_harness, leg):
    Y = shipped_angles()[leg]
    for ots, nts, nf in STEP_PAIRS:
        y = Y[:nf]
        x, u = grid(nf, ots, nts)
        got = rs_harness.chain(y, ots, nts)
        front = u < x[-1]
        j = np.searchsorted(x, u[front], side="right") - 1
        lo, hi = np.minimum(y[j], y[j + 1]), np.maximum(y[j], y[j + 1])
        tol = np.array([bound_of(y[:, c]) for c in range(7)])
        assert (got[front] >= lo - tol).all() and (got[front] <= hi + tol).all(), (ots, nts)


@pytest.mark.parametrize("leg", ["RF", "LF"])
@pytest.mark.parametrize("first,last", [(0, 0), (5, 0), (0, 5)])
def test_bridge_equals_scipy_over_the_valid_knots(rs_harness, leg, first, last):
    Y = shipped_angles()[leg]
    for pi, (ots, nts, nf) in enumerate(STEP_PAIRS):
        y = Y[:nf]
        mask = gap_mask(nf, 10 + pi, first, last)
        gy = with_gaps(y, mask, 20 + pi)
        ref, inside = scipy_bridge(y, mask, ots, nts)
        got = rs_harness.chain(gy, ots, nts, bridge=True)
        assert got.shape == ref.shape
        assert np.isnan(got[~inside]).all()
        assert np.isfinite(got[inside]).all() and inside.mean() >= 0.5
        for c in range(7):
            err = np.abs(got[inside, c] - ref[inside, c]).max()
            print(f"{leg} bridge {ots:g}->{nts:g} first {first} last {last} col {c}: {err:.3g}")
            assert err <= bound_of(y[:, c]), (ots, nts, c, err)
        # width 1: every series has its own mask
        col = with_gaps(y[:, 3], mask, 30 + pi)
        got1 = rs_harness.chain(col, ots, nts, bridge=True)
        assert np.isnan(got1[~inside]).all()
        assert np.abs(got1[inside] - ref[inside, 3]).max() <= bound_of(y[:, 3])


def test_bridge_max_gap(rs_harness):
    Y = shipped_angles()["RF"]
    ots, nts = 1e-2, 1e-3
    mask = gap_mask(6000, 5)
    gy = with_gaps(Y, mask, 6)
    x, u = grid(6000, ots, nts)
    full = rs_harness.chain(gy, ots, nts, bridge=True)
    valid = np.flatnonzero(~mask)
    a = valid[np.searchsorted(valid, np.minimum(np.searchsorted(x, u, side="right") - 1, 5999), side="right") - 1]
    b_pos = np.searchsorted(valid, a, side="right")
    has_b = b_pos < valid.size
    b = valid[np.minimum(b_pos, valid.size - 1)]
    assert (b - a - 1)[has_b].max() == 120
    for max_gap in (0, 3, 119, 120):
        got = rs_harness.chain(gy, ots, nts, bridge=True, max_gap=max_gap)
        cut = has_b & (b - a - 1 > max_gap) & (u > x[a]) & (u < x[b])
        assert cut.any() == (max_gap < 120)
        assert np.isnan(got[cut]).all()
        assert np.array_equal(got[~cut], full[~cut], equal_nan=True)   # bit for bit
        assert np.isfinite(got[~cut & (u < x[valid[-1]] + ots)]).all()


def test_bridge_degenerate_chains_and_default_mode_stencil(rs_harness):
    ots, nts = 1e-2, 1e-3
    y = np.sin(np.arange(50) * 0.3)
    x, u = grid(50, ots, nts)
    none = np.full(50, np.nan)
    assert np.isnan(rs_harness.chain(none, ots, nts, bridge=True)).all()
    one = none.copy(); one[17] = 1.0
    assert np.isnan(rs_harness.chain(one, ots, nts, bridge=True)).all()
    two = none.copy(); two[10], two[30] = 1.0, 3.0
    got = rs_harness.chain(two, ots, nts, bridge=True)
    inside = (u >= x[10]) & (u < x[30] + ots)
    assert np.isnan(got[~inside]).all()
    line = 1.0 + 2.0 * (u[inside] - x[10]) / (x[30] - x[10])
    assert np.abs(got[inside] - line).max() <= 32 * 2.0 ** -52 * 3.0
    # default mode: a non-finite knot k spoils exactly the samples of intervals k-2 .. k+1 (stencil j-1 .. j+2)
    clean = rs_harness.chain(y, ots, nts)
    for k, val in ((20, np.nan), (0, np.inf), (49, -np.inf), (1, np.nan), (48, np.nan)):
        bad = y.copy(); bad[k] = val
        got = rs_harness.chain(bad, ots, nts)
        j = np.minimum(np.searchsorted(x, u, side="right") - 1, 48)
        hit = (k >= j - 1) & (k <= j + 2)
        assert np.isnan(got[hit]).all() and hit.any()
        assert np.array_equal(got[~hit], clean[~hit])
    # two knots: the straight line, continued behind the last knot
    got = rs_harness.chain(np.array([1.0, 2.0]), 1.0, 0.25)
    assert np.allclose(got, 1.0 + np.arange(8) * 0.25, rtol=0, atol=1e-15)


def _c_call(hiplib, y=1, out=1, n_chains=2, n_frames=100, width=7, ots=1e-2, nts=1e-3, flags=0, max_gap=-1, n_out=None,
            ws=1, device_entry=True, launchable=True):
    """The C entry points with made-up non-null pointers: returns the error text of a refused call.  Only calls that
    the argument checks refuse reach the library; one that would pass them (``launchable=False`` asserts that the call
    is such a one) is recognised by its arguments passing seqik_resample_count and is not made."""
    lib = hiplib.load()
    fake = ctypes.c_void_p(4096)
    cnt = lib.seqik_resample_count(n_frames, ots, nts)
    if n_out is None:
        n_out = cnt if cnt > 0 else 10
    good = (y and out and n_chains >= 0 and 1 <= width <= 16 and cnt > 0 and n_out == cnt and flags in (0, 1)
            and (ws or not flags or not device_entry))
    if good:
        assert not launchable, "a call that passes the checks must not be made with made-up pointers"
        return "passed the checks"
    assert launchable
    yp, op = (fake if y else None), (fake if out else None)
    if device_entry:
        rc = lib.seqik_resample_pchip_device(yp, n_chains, n_frames, width, ots, nts, flags, max_gap, op, n_out,
                                             fake if ws else None, None)
    else:
        rc = lib.seqik_resample_pchip(ctypes.cast(yp, _dp), n_chains, n_frames, width, ots, nts, flags, max_gap,
                                      ctypes.cast(op, _dp), n_out, -1)
    assert rc == hiplib.ERR_ARG, rc
    return lib.seqik_last_error().decode()


@pytest.mark.parametrize("device_entry", [True, False])
def test_c_entry_points_refuse_bad_arguments_before_any_launch(hiplib, device_entry):
    d = dict(device_entry=device_entry)
    assert "null" in _c_call(hiplib, y=0, **d)
    assert "null" in _c_call(hiplib, out=0, **d)
    assert "n_chains" in _c_call(hiplib, n_chains=-1, **d)
    assert "at least 2" in _c_call(hiplib, n_frames=1, **d)
    assert "2^31" in _c_call(hiplib, n_frames=2 ** 31, **d)
    for w in (0, 17, -3):
        assert "width" in _c_call(hiplib, width=w, **d)
    for ts in (0.0, -1e-2, float("nan"), float("inf")):
        assert "finite and positive" in _c_call(hiplib, ots=ts, **d)
        assert "finite and positive" in _c_call(hiplib, nts=ts, **d)
    assert "n_out" in _c_call(hiplib, n_out=999, **d)
    assert "n_out" in _c_call(hiplib, n_out=1001, **d)
    assert "flags" in _c_call(hiplib, flags=2, **d)
    assert "flags" in _c_call(hiplib, flags=-1, **d)
    if device_entry:
        assert "workspace" in _c_call(hiplib, flags=1, ws=0, **d)
    lib = hiplib.load()
    assert lib.seqik_resample_workspace_bytes(6, 1000, 0) == 0
    assert lib.seqik_resample_workspace_bytes(6, 1000, 1) == 8 * 6 * 1000
    # no chains: nothing to launch
    fake = ctypes.c_void_p(4096)
    assert lib.seqik_resample_pchip_device(fake, 0, 100, 7, 1e-2, 1e-3, 0, -1, fake, 1000, None, None) == 0


def test_python_argument_handling(hiplib):
    from seqikpy_amd import utils
    y = np.linspace(0, 1, 50)
    bad = y.copy(); bad[7] = np.nan
    with pytest.raises(ValueError, match="finite"):
        hiplib.resample_pchip(bad[:, None], 1e-2, 1e-3)
    with pytest.raises(ValueError, match="finite"):
        utils.interpolate_signal(bad, 1e-2, 1e-3, on_gpu=True)
    assert np.isnan(bad[7]) and bad[-1] == 1.0                       # on_gpu=True never repairs the caller's array
    with pytest.raises(ValueError, match="finite"):
        utils.interpolate_joint_angles({"a": y, "b": bad}, original_ts=1e-2, new_ts=1e-3, on_gpu=True)
    for kw in (dict(missing="interpolate"), dict(missing="skip"), dict(missing="fill")):
        with pytest.raises(ValueError, match="missing"):
            hiplib.resample_pchip(y[:, None], 1e-2, 1e-3, **kw)
        with pytest.raises(ValueError, match="missing"):
            utils.interpolate_signal(y, 1e-2, 1e-3, on_gpu=True, **kw)
    with pytest.raises(ValueError, match="max_gap"):
        hiplib.resample_pchip(y[:, None], 1e-2, 1e-3, max_gap=3)
    with pytest.raises(ValueError, match="max_gap"):
        hiplib.resample_pchip(y[:, None], 1e-2, 1e-3, missing="bridge", max_gap=-2)
    with pytest.raises(ValueError, match="at least 2"):
        hiplib.resample_pchip(y[:1, None], 1e-2, 1e-3)
    with pytest.raises(ValueError, match="at least 2"):
        utils.interpolate_signal(y[:1], 1e-2, 1e-3, on_gpu=True)
    with pytest.raises(ValueError, match="width"):
        hiplib.resample_pchip(np.zeros((10, 17)), 1e-2, 1e-3)
    with pytest.raises(ValueError, match="shape"):
        hiplib.resample_pchip(y, 1e-2, 1e-3)
    with pytest.raises(ValueError, match="on_gpu"):
        utils.interpolate_signal(y, 1e-2, 1e-3, missing="bridge")
    # on_gpu=False is today's path: scipy, the in-place repair included
    from scipy.interpolate import pchip_interpolate
    got = utils.interpolate_signal(y, 1.0, 0.5)
    assert np.array_equal(got, pchip_interpolate(np.arange(0, 50, 1.0), y, np.arange(0, 50, 0.5)))
    assert np.array_equal(utils.interpolate_signal(y, 1.0, 0.5, on_gpu=False), got)
    inf = y.copy(); inf[3] = np.inf
    utils.interpolate_signal(inf, 1.0, 0.5)
    assert inf[3] == 0 and inf[-1] == 0
    import inspect
    from seqikpy_amd.leg_inverse_kinematics import LegInvKinGeneric, LegInvKinSeq
    for cls in (LegInvKinSeq, LegInvKinGeneric):
        ps = inspect.signature(cls.run_resample).parameters
        assert list(ps)[:3] == ["self", "original_ts", "new_ts"]
        assert (ps["missing"].default, ps["max_gap"].default, ps["with_fk"].default) == ("error", None, False)


# ---------------------------------------------------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------------------------------------------------

def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.mark.gpu
def test_kernel_equals_host_rules_bit_for_bit(hiplib, rs_harness):
    from scipy.interpolate import pchip_interpolate
    angles = shipped_angles()
    for pi, (ots, nts, nf) in enumerate(STEP_PAIRS):
        y = np.stack([angles[leg][:nf] for leg in ("RF", "LF")])                      # (2, nf, 7)
        series = np.ascontiguousarray(y.transpose(0, 2, 1)).reshape(14, nf, 1)        # (14, nf, 1)
        for data in (y, series):
            got = hiplib.resample_pchip(data, ots, nts)
            assert _bits_equal(got, rs_harness.chains(data, ots, nts)), (ots, nts, data.shape)
        x, u = grid(nf, ots, nts)
        ref = np.stack([[pchip_interpolate(x, y[l][:, c], u) for c in range(7)] for l in range(2)]).transpose(0, 2, 1)
        assert np.abs(hiplib.resample_pchip(y, ots, nts) - ref).max() <= bound_of(y)
        for first, last in ((0, 0), (5, 0), (0, 5)):
            mask = gap_mask(nf, 10 + pi, first, last)
            gy = np.stack([with_gaps(y[l], mask, 20 + pi + l) for l in range(2)])
            gs = np.stack([with_gaps(series[k, :, 0], mask, 40 + k) for k in range(14)])[:, :, None]
            for data in (gy, gs):
                for max_gap in (None, 3):
                    got = hiplib.resample_pchip(data, ots, nts, missing="bridge", max_gap=max_gap)
                    want = rs_harness.chains(data, ots, nts, bridge=True, max_gap=max_gap)
                    assert _bits_equal(got, want), (ots, nts, data.shape, first, last, max_gap)
    # the knot grids np.arange makes one longer are no obstacle here
    for n, ots in ((3, 0.1), (1000, 1 / 30)):
        y = np.cumsum(np.random.default_rng(n).normal(size=(2, n, 3)), axis=1)
        assert _bits_equal(hiplib.resample_pchip(y, ots, ots / 10), rs_harness.chains(y, ots, ots / 10))


@pytest.mark.gpu
def test_tiling_shapes(hiplib, rs_harness):
    rng = np.random.default_rng(8)
    # sizes that are no multiples of 64, every width, up- and downsampling, n_frames from 2 on
    for n, w, ots, nts in ((2, 1, 1.0, 0.3), (3, 16, 1e-2, 1e-3), (65, 7, 1e-2, 7e-4), (127, 2, 1e-2, 1.3e-2),
                           (1001, 5, 1 / 30, 1e-3), (777, 7, 1e-2, 1e-2), (4099, 3, 1e-3, 0.1), (130, 11, 1e-2, 1e-4)):
        y = np.cumsum(rng.normal(size=(3, n, w)), axis=1)
        assert _bits_equal(hiplib.resample_pchip(y, ots, nts), rs_harness.chains(y, ots, nts)), (n, w)
        gy = y.copy()
        gy[rng.random((3, n)) < 0.2, rng.integers(0, w)] = np.nan
        got = hiplib.resample_pchip(gy, ots, nts, missing="bridge")
        assert _bits_equal(got, rs_harness.chains(gy, ots, nts, bridge=True)), (n, w)
    # many short chains
    y = np.cumsum(rng.normal(size=(15625, 6, 64, 7)), axis=2) * 0.1
    got = hiplib.resample_pchip(y, 1e-2, 1e-3)
    assert got.shape == (15625, 6, 640, 7)
    pick = rng.choice(15625, 40, replace=False)
    assert _bits_equal(got[pick], rs_harness.chains(y[pick], 1e-2, 1e-3))
    assert np.isfinite(got).all()
    # downsampling by 100: 64 samples span 6400 knots, the direct-load path
    y = np.cumsum(rng.normal(size=(2, 200000, 7)), axis=1) * 0.01
    assert _bits_equal(hiplib.resample_pchip(y, 1e-4, 1e-2), rs_harness.chains(y, 1e-4, 1e-2))
    gy = y.copy()
    gy[:, 50000:90000] = np.nan
    gy[rng.random((2, 200000)) < 0.05] = np.inf
    assert _bits_equal(hiplib.resample_pchip(gy, 1e-4, 1e-2, missing="bridge", max_gap=1000),
                       rs_harness.chains(gy, 1e-4, 1e-2, bridge=True, max_gap=1000))


@pytest.mark.gpu
def test_million_frame_chains_with_a_long_gap(hiplib, rs_harness):
    """6 chains of 1 M frames, ratio 10, 5 % missing and a gap of 100 000 frames: the neighbour tables (several table
    tiles per chain) against the host, a strided sample of 1e6 outputs and every output around the gap."""
    import torch
    rng = np.random.default_rng(99)
    C, N, W = 6, 1_000_000, 7
    ots, nts = 1e-2, 1e-3
    y = np.cumsum(rng.normal(size=(C, N, W)) * 0.01, axis=1)
    y[rng.random((C, N)) < 0.05] = np.nan
    y[:, 400_000:500_000] = np.nan
    y[0, :70_000] = np.nan          # a chain whose first table tiles hold no valid knot
    y[1, -70_000:] = np.nan         # ... and one whose last tiles hold none
    y[2] = np.nan                   # ... and one without any
    d_y = torch.from_numpy(y).cuda()
    n_out = hiplib.resample_count(N, ots, nts)
    d_out = torch.empty((C, n_out, W), dtype=torch.float64, device="cuda")
    assert hiplib.resample_workspace_bytes(C, N, "bridge") == 8 * C * N
    d_ws = torch.empty((2, C, N), dtype=torch.int32, device="cuda")
    hiplib.resample_pchip_device(d_y, C, N, W, ots, nts, d_out, missing="bridge", d_workspace=d_ws)
    torch.cuda.synchronize()
    ws = d_ws.cpu().numpy()
    stride = (C * n_out) // 1_000_000
    for c in range(C):
        tables = rs_harness.tables(y[c])
        assert np.array_equal(ws[0, c], tables[0]) and np.array_equal(ws[1, c], tables[1]), c
        count = (n_out + stride - 1) // stride
        want = rs_harness.samples(y[c], ots, nts, 0, stride, count, bridge=True, tables=tables)
        assert _bits_equal(d_out[c, ::stride].cpu().numpy(), want), c
        lo, hi = 3_990_000, 5_010_000
        want = rs_harness.samples(y[c], ots, nts, lo, 1, hi - lo, bridge=True, tables=tables)
        got = d_out[c, lo:hi].cpu().numpy()
        assert _bits_equal(got, want), c
        if c != 2:
            assert np.isfinite(got).all()       # the gap is bridged
    assert torch.isnan(d_out[2]).all()


@pytest.mark.gpu
def test_skip_mode_angles_bridge_and_feed_forward_kinematics(hiplib, rs_harness):
    from seqikpy_amd.data import BOUNDS, INITIAL_ANGLES
    from seqikpy_amd.kinematic_chain import KinematicChainSeq
    from seqikpy_amd.leg_inverse_kinematics import LegInvKinSeq
    from conftest import DOFS
    z = load_golden("df3d_1000")
    rng = np.random.default_rng(12)
    legs = ["RF", "LF"]
    gapped = {}
    for l in legs:
        p = np.array(z[f"{l}_pose"], dtype=np.float64, copy=True)
        hit = rng.random(1000) < 0.05
        hit[100:130] = True
        hit[0] = hit[-1] = False
        p[hit, rng.integers(1, 5), :] = np.nan
        gapped[f"{l}_leg"] = p
    ik = LegInvKinSeq(gapped, KinematicChainSeq(BOUNDS, legs), INITIAL_ANGLES, log_level="ERROR")
    ja, _ = ik.run_ik_and_fk(missing_key_points="skip")
    assert all(ik.missing_frames[l].sum() >= 30 for l in legs)
    with pytest.raises(ValueError, match="finite"):
        ik.run_resample(1e-2, 1e-3)
    res = ik.run_resample(1e-2, 1e-3, missing="bridge")
    origin = np.array([0.1, -0.2, 0.3])
    res2, fk = ik.run_resample(1e-2, 1e-3, missing="bridge", with_fk=True, origin=origin)
    assert list(fk) == [f"{l}_leg" for l in legs]
    for l in legs:
        ang = np.stack([ja[f"Angle_{l}_{d}"] for d in DOFS], axis=1)
        want = rs_harness.chain(ang, 1e-2, 1e-3, bridge=True)
        got = np.stack([res[f"Angle_{l}_{d}"] for d in DOFS], axis=1)
        assert _bits_equal(got, want), l
        assert _bits_equal(np.stack([res2[f"Angle_{l}_{d}"] for d in DOFS], axis=1), want), l
        assert np.isfinite(got[:9991]).all() and got.shape == (10000, 7)   # frames 0 and 999 were solved
        ref_fk = hiplib.forward_kinematics(got[None, None], [ik._fk_leg_params(l)], kind="seq",
                                           origin=origin)["fk"][0, 0]
        assert _bits_equal(fk[f"{l}_leg"], ref_fk), l
    # the default origin: key point 0, when it does not move
    kp0 = {l: z[f"{l}_pose"][:, 0] for l in legs}
    if all((kp0[l] == kp0[l][0]).all() for l in legs):
        _, fk0 = ik.run_resample(1e-2, 1e-3, missing="bridge", with_fk=True)
        assert np.array_equal(fk0["RF_leg"][0, 0], kp0["RF"][0])
    else:
        with pytest.raises(ValueError, match="origin"):
            ik.run_resample(1e-2, 1e-3, missing="bridge", with_fk=True)


@pytest.mark.gpu
def test_interpolate_joint_angles_on_gpu_equals_the_host_path(hiplib):
    from seqikpy_amd import utils
    from conftest import DOFS
    angles = shipped_angles()
    series = {f"Angle_{leg}_{d}": angles[leg][:, i].copy() for leg in ("RF", "LF") for i, d in enumerate(DOFS)}
    assert len(series) == 14
    keep = {k: v.copy() for k, v in series.items()}
    host = utils.interpolate_joint_angles(series, original_ts=1e-2, new_ts=1e-3)
    gpu = utils.interpolate_joint_angles(series, original_ts=1e-2, new_ts=1e-3, on_gpu=True)
    assert list(gpu) == list(host)
    for k in host:
        assert gpu[k].shape == host[k].shape == (60000,)
        assert np.abs(gpu[k] - host[k]).max() <= bound_of(series[k]), k
        assert np.array_equal(series[k], keep[k])
    one = utils.interpolate_signal(series["Angle_RF_ThC_yaw"], 1e-2, 1e-3, on_gpu=True)
    assert np.array_equal(one, gpu["Angle_RF_ThC_yaw"])
    gappy = {k: v.copy() for k, v in series.items()}
    gappy["Angle_LF_FTi_pitch"][100:140] = np.nan
    out = utils.interpolate_joint_angles(gappy, original_ts=1e-2, new_ts=1e-3, on_gpu=True, missing="bridge", max_gap=50)
    assert np.isfinite(out["Angle_LF_FTi_pitch"]).all()
    assert np.array_equal(out["Angle_RF_ThC_yaw"], gpu["Angle_RF_ThC_yaw"])


@pytest.mark.gpu
def test_device_entry_point_only_enqueues(hiplib, rs_harness):
    import torch
    rng = np.random.default_rng(4)
    C, N, W = 6, 5000, 7
    ys = [np.cumsum(rng.normal(size=(C, N, W)) * 0.05, axis=1) for _ in range(2)]
    for y in ys:
        y[rng.random((C, N)) < 0.05] = np.nan
    want = [rs_harness.chains(y, 1e-2, 1e-3, bridge=True) for y in ys]
    n_out = hiplib.resample_count(N, 1e-2, 1e-3)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_y = [torch.from_numpy(y).cuda() for y in ys]
    d_out = [torch.full((C, n_out, W), 7.0, dtype=torch.float64, device="cuda") for _ in ys]
    d_ws = [torch.empty((2, C, N), dtype=torch.int32, device="cuda") for _ in ys]
    torch.cuda.synchronize()
    for k in range(2):
        hiplib.resample_pchip_device(d_y[k], C, N, W, 1e-2, 1e-3, d_out[k], missing="bridge", d_workspace=d_ws[k],
                                     stream=streams[k])
    for s in streams:
        s.synchronize()
    for k in range(2):
        assert _bits_equal(d_out[k].cpu().numpy(), want[k]), k
    # default mode on a non-default stream, raw pointers, no workspace
    fin = np.nan_to_num(ys[0], nan=0.5)
    d_f = torch.from_numpy(fin).cuda()
    torch.cuda.synchronize()
    hiplib.resample_pchip_device(d_f.data_ptr(), C, N, W, 1e-2, 1e-3, d_out[0].data_ptr(), stream=streams[1].cuda_stream)
    streams[1].synchronize()
    assert _bits_equal(d_out[0].cpu().numpy(), rs_harness.chains(fin, 1e-2, 1e-3))
    with pytest.raises(ValueError, match="elements"):
        hiplib.resample_pchip_device(d_f, C, N, W, 1e-2, 1e-3, d_out[0][:, :-1])
