"""PCHIP resampling against a 200-bit yardstick, on inputs that reach every branch of the rules, and the GPU paths the
other tests leave out.

tests/test_resample.py compares the per-sample rules of csrc/seqik_resample.hpp (run on the host) and the kernels of
csrc/seqik_resample.hip with scipy on one data set, the shipped joint angles, at a flat per-series bound.  scipy is a
float64 program itself, and smooth angles below pi reach few of the branches of ``pchip_interior`` / ``pchip_edge``.  Here
the rules -- on the host (CPU tier) and as kernels (``-m gpu``) -- are held to a bound derived from the number format,
per sample and at the scale of the sample's own stencil, on inputs built for those branches.

YARDSTICK.  ``mp_pchip(x_valid, y_valid, u)``: the interpolant that include/seqik_resample.h describes, written from that
header and scipy's documentation, nothing taken from csrc.  mpmath at 200 bits (the issue asked for >= 160); the float64
inputs, the float64 knots fl(j * ots) and the float64 samples fl(i * nts) are taken as exact.  Derivatives: 0 where the
secant slopes differ in sign or one is 0, else the weighted harmonic mean; the three-point end rule with its two
clamps; two knots give the straight line.  The value is the cubic in the Hermite basis (the code uses powers of
u - x_A).  Interval: the largest valid knot <= u, at most the last but one; the tail continues the last cubic.  Kept as a
float64 pair (hi, lo), so an error is ``(got - hi) - lo``.

BOUND.  u = 2^-53.  Per sample and column:  |got - truth| <= K u S, with S = max |y| over the knots P, A, B, Q of the
sample's stencil as far as they exist (valid knots only in bridge mode).  S == 0 therefore asks for exactly 0.  Every
sample of the contract's finite range is checked (default mode: all of them; bridge mode: x_first_valid <= u <
x_last_valid + ots); outside it the output must be NaN.  ``K_ref`` is the smallest power of two for which
``scipy.interpolate.pchip_interpolate`` stays inside the bound on exactly the inputs below, K = 4 K_ref: the rule and
the margin of tests/test_head_accuracy.py and tests/test_fk_accuracy.py (two correctly rounded evaluation orders of one
cubic differ by a small factor).  K is never read off the code under test; ``test_k_ref_is_measured_on_scipy`` fails
when a scipy or numpy needs more than K_ref.

INPUTS (seeded, built here).  150 knots per chain (three table tiles of bridge mode).  Width 1 (member 0 of a family)
and width 7 (members 0..6, one per column).  Step pairs (ots, nts): (1e-2, 1e-3), (1/100, 1/30), (1e-2, 7e-4),
(1.0, 0.25): the last has samples exactly on knots.
  a. random walk, |y| ~ 10                         e. sawtooth: alternating sign, amplitude in [0.5, 1]
  b. white noise (slope sign changes at most knots) f. monotone: increments from {0, 1e-12, 1e-6, 1}
  c. 1e6 + 1e-3 * noise                            g. decades: noise * 10^k, k in -8..8 per knot (stencil-local S matters)
  d. steps: integers -3..3 held for 5 knots        h. smooth: 2.5 sin(0.07 j + member)
  bridge: a, c, e, g, h with half of the knots missing at random and knots 40..119 missing, knots 0, 38, 39, 120, 121
  and 149 kept, so neighbouring spacings reach 81 : 1; the same with the first 3 or the last 3 knots missing as well.
  A missing knot is a record with NaN, +inf or -inf in one or all of its values (``with_gaps`` of test_resample.py).

MEASURED (EXPERIMENTS.md, "Resampling accuracy"; the tests print the figures, ``-s``).  K_ref = 32 (scipy's largest ratio: 23.266, sawtooth e/last3 at 1e-2 -> 7e-4), K = 128.
Worst error / (u S) per family over all step pairs and members:
    family      a      b      c      d      e      f      g      h
    scipy       8.240 11.306  1.524  9.010 19.511  6.717  9.748  2.744
    host build  5.309 11.373  0.524  6.963 15.548  2.717 12.512  2.287
    bridge      a/gaps a/first3 a/last3  c/*    e/gaps e/first3 e/last3  g/gaps g/first3 g/last3  h/*
    scipy       13.561 13.561   13.561   1.497  19.511 19.511   23.266   9.448  9.448    13.644   7.743
    host build   8.421  8.421    8.421   0.524  15.548 15.548   21.489   7.001  7.001    11.896   2.788
    device      not measured when this was written (no GPU run could be made); the GPU tier asserts the host build's bits and
                the bound on the device output itself, and prints the figures.

FOUND BY THIS MODULE.  The sample on the LAST knot (u == x_{n-1}: nts == ots, or (1.0, 0.25)) was evaluated with the
last interval's cubic at s = h and missed y_{n-1} by rounding -- by 4e-4 of its value in family g, where the neighbours
are decades larger (44 of 224 series at equal steps; scipy does the same).  ``test_equal_steps_return_the_input`` and
``test_samples_on_knots_return_the_knot_values`` failed on it; ``pchip_eval`` and the staged kernel now return the
knot's value there.
"""
import numpy as np
import pytest

from test_resample import ResampleHarness, rs_harness, with_gaps  # noqa: F401  (fixture: the rules run on the host)

import mpmath
from mpmath.libmp import fone, from_float, from_int, mpf_add, mpf_mul, mpf_neg, mpf_shift, mpf_sub, to_float

U = 2.0 ** -53
K_REF = 32
K = 4 * K_REF
N_KNOTS = 150
MEMBERS = 7
STEPS = [(1e-2, 1e-3), (1 / 100, 1 / 30), (1e-2, 7e-4), (1.0, 0.25)]
FAMILIES = "abcdefgh"
BRIDGE_FAMILIES = "acegh"
VARIANTS = ("gaps", "first3", "last3")
NONFINITE_KNOTS = (0, 1, 20, 63, 64, 65, 148, 149)
NONFINITE_VALUES = (np.nan, np.inf, -np.inf)

_MP = mpmath.mp.clone()
_MP.prec = 200
_THREE = from_int(3)


# ------------------------------------------------------ yardstick ------------------------------------------------------

def _sgn(v):
    return (v > 0) - (v < 0)


def _mp_edge(h0, h1, m0, m1):
    """three-point rule at an end knot: h0, m0 of the interval next to it, h1, m1 of the one behind that"""
    d = ((2 * h0 + h1) * m0 - h0 * m1) / (h0 + h1)
    if _sgn(d) != _sgn(m0):
        return _MP.mpf(0)
    if _sgn(m0) != _sgn(m1) and abs(d) > 3 * abs(m0):
        return 3 * m0
    return d


def mp_pchip(x_valid, y_valid, u):
    """The interpolant of include/seqik_resample.h over the knots (x_valid, y_valid) at the samples u, all float64 and
    taken as exact -> (hi, lo): the float64 nearest to the exact value and what is left."""
    mpf = _MP.mpf
    X, Y = [mpf(float(v)) for v in x_valid], [mpf(float(v)) for v in y_valid]
    n = len(X)
    assert n >= 2
    H = [X[k + 1] - X[k] for k in range(n - 1)]
    M = [(Y[k + 1] - Y[k]) / H[k] for k in range(n - 1)]
    if n == 2:
        D = [M[0], M[0]]
    else:
        D = [_mp_edge(H[0], H[1], M[0], M[1])]
        for k in range(1, n - 1):
            m0, m1 = M[k - 1], M[k]
            if _sgn(m0) != _sgn(m1) or m0 == 0 or m1 == 0:
                D.append(mpf(0))
            else:
                w1, w2 = 2 * H[k] + H[k - 1], H[k] + 2 * H[k - 1]
                D.append((w1 + w2) / (w1 / m0 + w2 / m1))
        D.append(_mp_edge(H[-1], H[-2], M[-1], M[-2]))
    j = np.clip(np.searchsorted(x_valid, u, side="right") - 1, 0, n - 2)
    hi, lo = np.empty(len(u)), np.empty(len(u))
    # y_A h00(t) + h d_A h10(t) + y_B h01(t) + h d_B h11(t), t = (u - x_A) / h, on mpmath's raw numbers (libmp: the same
    # arithmetic at the same 200 bits without the per-operation cost of the mpf class; 1 / h is rounded once more)
    P, R = _MP.prec, "n"
    raw = [(X[k]._mpf_, (1 / H[k])._mpf_, Y[k]._mpf_, (H[k] * D[k])._mpf_, Y[k + 1]._mpf_, (H[k] * D[k + 1])._mpf_)
           for k in range(n - 1)]
    for i in range(len(u)):
        xa, ih, ya, hda, yb, hdb = raw[int(j[i])]
        t = mpf_mul(mpf_sub(from_float(float(u[i])), xa, P, R), ih, P, R)
        s = mpf_sub(fone, t, P, R)
        tt, ss = mpf_mul(t, t, P, R), mpf_mul(s, s, P, R)
        h00 = mpf_mul(mpf_add(fone, mpf_shift(t, 1), P, R), ss, P, R)
        h10 = mpf_mul(t, ss, P, R)
        h01 = mpf_mul(tt, mpf_sub(_THREE, mpf_shift(t, 1), P, R), P, R)
        h11 = mpf_neg(mpf_mul(tt, s, P, R))
        v = mpf_add(mpf_add(mpf_mul(ya, h00, P, R), mpf_mul(hda, h10, P, R), P, R),
                    mpf_add(mpf_mul(yb, h01, P, R), mpf_mul(hdb, h11, P, R), P, R), P, R)
        hi[i] = to_float(v, rnd=R)
        lo[i] = to_float(mpf_sub(v, from_float(float(hi[i])), P, R), rnd=R)
    return hi, lo


# -------------------------------------------------------- inputs --------------------------------------------------------

def grid(n, ots, nts):
    u = np.arange(0, n * ots, nts)
    assert np.array_equal(u, np.arange(len(u)) * nts)
    return np.arange(n) * ots, u


def family(name, n=N_KNOTS, members=MEMBERS):
    """(n, members) float64: one member of the family per column"""
    cols = []
    for m in range(members):
        rng = np.random.default_rng([ord(name), m, n])
        j = np.arange(n)
        if name == "a":
            y = np.cumsum(rng.normal(size=n)) * 0.8
        elif name == "b":
            y = rng.normal(size=n)
        elif name == "c":
            y = 1e6 + 1e-3 * rng.normal(size=n)
        elif name == "d":
            y = np.repeat(rng.integers(-3, 4, (n + 4) // 5), 5)[:n].astype(np.float64)
        elif name == "e":
            y = np.where((j + m) % 2 == 0, 1.0, -1.0) * rng.uniform(0.5, 1.0, n)
        elif name == "f":
            y = np.cumsum(rng.choice([0.0, 1e-12, 1e-6, 1.0], n))
        elif name == "g":
            y = rng.normal(size=n) * 10.0 ** rng.integers(-8, 9, n)
        else:
            assert name == "h"
            y = 2.5 * np.sin(0.07 * j + m)
        cols.append(y)
    return np.ascontiguousarray(np.stack(cols, axis=1))


def bridge_mask(name, variant, n=N_KNOTS):
    rng = np.random.default_rng([ord(name), 77, n])
    m = rng.random(n) < 0.5
    m[40:120] = True
    m[[0, 38, 39, 120, 121, n - 1]] = False
    if variant == "first3":
        m[:3] = True
    elif variant == "last3":
        m[-3:] = True
    else:
        assert variant == "gaps"
    return m


def stencil_scale(xv, yv, u):
    """S per sample and column: max |y| over the knots P, A, B, Q of the sample's interval, as far as they exist"""
    nv = len(xv)
    j = np.clip(np.searchsorted(xv, u, side="right") - 1, 0, nv - 2)
    a = np.abs(yv)
    S = np.maximum(a[j], a[j + 1])
    S = np.maximum(S, np.where((j > 0)[:, None], a[np.maximum(j - 1, 0)], 0.0))
    return np.maximum(S, np.where((j + 2 < nv)[:, None], a[np.minimum(j + 2, nv - 1)], 0.0))


class Case:
    """One input of the accuracy tests: the clean values, the missing knots (bridge mode), and per step pair the truth"""

    def __init__(self, name, variant=None):
        self.name, self.variant, self.bridge = name, variant, variant is not None
        self.label = name if variant is None else f"{name}/{variant}"
        self.y = family(name)
        self.mask = bridge_mask(name, variant) if self.bridge else np.zeros(N_KNOTS, bool)
        self._truth = {}

    def data(self, width):
        """what the code under test gets: (150, 7), or member 0 as (150,); missing knots as non-finite records"""
        y = self.y if width == MEMBERS else self.y[:, 0]
        return with_gaps(y, self.mask, 5 + width) if self.bridge else y.copy()

    def valid(self, ots, nts):
        x, u = grid(N_KNOTS, ots, nts)
        keep = ~self.mask
        inside = (u >= x[keep][0]) & (u < x[keep][-1] + ots) if self.bridge else np.ones(len(u), bool)
        return x[keep], self.y[keep], u, inside

    def stencils(self, ots, nts):
        """(n_out, 4): the knots P, A, B, Q of every sample's stencil, -1 / 150 for a P / Q that does not exist"""
        x, u = grid(N_KNOTS, ots, nts)
        keep = np.flatnonzero(~self.mask)
        nv = len(keep)
        j = np.clip(np.searchsorted(x[keep], u, side="right") - 1, 0, nv - 2)
        P = np.where(j > 0, keep[np.maximum(j - 1, 0)], -1)
        Q = np.where(j + 2 < nv, keep[np.minimum(j + 2, nv - 1)], N_KNOTS)
        return np.stack([P, keep[j], keep[j + 1], Q], axis=1)

    def truth(self, si):
        """(hi, lo, S, inside) of step pair si; hi / lo / S are (n_out, 7), rows outside the finite range unset.  The
        interpolant at a sample is a function of its stencil's four knots alone, so a first3 / last3 chain takes from
        the gaps chain of its family (the same values and random mask) the samples whose stencil is the same, and the
        yardstick runs on the rest."""
        if si not in self._truth:
            xv, yv, u, inside = self.valid(*STEPS[si])
            hi, lo = np.full((len(u), MEMBERS), np.nan), np.full((len(u), MEMBERS), np.nan)
            todo = inside
            if self.variant in ("first3", "last3"):
                base = case(self.name, "gaps")
                bhi, blo, _, binside = base.truth(si)
                same = inside & binside & (self.stencils(*STEPS[si]) == base.stencils(*STEPS[si])).all(axis=1)
                assert same.any()
                hi[same], lo[same] = bhi[same], blo[same]
                todo = inside & ~same
            for c in range(MEMBERS):
                hi[todo, c], lo[todo, c] = mp_pchip(xv, yv[:, c], u[todo])
            self._truth[si] = (hi, lo, stencil_scale(xv, yv, u), inside)
        return self._truth[si]

    def scipy(self, si):
        from scipy.interpolate import pchip_interpolate
        xv, yv, u, inside = self.valid(*STEPS[si])
        return np.stack([pchip_interpolate(xv, yv[:, c], u) for c in range(MEMBERS)], axis=1)


_CASES = {}


def case(name, variant=None):
    if (name, variant) not in _CASES:
        _CASES[name, variant] = Case(name, variant)
    return _CASES[name, variant]


ALL_CASES = [(f, None) for f in FAMILIES] + [(f, v) for f in BRIDGE_FAMILIES for v in VARIANTS]
CASE_IDS = [f if v is None else f"{f}-{v}" for f, v in ALL_CASES]
RATIOS = {}


def worst_ratio(cs, si, got, cols=slice(None)):
    """max |got - truth| / (u S) over the finite range; asserts exact zeros where S == 0 and NaN outside the range"""
    hi, lo, S, inside = cs.truth(si)
    hi, lo, S = hi[:, cols], lo[:, cols], S[:, cols]
    assert got.shape == hi.shape, (got.shape, hi.shape)
    assert np.isnan(got[~inside]).all(), (cs.label, si, "finite outside the contract's range")
    g, h, l, s = got[inside], hi[inside], lo[inside], S[inside]
    assert np.isfinite(g).all(), (cs.label, si, "not finite inside the contract's range")
    err = np.abs((g - h) - l)
    assert (err[s == 0] == 0).all() and (g[s == 0] == 0).all(), (cs.label, si, "S == 0 asks for exactly 0")
    return float((err[s > 0] / (U * s[s > 0])).max())


def note(who, cs, ratio):
    key = (who, cs.label)
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)


def bits_equal(a, b):
    """the same values, zeros of the same sign, NaN where the other has NaN (a NaN's payload and sign are not compared)"""
    if a.shape != b.shape or not np.array_equal(a, b, equal_nan=True):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(np.signbit(a[ok]), np.signbit(b[ok]))


# ---------------------------------------------------------------------------------------------------------------------
# CPU tier
# ---------------------------------------------------------------------------------------------------------------------

def test_yardstick_on_cubics_and_lines():
    """mp_pchip reproduces what needs no rule: two knots give the line, knots on a line give the line, a monotone cubic's
    own data with equal spacing is interpolated at the knots."""
    x = np.array([0.0, 0.5, 2.0, 2.25, 7.0])
    u = np.linspace(0.0, 8.0, 33)
    tiny = 2.0 ** -180       # the 200-bit quotient (u - x_A) / h is rounded
    hi, lo = mp_pchip(x[:2], np.array([1.0, 3.0]), u)
    assert np.abs(hi - (1.0 + 4.0 * u)).max() <= tiny and np.abs(lo).max() <= tiny
    hi, lo = mp_pchip(x, 3.0 - 0.5 * x, u)
    assert np.abs(hi - (3.0 - 0.5 * u)).max() <= tiny and np.abs(lo).max() <= tiny
    y = np.array([1.0, -2.0, 4.0, 4.0, 1e-3])
    hi, lo = mp_pchip(x, y, x)
    assert np.array_equal(hi, y) and not lo.any()
    # sign change at knot 1 and 2, a flat interval: the derivative is 0 there and the flat interval stays flat
    hi, _ = mp_pchip(x, y, np.array([2.0, 2.1, 2.2, 2.25]))
    assert np.array_equal(hi, np.full(4, 4.0))
    from scipy.interpolate import pchip_interpolate
    assert np.abs(hi - pchip_interpolate(x, y, np.array([2.0, 2.1, 2.2, 2.25]))).max() == 0
    hi, _ = mp_pchip(x, y, u)
    assert np.abs(hi - pchip_interpolate(x, y, u)).max() <= 64 * U * 4.0


def test_bridge_inputs_reach_spacing_ratios_of_80():
    for f in BRIDGE_FAMILIES:
        for v in VARIANTS:
            keep = np.flatnonzero(~bridge_mask(f, v))
            h = np.diff(keep)
            assert (np.maximum(h[1:] / h[:-1], h[:-1] / h[1:])).max() >= 80
            assert 0.3 <= 1 - len(keep) / N_KNOTS
            assert (keep[0], keep[-1]) == {"gaps": (0, 149), "first3": (keep[0], 149), "last3": (0, keep[-1])}[v]
            assert keep[0] >= (3 if v == "first3" else 0) and keep[-1] <= (146 if v == "last3" else 149)


def test_k_ref_is_measured_on_scipy():
    """scipy.interpolate.pchip_interpolate itself, on every input of this module, stays within K_ref u S of the yardstick:
    K = 4 K_ref rests on this measurement.  A scipy / numpy that needs more fails here instead of loosening K unseen."""
    worst = 0.0
    for f, v in ALL_CASES:
        cs = case(f, v)
        for si in range(len(STEPS)):
            got = cs.scipy(si)
            got[~cs.truth(si)[3]] = np.nan
            r = worst_ratio(cs, si, got)
            note("scipy", cs, r)
            worst = max(worst, r)
        print(f"scipy       {cs.label:9s} worst |err| / (u S) = {RATIOS['scipy', cs.label]:.3f}")
    print(f"scipy overall {worst:.3f}; K_ref = {K_REF}, K = {K}")
    assert worst <= K_REF
    assert K == 4 * K_REF and K_REF & (K_REF - 1) == 0


@pytest.mark.parametrize("f,v", ALL_CASES, ids=CASE_IDS)
def test_host_rules_inside_the_bound(rs_harness, f, v):
    cs = case(f, v)
    for si, (ots, nts) in enumerate(STEPS):
        got7 = rs_harness.chain(cs.data(7), ots, nts, bridge=cs.bridge)
        got1 = rs_harness.chain(cs.data(1), ots, nts, bridge=cs.bridge)
        r7, r1 = worst_ratio(cs, si, got7), worst_ratio(cs, si, got1[:, None], slice(0, 1))
        note("host", cs, max(r7, r1))
        print(f"host build  {cs.label:9s} {ots:g}->{nts:g}: width 7 {r7:.3f}, width 1 {r1:.3f} (K = {K})")
        assert max(r7, r1) <= K, (cs.label, ots, nts, r7, r1)
        assert bits_equal(got1, got7[:, 0])          # a column knows nothing of its neighbours
        if f == "d":
            # on a flat run (both knots of the interval equal) the output is that value
            x, u = grid(N_KNOTS, ots, nts)
            j = np.clip(np.searchsorted(x, u, side="right") - 1, 0, N_KNOTS - 2)
            flat = cs.y[j] == cs.y[j + 1]
            assert flat.sum() > 0.5 * flat.size
            assert np.array_equal(got7[flat], cs.y[j][flat])


@pytest.mark.parametrize("ts", [1e-2, 1 / 30, 0.1, 1.0])
def test_equal_steps_return_the_input(rs_harness, ts):
    for f, v in ALL_CASES:
        cs = case(f, v)
        for w in (1, 7):
            y = cs.data(w)
            got = rs_harness.chain(y, ts, ts, bridge=cs.bridge)
            assert len(got) >= N_KNOTS
            want = (cs.y if w == 7 else cs.y[:, 0]).copy()
            want[cs.mask] = np.nan
            if cs.bridge:
                # a missing knot between valid ones is bridged: only the valid knots return their input
                keep = np.flatnonzero(~cs.mask)
                assert bits_equal(got[:N_KNOTS][keep], want[keep]), (cs.label, w)
                inside = cs.valid(ts, ts)[3]
                assert np.isnan(got[~inside]).all() and np.isfinite(got[inside]).all()
                assert inside[keep[0]:keep[-1] + 1].all() and not inside[:keep[0]].any()
            else:
                assert bits_equal(got[:N_KNOTS], want), (cs.label, w)


def test_samples_on_knots_return_the_knot_values(rs_harness):
    hits = 0
    for f, v in ALL_CASES:
        cs = case(f, v)
        for ots, nts in STEPS + [(1e-2, 5e-3), (0.5, 0.125)]:
            x, u = grid(N_KNOTS, ots, nts)
            got = rs_harness.chain(cs.data(7), ots, nts, bridge=cs.bridge)
            jj = np.searchsorted(x, u)
            on = (jj < N_KNOTS) & (x[np.minimum(jj, N_KNOTS - 1)] == u)
            on &= ~cs.mask[np.minimum(jj, N_KNOTS - 1)]
            hits += int(on.sum())
            assert bits_equal(got[on], cs.y[jj[on]]), (cs.label, ots, nts)
    assert hits > 5000


@pytest.mark.parametrize("f,v", ALL_CASES, ids=CASE_IDS)
def test_negation_commutes(rs_harness, f, v):
    cs = case(f, v)
    for ots, nts in STEPS:
        y = cs.data(7)
        pos, neg = rs_harness.chain(y, ots, nts, bridge=cs.bridge), rs_harness.chain(-y, ots, nts, bridge=cs.bridge)
        assert np.array_equal(np.isnan(pos), np.isnan(neg))
        ok = ~np.isnan(pos)
        assert np.array_equal(neg[ok], -pos[ok]), (cs.label, ots, nts)


@pytest.mark.parametrize("k", [-900, -300, 300, 900])
def test_power_of_two_scaling_commutes(rs_harness, k):
    for v in (None, "gaps"):
        cs = case("a", v)
        for ots, nts in STEPS:
            y = cs.data(7)
            base = rs_harness.chain(y, ots, nts, bridge=cs.bridge)
            got = rs_harness.chain(np.ldexp(y, k), ots, nts, bridge=cs.bridge)
            ok = ~np.isnan(base)
            assert np.array_equal(np.isnan(got), ~ok)
            assert np.isfinite(got[ok]).all()
            assert np.array_equal(got[ok], np.ldexp(base[ok], k)), (k, v, ots, nts)
            if k > 0:
                assert np.abs(got[ok]).max() > 2.0 ** (k - 2)


@pytest.mark.parametrize("value", [0.0, -0.0, 1.0, -2.5, 1e6 + 1e-3, 1e-300, -1e300, 0.1])
def test_a_constant_series_gives_that_constant(rs_harness, value):
    for ots, nts in STEPS:
        y = np.full((N_KNOTS, 7), value)
        got = rs_harness.chain(y, ots, nts)
        assert (got == value).all()
        y[bridge_mask("a", "gaps")] = np.nan
        got = rs_harness.chain(y, ots, nts, bridge=True)
        assert (got[~np.isnan(got)] == value).all() and np.isfinite(got).mean() > 0.9


def test_monotone_input_gives_monotone_output(rs_harness):
    cs = case("f")
    assert (np.diff(cs.y, axis=0) >= 0).all() and (np.diff(cs.y, axis=0) == 0).any()
    for ots, nts in STEPS:
        x, u = grid(N_KNOTS, ots, nts)
        got = rs_harness.chain(cs.y, ots, nts)
        front = got[u <= x[-1]]
        d = np.diff(front, axis=0)
        assert (d >= 0).all(), (ots, nts, d.min(), np.argwhere(d < 0)[:5])


def nonfinite_inputs(y):
    """(cases, n, w) chains from y (n, w): one knot of NONFINITE_KNOTS x one value at a time (in column knot % w), then all
    of them at once, and the mask (cases, n, w) of what is non-finite"""
    n, w = y.shape
    chains, k_all = [], 0
    for kn in NONFINITE_KNOTS:
        for val in NONFINITE_VALUES:
            c = y.copy()
            c[kn, kn % w] = val
            chains.append(c)
    c = y.copy()
    for kn in NONFINITE_KNOTS:
        c[kn, kn % w] = NONFINITE_VALUES[k_all % 3]
        k_all += 1
    chains.append(c)
    chains = np.stack(chains)
    return chains, ~np.isfinite(chains)


def predicted_nan(bad, ots, nts):
    """default mode: sample i of a column is NaN when one of the knots A - 1 .. A + 2 (A = its interval, at most n - 2)
    that exist is non-finite in that column.  bad (..., n, w) -> (..., n_out, w)"""
    n = bad.shape[-2]
    x, u = grid(n, ots, nts)
    A = np.clip(np.searchsorted(x, u, side="right") - 1, 0, n - 2)
    hit = np.zeros(bad.shape[:-2] + (len(u), bad.shape[-1]), bool)
    for o in (-1, 0, 1, 2):
        k = A + o
        ok = (k >= 0) & (k < n)
        hit |= bad[..., np.clip(k, 0, n - 1), :] & ok[:, None]
    return hit


def check_nonfinite(got, clean, bad, ots, nts, what):
    hit = predicted_nan(bad, ots, nts)
    assert hit.any() and not hit.all()
    assert np.array_equal(np.isnan(got), hit), (what, "NaN on another set than the stencils of the non-finite knots")
    assert not np.isinf(got).any()
    keep = ~hit
    assert np.array_equal(got[keep], np.broadcast_to(clean, got.shape)[keep]), (what, "a clean sample changed")


@pytest.mark.parametrize("width", [1, 7])
def test_default_mode_nonfinite_knots_spoil_exactly_their_stencils(rs_harness, width):
    y = family("a")[:, :width]
    chains, bad = nonfinite_inputs(y)
    assert chains.shape == (25, N_KNOTS, width)
    for ots, nts in STEPS:
        clean = rs_harness.chain(y, ots, nts)
        assert np.isfinite(clean).all()
        got = rs_harness.chains(chains, ots, nts)
        check_nonfinite(got, clean, bad, ots, nts, (width, ots, nts))


# ---------------------------------------------------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------------------------------------------------

GUARD = 64
SENTINEL_F64 = -7.0e77
SENTINEL_I32 = -123456789


def device_run(hiplib, y, ots, nts, bridge=False, max_gap=None, want_tables=False):
    """seqik_resample_pchip_device on (C, N, W) through raw pointers into guarded buffers: 64 sentinel words on either
    side of d_out and of the int32 workspace.  Returns the output (and the tables), after checking the sentinels."""
    import torch
    y = np.ascontiguousarray(y, dtype=np.float64)
    C, N, W = y.shape
    n_out = hiplib.resample_count(N, ots, nts)
    d_y = torch.from_numpy(y).cuda()
    out_buf = torch.full((2 * GUARD + C * n_out * W,), SENTINEL_F64, dtype=torch.float64, device="cuda")
    d_out = out_buf[GUARD:GUARD + C * n_out * W]
    ws_buf = torch.full((2 * GUARD + 2 * C * N,), SENTINEL_I32, dtype=torch.int32, device="cuda")
    d_ws = ws_buf[GUARD:GUARD + 2 * C * N]
    torch.cuda.synchronize()
    if bridge:
        assert hiplib.resample_workspace_bytes(C, N, "bridge") == 4 * d_ws.numel()
        hiplib.resample_pchip_device(d_y.data_ptr(), C, N, W, ots, nts, d_out.data_ptr(), missing="bridge", max_gap=max_gap,
                                     d_workspace=d_ws.data_ptr())
    else:
        hiplib.resample_pchip_device(d_y.data_ptr(), C, N, W, ots, nts, d_out.data_ptr())
    torch.cuda.synchronize()
    out, ws = out_buf.cpu().numpy(), ws_buf.cpu().numpy()
    for g in (out[:GUARD], out[-GUARD:]):
        assert (g == SENTINEL_F64).all(), "the kernel wrote outside d_out"
    for g in (ws[:GUARD], ws[-GUARD:]):
        assert (g == SENTINEL_I32).all(), "the table kernels wrote outside the workspace"
    if not bridge:
        assert (ws == SENTINEL_I32).all(), "default mode touched the workspace"
    res = out[GUARD:-GUARD].reshape(C, n_out, W)
    assert not (res == SENTINEL_F64).any(), "an output element was never written"
    if want_tables:
        return res, ws[GUARD:-GUARD].reshape(2, C, N)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("f,v", ALL_CASES, ids=CASE_IDS)
def test_device_equals_host_rules_and_meets_the_bound(hiplib, rs_harness, f, v):
    cs = case(f, v)
    for si, (ots, nts) in enumerate(STEPS):
        for w in (7, 1):
            y = cs.data(w).reshape(1, N_KNOTS, w)
            want = rs_harness.chains(y, ots, nts, bridge=cs.bridge)
            if cs.bridge:
                got = hiplib.resample_pchip(y, ots, nts, missing="bridge")
                assert bits_equal(device_run(hiplib, y, ots, nts, bridge=True), got)
            else:
                got = device_run(hiplib, y, ots, nts)
                assert bits_equal(hiplib.resample_pchip(y, ots, nts), got)
            assert bits_equal(got, want), (cs.label, ots, nts, w)
            r = worst_ratio(cs, si, got[0], slice(0, w))
            note("device", cs, r)
            assert r <= K, (cs.label, ots, nts, w, r)
    print(f"device      {cs.label:9s} worst |err| / (u S) = {RATIOS['device', cs.label]:.3f} (K = {K})")


def gappy(y, rng, frac):
    """frac of the records of y (C, N, W) made missing: one value of the record non-finite"""
    C, N, W = y.shape
    g = y.copy()
    hit = rng.random((C, N)) < frac
    cs, ns = np.nonzero(hit)
    g[cs, ns, rng.integers(0, W, len(cs))] = rng.choice(NONFINITE_VALUES, len(cs))
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("width", range(1, 17))
def test_every_width_bit_for_bit(hiplib, rs_harness, width):
    rng = np.random.default_rng(100 + width)
    for n in (150, 1000):
        y = np.cumsum(rng.normal(size=(3, n, width)), axis=1)
        gy = gappy(y, rng, 0.2)
        for ots, nts in ((1e-2, 1e-3), (1e-2, 7e-4), (1e-2, 1.3e-2)):
            assert bits_equal(device_run(hiplib, y, ots, nts), rs_harness.chains(y, ots, nts)), (width, n, ots, nts)
            assert bits_equal(device_run(hiplib, gy, ots, nts, bridge=True),
                              rs_harness.chains(gy, ots, nts, bridge=True)), (width, n, ots, nts, "bridge")


SEAM_RATIOS = (1.5, 2, 3, 3.5, 4, 4.5, 6, 9, 13, 20, 40, 70, 130, 260)


@pytest.mark.gpu
@pytest.mark.parametrize("width", [1, 7, 16])
def test_staged_direct_seam(hiplib, rs_harness, width):
    """A tile is staged in LDS when its knot run fits into 256 doubles, else every lane loads for itself: ratios at which
    one launch holds tiles of both kinds, and gaps (bridge mode) that push single tiles over the edge."""
    rng = np.random.default_rng(200 + width)
    n, ots = 2000, 1e-2
    y = np.cumsum(rng.normal(size=(3, n, width)), axis=1)
    gy = y.copy()
    for c in range(3):
        k = int(rng.integers(1, 20))
        while k < n - 1:
            g = int(rng.integers(1, 41))
            gy[c, k:min(k + g, n - 1), rng.integers(0, width)] = np.nan
            k += g + int(rng.integers(1, 60))
    assert np.isfinite(gy[:, 0]).all() and np.isfinite(gy[:, -1]).all()
    for ratio in SEAM_RATIOS:
        nts = ratio * ots
        assert bits_equal(device_run(hiplib, y, ots, nts), rs_harness.chains(y, ots, nts)), (width, ratio)
        for max_gap in (None, 5):
            got = device_run(hiplib, gy, ots, nts, bridge=True, max_gap=max_gap)
            want = rs_harness.chains(gy, ots, nts, bridge=True, max_gap=max_gap)
            assert bits_equal(got, want), (width, ratio, max_gap)
            if max_gap is None:
                assert np.isfinite(got).all()
        if ratio < 20:
            assert np.isnan(got).any()          # max_gap = 5 cuts samples out


@pytest.mark.gpu
@pytest.mark.parametrize("width", [1, 7, 16])
def test_default_mode_nonfinite_knots_on_the_device(hiplib, rs_harness, width):
    """The staged path's own code for non-finite knots (the finiteness test that poisons the leading coefficient) and the
    direct path's, through seqik_resample_pchip_device: the host rules' bits, NaN exactly on the predicted set."""
    rng = np.random.default_rng(300 + width)
    y = np.cumsum(rng.normal(size=(N_KNOTS, width)), axis=0)
    chains, bad = nonfinite_inputs(y)
    for ots, nts in ((1e-2, 1e-3), (1e-2, 7e-4), (1.0, 0.25)):
        got = device_run(hiplib, chains, ots, nts)
        assert bits_equal(got, rs_harness.chains(chains, ots, nts)), (width, ots, nts)
        check_nonfinite(got, rs_harness.chain(y, ots, nts), bad, ots, nts, (width, ots, nts))
    # 5 % of single values, staged (ratio 10, 1000 knots) and direct (nts / ots = 100, 20 000 knots)
    for n, ots, nts in ((1000, 1e-2, 1e-3), (20000, 1e-4, 1e-2)):
        y = np.cumsum(rng.normal(size=(3, n, width)), axis=1) * 0.1
        by = y.copy()
        hit = rng.random(y.shape) < 0.05 / width
        by[hit] = rng.choice(NONFINITE_VALUES, int(hit.sum()))
        got = device_run(hiplib, by, ots, nts)
        assert bits_equal(got, rs_harness.chains(by, ots, nts)), (width, n)
        check_nonfinite(got, rs_harness.chains(y, ots, nts), hit, ots, nts, (width, n))


def empty_tile_chains(n, width, tile, rng):
    """chains of n knots with whole table tiles missing: tile 0, a middle tile, the last tile, first and last, all but one
    knot, all knots"""
    tiles = (n + tile - 1) // tile
    base = np.cumsum(rng.normal(size=(6, n, width)), axis=1) * 0.1
    base[rng.random((6, n)) < 0.1, rng.integers(0, width)] = np.nan
    y = base.copy()
    y[0, :tile] = np.nan
    y[1, (tiles // 2) * tile:(tiles // 2 + 1) * tile] = np.inf
    y[2, (tiles - 1) * tile:] = np.nan
    y[3, :tile] = -np.inf
    y[3, (tiles - 1) * tile:] = np.nan
    y[4] = np.nan
    y[4, n // 2 + 3] = 1.0
    y[5] = np.nan
    return y


def check_tables_and_output(hiplib, rs_harness, y, ots, nts, what):
    got, ws = device_run(hiplib, y, ots, nts, bridge=True, want_tables=True)
    for c in range(y.shape[0]):
        prev, nxt = rs_harness.tables(y[c])
        assert np.array_equal(ws[0, c], prev), (what, c, "prev")
        assert np.array_equal(ws[1, c], nxt), (what, c, "next")
    assert bits_equal(got, rs_harness.chains(y, ots, nts, bridge=True)), what
    return got


@pytest.mark.gpu
def test_empty_table_tiles_at_small_sizes(hiplib, rs_harness):
    rng = np.random.default_rng(400)
    for n in (200, 260):
        for width in (1, 7):
            y = empty_tile_chains(n, width, 64, rng)
            for ots, nts in ((1e-2, 1e-3), (1e-2, 1.3e-2)):
                got = check_tables_and_output(hiplib, rs_harness, y, ots, nts, (n, width, ots, nts))
                assert np.isnan(got[4:]).all() and np.isfinite(got[:4]).any(axis=(1, 2)).all()
    # tiles wider than 64 knots: 70 000 knots make tiles of 128
    y = empty_tile_chains(70000, 1, 128, rng)
    check_tables_and_output(hiplib, rs_harness, y, 1e-2, 3e-3, 70000)
    # the downsampling geometry of test_tiling_shapes (200 000 knots, tiles of 256, the direct path), whole tiles empty
    y = empty_tile_chains(200000, 7, 256, rng)[:4]
    y[1, 50000:90000] = np.nan
    check_tables_and_output(hiplib, rs_harness, y, 1e-4, 1e-2, 200000)


@pytest.mark.gpu
def test_guard_words_around_output_and_workspace(hiplib, rs_harness):
    """device_run surrounds d_out and the workspace with sentinels in every GPU test of this module; here on shapes whose
    n_out * width is no multiple of 64, with the guards counted."""
    rng = np.random.default_rng(500)
    shapes = 0
    for n, width, ots, nts in ((150, 1, 1e-2, 7e-4), (150, 7, 1e-2, 1e-3), (1000, 3, 1e-2, 1.3e-2), (150, 13, 1e-2, 1.3e-2),
                               (2000, 7, 1e-2, 3.5e-2), (2000, 16, 1e-2, 0.13), (2000, 1, 1e-2, 4.5e-2), (2, 5, 1.0, 0.3)):
        n_out = hiplib.resample_count(n, ots, nts)
        assert (n_out * width) % 64 != 0
        for chains in (1, 3):
            y = np.cumsum(rng.normal(size=(chains, n, width)), axis=1)
            assert bits_equal(device_run(hiplib, y, ots, nts), rs_harness.chains(y, ots, nts))
            gy = gappy(y, rng, 0.2) if n > 2 else y
            for max_gap in (None, 5):
                assert bits_equal(device_run(hiplib, gy, ots, nts, bridge=True, max_gap=max_gap),
                                  rs_harness.chains(gy, ots, nts, bridge=True, max_gap=max_gap))
            shapes += 1
    assert shapes == 16
