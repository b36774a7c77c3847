// seqik_resample.hpp -- the per-sample rules of PCHIP resampling (include/seqik_resample.h), host and device.
//
// The kernels of seqik_resample.hip and the host test harness (tests/harness/resample_harness.hip) share these functions:
//   resample_x / resample_interval   where knot j and sample i sit, and the knot interval a sample falls into
//   pchip_interior / pchip_edge      scipy's PchipInterpolator._find_derivatives / _edge_case on one knot
//   pchip_deriv                      the derivative at a knot from its (up to four) neighbours
//   pchip_coefs / pchip_horner       the cubic of one interval in powers of (u - x_A), as scipy's CubicHermiteSpline
//   resample_bridge_stencil / _ok    bridge mode: the interval and stencil between VALID knots from the neighbour tables
//   resample_neighbours              the knots a knot's derivative is made from, in either mode
//   pchip_horner / _d1 / _d2, pchip_cubic_orders   the cubic's value, first and second derivative; the on-knot-B rule
//   pchip_eval_der / resample_sample_der   the orders asked for of one output sample (include/seqik_resample_der.h): what
//                                    the kernel's direct path runs per lane; pchip_eval / resample_sample: the value alone
// resample_tables_chain / resample_chain (_der) apply them to one chain on the host: the restatement of the contract.  Every
// operation is one IEEE binary64 operation or an explicit fused multiply-add (built with -ffp-contract=off), divisions are
// the compiler's correctly rounded ones, so host and device agree bit for bit.
#pragma once
#include "seqik_core.hpp"
#include "../../include/seqik_resample.h"

namespace seqik {

constexpr int kResampleMaxWidth = 16;

struct ResampleParams {
    double ots, inv_ots, nts;  // inv_ots = 1 / ots, computed once on the host (a guess only, see resample_interval)
    int32_t n_frames, n_out;   // both below 2^31
    int32_t width, flags, max_gap;
};

SEQIK_HD ResampleParams resample_params(double ots, double nts, int32_t n_frames, int32_t n_out, int32_t width,
                                        int32_t flags, int32_t max_gap)
{
    ResampleParams p;
    p.ots = ots;
    p.inv_ots = 1.0 / ots;
    p.nts = nts;
    p.n_frames = n_frames;
    p.n_out = n_out;
    p.width = width;
    p.flags = flags;
    p.max_gap = max_gap;
    return p;
}

// numpy's length rule for np.arange(0, n_frames * ots, nts), as a double (the caller checks the range)
inline double resample_count_f64(int64_t n_frames, double ots, double nts)
{
    return ceil(((double)n_frames * ots) / nts);
}

SEQIK_HD double resample_nan() { return __builtin_nan(""); }

// position of knot j (ts = original_ts) or of sample i (ts = new_ts): one multiplication
SEQIK_HD double resample_x(int32_t j, double ts) { return (double)j * ts; }

// the largest j in [0, n - 1] with x_j <= u (u >= 0); the product with 1 / ots is a guess that the loops correct
SEQIK_HD int32_t resample_interval(double u, double ots, double inv_ots, int32_t n)
{
    const double g = u * inv_ots;
    int32_t j = g < (double)(n - 1) ? (int32_t)g : n - 1;
    while (j + 1 < n && resample_x(j + 1, ots) <= u) ++j;
    while (j > 0 && resample_x(j, ots) > u) --j;
    return j;
}

SEQIK_HD double pchip_sign(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0); }

// interior knot: h0, m0 the spacing and secant slope on its left, h1, m1 on its right
SEQIK_HD double pchip_interior(double h0, double h1, double m0, double m1)
{
    const bool flat = pchip_sign(m0) != pchip_sign(m1) || m0 == 0.0 || m1 == 0.0;
    const double w1 = 2.0 * h1 + h0, w2 = h1 + 2.0 * h0;
    const double whmean = (w1 / m0 + w2 / m1) / (w1 + w2);
    return flat ? 0.0 : 1.0 / whmean;
}

// end knot: h0, m0 of the interval next to it, h1, m1 of the one behind that (three-point rule)
SEQIK_HD double pchip_edge(double h0, double h1, double m0, double m1)
{
    double d = ((2.0 * h0 + h1) * m0 - h0 * m1) / (h0 + h1);
    if (pchip_sign(d) != pchip_sign(m0)) d = 0.0;
    else if (pchip_sign(m0) != pchip_sign(m1) && fabs(d) > 3.0 * fabs(m0)) d = 3.0 * m0;
    return d;
}

struct PchipKnot {
    double x, y;
    bool has;
};

// Derivative at knot k0 from its neighbours m1 / p1 (one of them exists) and, at an end, the knot behind the neighbour
// (m2 / p2; when that does not exist either there are two knots in all: the straight line).
SEQIK_HD double pchip_deriv(const PchipKnot &m2, const PchipKnot &m1, const PchipKnot &k0, const PchipKnot &p1,
                            const PchipKnot &p2)
{
    if (m1.has && p1.has) {
        const double h0 = k0.x - m1.x, h1 = p1.x - k0.x;
        return pchip_interior(h0, h1, (k0.y - m1.y) / h0, (p1.y - k0.y) / h1);
    }
    if (p1.has) {
        const double h0 = p1.x - k0.x, s0 = (p1.y - k0.y) / h0;
        if (!p2.has) return s0;
        const double h1 = p2.x - p1.x;
        return pchip_edge(h0, h1, s0, (p2.y - p1.y) / h1);
    }
    const double h0 = k0.x - m1.x, s0 = (k0.y - m1.y) / h0;
    if (!m2.has) return s0;
    const double h1 = m1.x - m2.x;
    return pchip_edge(h0, h1, s0, (m1.y - m2.y) / h1);
}

// cubic on [x_A, x_B] in powers of s = u - x_A: c0 s^3 + c1 s^2 + dA s + yA
SEQIK_HD void pchip_coefs(double xa, double ya, double xb, double yb, double da, double db, double &c0, double &c1)
{
    const double h = xb - xa, slope = (yb - ya) / h;
    const double t = (da + db - 2.0 * slope) / h;
    c0 = t / h;
    c1 = (slope - da) / h - t;
}

SEQIK_HD double pchip_horner(double c0, double c1, double c2, double c3, double s)
{
    const double r = fma_(fma_(fma_(c0, s, c1), s, c2), s, c3);
    return r == r ? r : resample_nan();
}

// d/ds and d2/ds2 of c0 s^3 + c1 s^2 + c2 s + c3; 3 c0, 2 c1 and 6 c0 are one rounding each
SEQIK_HD double pchip_horner_d1(double c0, double c1, double c2, double s)
{
    const double r = fma_(fma_(3.0 * c0, s, 2.0 * c1), s, c2);
    return r == r ? r : resample_nan();
}

SEQIK_HD double pchip_horner_d2(double c0, double c1, double s)
{
    const double r = fma_(6.0 * c0, s, 2.0 * c1);
    return r == r ? r : resample_nan();
}

constexpr int kResampleValue = 1, kResampleD1 = 2, kResampleD2 = 4;  // orders 0, 1, 2 as bits of `want`
constexpr int kResampleAll = kResampleValue | kResampleD1 | kResampleD2;

// The orders in `want` of the cubic c0 s^3 + c1 s^2 + dA s + yA at s: v[0] the value, v[1] and v[2] the first and second
// derivative; orders not asked for are left alone.  on_b: the sample sits ON knot B.  It takes that knot's value y_B (the
// power form at s = h equals it only up to rounding) and that knot's derivative d_B as its first derivative; its second
// derivative is the cubic's at s = h.  Every knot but the last (valid) one starts an interval of its own, where s = 0
// returns y_A and d_A exactly, so this is the last knot's sample alone.  yb, db are read only when on_b.
SEQIK_HD void pchip_cubic_orders(double c0, double c1, double da, double ya, double s, bool on_b, double yb, double db,
                                 int want, double v[3])
{
    if (want & kResampleValue) v[0] = on_b ? yb : pchip_horner(c0, c1, da, ya, s);
    if (want & kResampleD1) v[1] = on_b ? (db == db ? db : resample_nan()) : pchip_horner_d1(c0, c1, da, s);
    if (want & kResampleD2) v[2] = pchip_horner_d2(c0, c1, s);
}

// the stencil P, A, B, Q of interval (A, B) as knots: the orders in `want` of the interpolant at u
SEQIK_HD void pchip_eval_der(const PchipKnot &P, const PchipKnot &A, const PchipKnot &B, const PchipKnot &Q, double u,
                             int want, double v[3])
{
    const PchipKnot none = {0.0, 0.0, false};
    const double da = pchip_deriv(none, P, A, B, Q), db = pchip_deriv(P, A, B, Q, none);
    double c0, c1;
    pchip_coefs(A.x, A.y, B.x, B.y, da, db, c0, c1);
    pchip_cubic_orders(c0, c1, da, A.y, u - A.x, u == B.x, B.y, db, want, v);
}

SEQIK_HD double pchip_eval(const PchipKnot &P, const PchipKnot &A, const PchipKnot &B, const PchipKnot &Q, double u)
{
    double v[3];
    pchip_eval_der(P, A, B, Q, u, kResampleValue, v);
    return v[0];
}

// Bridge mode.  prev[j] = last valid knot <= j (-1: none), next[j] = first valid knot >= j (n: none).  For the raw
// interval j (the largest knot with x_j <= u): the interval (A, B) between valid knots and its stencil knots P (-1: none)
// and Q (n: none).  tail: there is no valid knot behind j and the LAST interval's cubic is used.  false: the sample lies
// in front of the first valid knot, or the chain has fewer than two valid knots.
SEQIK_HD bool resample_bridge_stencil(const int32_t *prev, const int32_t *next, int32_t j, int32_t n, int32_t &P,
                                      int32_t &A, int32_t &B, int32_t &Q, bool &tail)
{
    P = A = B = -1;
    Q = n;
    tail = false;
    const int32_t a = prev[j];
    if (a < 0) return false;
    const int32_t b = j + 1 < n ? next[j + 1] : n;
    tail = b >= n;
    if (tail) {
        B = a;
        A = a > 0 ? prev[a - 1] : -1;
        if (A < 0) return false;
    } else {
        A = a;
        B = b;
    }
    P = A > 0 ? prev[A - 1] : -1;
    Q = B + 1 < n ? next[B + 1] : n;
    return true;
}

// what bridge mode refuses to fill: behind x_last_valid + original_ts, and strictly inside an interval that spans more
// than max_gap missing knots
SEQIK_HD bool resample_bridge_ok(double u, int32_t A, int32_t B, bool tail, double ots, int32_t max_gap)
{
    if (tail) return u < resample_x(B, ots) + ots;
    if (max_gap >= 0 && B - A - 1 > max_gap) return !(u > resample_x(A, ots) && u < resample_x(B, ots));
    return true;
}

// The knots the derivative at knot g is made from (pchip_deriv's m2, m1, p1, p2), in bridge mode its VALID neighbours
// from the tables.  false: g is a missing knot, or has no neighbour at all (fewer than two valid knots).
struct PchipNeighbours {
    int32_t m2, m1, p1, p2;
    bool hm2, hm1, hp1, hp2;  // m2 / p2 count only at an end, where pchip_deriv reads them
};

SEQIK_HD bool resample_neighbours(const int32_t *prev, const int32_t *next, bool bridge, int32_t g, int32_t n,
                                  PchipNeighbours &k)
{
    if (bridge) {
        if (prev[g] != g) return false;
        k.m1 = g > 0 ? prev[g - 1] : -1;
        k.p1 = g + 1 < n ? next[g + 1] : n;
        k.m2 = k.m1 > 0 ? prev[k.m1 - 1] : -1;
        k.p2 = k.p1 + 1 < n ? next[k.p1 + 1] : n;
    } else {
        k.m1 = g - 1;
        k.p1 = g + 1;
        k.m2 = g - 2;
        k.p2 = g + 2;
    }
    k.hm1 = k.m1 >= 0;
    k.hp1 = k.p1 < n;
    if (!k.hm1 && !k.hp1) return false;
    k.hm2 = k.hm1 && !k.hp1 && k.m2 >= 0;
    k.hp2 = !k.hm1 && k.hp1 && k.p2 < n;
    return true;
}

// One output sample, the orders in `want` (v as pchip_cubic_orders): sample i, column col of the chain at ych
// ([n_frames][width]); prev / next: the chain's tables in bridge mode.  Where the interval, stencil, bridge and max_gap
// rules refuse a value every order is NaN.
SEQIK_HD void resample_sample_der(const double *ych, const int32_t *prev, const int32_t *next, const ResampleParams &p,
                                  int32_t i, int col, int want, double v[3])
{
    v[0] = v[1] = v[2] = resample_nan();
    const int32_t n = p.n_frames;
    const double u = resample_x(i, p.nts);
    const int32_t j = resample_interval(u, p.ots, p.inv_ots, n);
    const bool bridge = p.flags & SEQIK_RESAMPLE_BRIDGE;
    int32_t iP, iA, iB, iQ;
    if (bridge) {
        bool tail;
        if (!resample_bridge_stencil(prev, next, j, n, iP, iA, iB, iQ, tail)) return;
        if (!resample_bridge_ok(u, iA, iB, tail, p.ots, p.max_gap)) return;
    } else {
        iA = j < n - 2 ? j : n - 2;
        iB = iA + 1;
        iP = iA - 1;
        iQ = iA + 2;
    }
    const bool hp = iP >= 0, hq = iQ < n;
    const PchipKnot P = {hp ? resample_x(iP, p.ots) : 0.0, hp ? ych[(int64_t)iP * p.width + col] : 0.0, hp};
    const PchipKnot A = {resample_x(iA, p.ots), ych[(int64_t)iA * p.width + col], true};
    const PchipKnot B = {resample_x(iB, p.ots), ych[(int64_t)iB * p.width + col], true};
    const PchipKnot Q = {hq ? resample_x(iQ, p.ots) : 0.0, hq ? ych[(int64_t)iQ * p.width + col] : 0.0, hq};
    if (!bridge && !(is_finite(P.y) && is_finite(A.y) && is_finite(B.y) && is_finite(Q.y))) return;
    pchip_eval_der(P, A, B, Q, u, want, v);
}

SEQIK_HD double resample_sample(const double *ych, const int32_t *prev, const int32_t *next, const ResampleParams &p,
                                int32_t i, int col)
{
    double v[3];
    resample_sample_der(ych, prev, next, p, i, col, kResampleValue, v);
    return v[0];
}

// a knot is missing when any value of its record is non-finite
SEQIK_HD bool resample_knot_valid(const double *rec, int width)
{
    bool ok = true;
    for (int k = 0; k < width; ++k) ok = ok && is_finite(rec[k]);
    return ok;
}

// One chain on the host: the neighbour tables.
inline void resample_tables_chain(const double *y, int32_t n, int width, int32_t *prev, int32_t *next)
{
    int32_t last = -1;
    for (int32_t j = 0; j < n; ++j) {
        if (resample_knot_valid(y + (int64_t)j * width, width)) last = j;
        prev[j] = last;
    }
    int32_t first = n;
    for (int32_t j = n - 1; j >= 0; --j) {
        if (prev[j] == j) first = j;
        next[j] = first;
    }
}

// One chain on the host: y [n_frames][width] -> out_value, out_d1, out_d2 [n_out][width], a null one is not asked for and
// not written; prev / next are filled here in bridge mode.
inline void resample_chain_der(const double *y, const ResampleParams &p, int32_t *prev, int32_t *next, double *out_value,
                               double *out_d1, double *out_d2)
{
    if (p.flags & SEQIK_RESAMPLE_BRIDGE) resample_tables_chain(y, p.n_frames, p.width, prev, next);
    const int want = (out_value ? kResampleValue : 0) | (out_d1 ? kResampleD1 : 0) | (out_d2 ? kResampleD2 : 0);
    for (int32_t i = 0; i < p.n_out; ++i)
        for (int c = 0; c < p.width; ++c) {
            double v[3];
            resample_sample_der(y, prev, next, p, i, c, want, v);
            const int64_t e = (int64_t)i * p.width + c;
            if (out_value) out_value[e] = v[0];
            if (out_d1) out_d1[e] = v[1];
            if (out_d2) out_d2[e] = v[2];
        }
}

inline void resample_chain(const double *y, const ResampleParams &p, int32_t *prev, int32_t *next, double *out)
{
    resample_chain_der(y, p, prev, next, out, nullptr, nullptr);
}

}  // namespace seqik
