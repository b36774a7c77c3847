// seqik_refine_sens.hpp -- how the angles that minimise the whole-leg fit move when the key points move
// (include/seqik_refine_sensitivity.h): the device rule of one leg-frame, host-runnable.
//
// The header states the rule; this file fixes its arithmetic so that the rule run on the host and the kernel agree bit
// for bit (-ffp-contract=off, correctly rounded sqrt and /):
//
//   chain     seq_chain_walk of seqik_leg_chain.hpp at the angles as they are (they are not clamped).
//   residual  refine_residual of seqik_refine.hpp: r[k][c] = w_k (f_k[c] - t_k[c]); a key point with w_k == 0 is not read.
//   H, g      pass 1, key point by key point and within a key point column by column, as seqik_refine.hpp forms A: the
//             column of DOF D for key point k is w_k (a_D x (f_k - o_D)) (jac_column); it adds J_D . r_k to g_D and, for the
//             columns i <= D of the same key point, J_i . J_D + r_k . (a_i x J_D) (sens_hessian of seqik_sensitivity.hpp) to
//             H_Di.  21 entries of J at most are held, never the 84; sums run over k ascending.  g has the bits of the g
//             of seqik_refine.hpp at the same angles.
//   held      sens_held of seqik_sensitivity.hpp.  grad = max over the free DOFs of |g_j| (none free: 0), divided by len^2,
//             len = ((seg_0 + seg_1) + seg_2) + seg_3.
//   factor    M = H with the rows and columns of held DOFs replaced by those of the identity; the 7 x 7 Cholesky
//             factorisation of seqik_refine.hpp's refine_solve in the same fixed order, without damping.  That function
//             masks, damps, factors and substitutes one right-hand side in one piece; the factor is needed here for twelve,
//             so this is a sibling (refsens_factor) and not a call.
//   solve     pass 2, one key point (three right-hand sides) at a time: the columns are formed again, b_D = w_k J_kD for a
//             free D that moves key point k and 0 otherwise, and
//                 y_i = (b_i - sum_{k<i} L_ik y_k) / L_ii;   x_i = (y_i - sum_{k>i} L_ki x_k) / L_ii  (k ascending)
//             sens[d][k][c] = held d: +0.0; a pivot not positive: NaN; w_k == 0: +0.0; otherwise x_d (a NaN: the one NaN).
//             The record is emitted key point by key point, so IDX = 12 d + 3 k + c does not arrive in increasing order:
//             the staged path stores through QuadAnySink below.
//   std       acc_d = sum_k (sigma_k sigma_k) ((s_0^2 + s_1^2) + s_2^2), k ascending, std_d = sqrt(acc_d).
#pragma once
#include <stdint.h>
#include <utility>

#include "seqik_refine.hpp"
#include "seqik_sensitivity.hpp"

namespace seqik {

constexpr int32_t REFSENS_FLAG_NOT_PD = 1 << 8;
constexpr int32_t REFSENS_FLAG_BAD_INPUT = 1 << 16;

// DOFs that move key point K0 + 1: 2, 4, 6, 7
constexpr int refsens_columns(int k0) { return k0 == 3 ? 7 : 2 * (k0 + 1); }

// A sink that forms no record.
struct NoSink {
    template <int IDX> SEQIK_HD void put(double) {}
};

// QuadSink for values that do not arrive in increasing IDX: clear() first, then one select per value.
template <int QUAD>
struct QuadAnySink {
    QuadSink<QUAD> &s;
    SEQIK_HD void clear()
    {
#pragma unroll
        for (int j = 0; j < QUAD; ++j) s.buf[j] = 0.0;
    }
    template <int IDX> SEQIK_HD void put(double v)
    {
        constexpr int Q = IDX / QUAD, J = IDX % QUAD;
        s.buf[J] = (s.q == Q) ? v : s.buf[J];
    }
};

// Column D of key point K0 + 1 into Jk[D], its share of g[D] and of row D of H (lower triangle, H[D][i], i <= D).
template <int K0, int D>
SEQIK_HD void refsens_column(const JacChain &ch, double w, const double *rk, double (&Jk)[7][3], double (&H)[7][7], double *g)
{
    constexpr bool FIRST = K0 == D / 2;  // the first key point DOF D moves
    double col[3];
    jac_column<K0, D>(col, ch);
#pragma unroll
    for (int c = 0; c < 3; ++c) Jk[D][c] = w * col[c];
    const double gd = chain_dot(Jk[D], rk);
    g[D] = FIRST ? gd : g[D] + gd;
#pragma unroll
    for (int i = 0; i <= D; ++i) {
        const double h = sens_hessian(Jk[i], Jk[D], ch.ax[i], rk);
        H[D][i] = FIRST ? h : H[D][i] + h;
    }
}

template <int K0, int... D>
SEQIK_HD void refsens_hessian_key_point(const JacChain &ch, double w, const double *rk, double (&H)[7][7], double *g,
                                        std::integer_sequence<int, D...>)
{
    double Jk[7][3];
    (refsens_column<K0, D>(ch, w, rk, Jk, H, g), ...);
}

// H (lower triangle) and g = J^T r at the chain `ch`
SEQIK_HD void refsens_hessian(const JacChain &ch, const double *w, const double (&r)[4][3], double (&H)[7][7], double *g)
{
    refsens_hessian_key_point<0>(ch, w[0], r[0], H, g, std::make_integer_sequence<int, 2>{});
    refsens_hessian_key_point<1>(ch, w[1], r[1], H, g, std::make_integer_sequence<int, 4>{});
    refsens_hessian_key_point<2>(ch, w[2], r[2], H, g, std::make_integer_sequence<int, 6>{});
    refsens_hessian_key_point<3>(ch, w[3], r[3], H, g, std::make_integer_sequence<int, 7>{});
}

// H -> its masked Cholesky factor, in place (lower triangle) -> whether every pivot was positive
SEQIK_HD bool refsens_factor(double (&M)[7][7], int held)
{
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const bool fi = !((held >> i) & 1);
#pragma unroll
        for (int j = 0; j < i; ++j) M[i][j] = (fi && !((held >> j) & 1)) ? M[i][j] : 0.0;
        M[i][i] = fi ? M[i][i] : 1.0;
    }
    bool pd = true;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        double s = M[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s = s - M[j][k] * M[j][k];
        pd = pd && (s > 0.0);
        const double l = sqrt(s);
        M[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < 7; ++i) {
            double v = M[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v = v - M[i][k] * M[j][k];
            M[i][j] = v / l;
        }
    }
    return pd;
}

// b_D of key point K0 + 1, three components: w J_kD for a free DOF that moves it, 0 otherwise
template <int K0, int D>
SEQIK_HD void refsens_rhs(const JacChain &ch, double w, int held, double (&b)[7][3])
{
    if constexpr (D < refsens_columns(K0)) {
        double col[3];
        jac_column<K0, D>(col, ch);
        const bool free = !((held >> D) & 1);
#pragma unroll
        for (int c = 0; c < 3; ++c) b[D][c] = free ? w * (w * col[c]) : 0.0;
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) b[D][c] = 0.0;
    }
}

template <int K0, int I, class Sink>
SEQIK_HD void refsens_put(Sink &sink, const double (&x)[7][3])
{
    sink.template put<12 * (I / 3) + 3 * K0 + I % 3>(x[I / 3][I % 3]);
}

// The three columns of key point K0 + 1: solve, select, emit, and their share of acc (sigma: four finite values).
template <int K0, bool RECORD, class Sink, int... D, int... I>
SEQIK_HD void refsens_key_point(const JacChain &ch, double w, const double (&L)[7][7], int held, bool pd, const double *sigma,
                                Sink &sink, double (&acc)[7], std::integer_sequence<int, D...>, std::integer_sequence<int, I...>)
{
    const double nan = __builtin_nan("");
    double b[7][3];
    (refsens_rhs<K0, D>(ch, w, held, b), ...);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            double v = b[i][c];
#pragma unroll
            for (int k = 0; k < i; ++k) v = v - L[i][k] * b[k][c];
            b[i][c] = v / L[i][i];
        }
#pragma unroll
        for (int i = 6; i >= 0; --i) {
            double v = b[i][c];
#pragma unroll
            for (int k = i + 1; k < 7; ++k) v = v - L[k][i] * b[k][c];
            b[i][c] = v / L[i][i];
        }
    }
#pragma unroll
    for (int d = 0; d < 7; ++d) {
        const bool h = (held >> d) & 1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double x = b[d][c];
            b[d][c] = h ? 0.0 : !pd ? nan : w == 0.0 ? 0.0 : x == x ? x : nan;
        }
        const double t = (sigma[K0] * sigma[K0]) * ((b[d][0] * b[d][0] + b[d][1] * b[d][1]) + b[d][2] * b[d][2]);
        acc[d] = K0 == 0 ? t : acc[d] + t;
    }
    if constexpr (RECORD) (refsens_put<K0, I>(sink, b), ...);
}

template <class Sink, int... IDX>
SEQIK_HD void refsens_put_nan(Sink &sink, std::integer_sequence<int, IDX...>)
{
    const double nan = __builtin_nan("");
    (sink.template put<IDX>(nan), ...);
}

// One leg-frame.  ang [7], pose [5][3], kp_weight [4] nullable, kp_sigma [4] nullable (read for the domain test when given,
// required when std_out is); the record goes to `sink` when RECORD; std_out [7], grad [1], flags [1]: each nullable.
template <bool RECORD, class Sink>
SEQIK_HD void refsens_rule(const FkLeg &fl, const LegBounds &sb, const double *ang, const double *pose,
                           const double *kp_weight, const double *kp_sigma, double tol, Sink &sink, double *std_out,
                           double *grad, int32_t *flags)
{
    const double nan = __builtin_nan("");
    double q[7], w[4], t[4][3], sg[4] = {0.0, 0.0, 0.0, 0.0};
    bool ok = true;
#pragma unroll
    for (int d = 0; d < 7; ++d) {
        q[d] = ang[d];
        ok = ok && angle_in_domain(q[d]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        w[k] = kp_weight ? kp_weight[k] : 1.0;
        ok = ok && is_finite(fl.nseg[k]) && is_finite(w[k]) && w[k] >= 0.0;
        if (kp_sigma) {
            sg[k] = kp_sigma[k];
            ok = ok && is_finite(sg[k]);
        }
    }
    double o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o[c] = pose[c];
        ok = ok && is_finite(o[c]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double v = 0.0;
            if (w[k] != 0.0) {  // a key point without weight is not read
                v = pose[3 * (k + 1) + c];
                ok = ok && is_finite(v);
                v = v - o[c];
            }
            t[k][c] = v;
        }
    }
    if (!ok) {
        if constexpr (RECORD) refsens_put_nan(sink, std::make_integer_sequence<int, kSensRow>{});
        if (std_out) {
#pragma unroll
            for (int d = 0; d < 7; ++d) std_out[d] = nan;
        }
        if (grad) *grad = nan;
        if (flags) *flags = REFSENS_FLAG_BAD_INPUT;
        return;
    }
    JacChain ch;
    double r[4][3], H[7][7], g[7];
    seq_chain_walk(fl, q, ch);
    refine_residual(ch, t, w, r);
    refsens_hessian(ch, w, r, H, g);
    int32_t held = 0;
    double gmax = 0.0;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const bool h = sens_held(q[j], sb.lb[j], sb.ub[j], g[j], tol);
        held |= h ? 1 << j : 0;
        const double a = fabs(g[j]);
        gmax = (!h && a > gmax) ? a : gmax;
    }
    const bool pd = refsens_factor(H, held);
    if (flags) *flags = held | (pd ? 0 : REFSENS_FLAG_NOT_PD);
    if (grad) {
        const double len = ((fl.nseg[0] + fl.nseg[1]) + fl.nseg[2]) + fl.nseg[3];  // minus the leg length; only its square is used
        const double gr = gmax / (len * len);
        *grad = gr == gr ? gr : nan;
    }
    if (!RECORD && !std_out) return;
    double acc[7];  // formed whether std is wanted or not (sigma 0 then): 28 products next to the 168 divisions of the solves
    constexpr std::make_integer_sequence<int, 7> dofs{};
    constexpr std::make_integer_sequence<int, 21> entries{};
    refsens_key_point<0, RECORD>(ch, w[0], H, held, pd, sg, sink, acc, dofs, entries);
    refsens_key_point<1, RECORD>(ch, w[1], H, held, pd, sg, sink, acc, dofs, entries);
    refsens_key_point<2, RECORD>(ch, w[2], H, held, pd, sg, sink, acc, dofs, entries);
    refsens_key_point<3, RECORD>(ch, w[3], H, held, pd, sg, sink, acc, dofs, entries);
    if (std_out) {
#pragma unroll
        for (int d = 0; d < 7; ++d) {
            const double sd = sqrt(acc[d]);
            std_out[d] = sd == sd ? sd : nan;
        }
    }
}

// One leg-frame into arrays.  sens [7][4][3], std_out [7], grad [1], flags [1]: each nullable (std_out needs kp_sigma,
// which is read exactly when std_out is given).
SEQIK_HD void refsens_leg_frame(const FkLeg &fl, const LegBounds &sb, const double *ang, const double *pose,
                                const double *kp_weight, const double *kp_sigma, double tol, double *sens, double *std_out,
                                double *grad, int32_t *flags)
{
    const double *sigma = std_out ? kp_sigma : nullptr;
    if (sens) {
        ArraySink sink{sens};
        refsens_rule<true>(fl, sb, ang, pose, kp_weight, sigma, tol, sink, std_out, grad, flags);
    } else {
        NoSink sink;
        refsens_rule<false>(fl, sb, ang, pose, kp_weight, sigma, tol, sink, std_out, grad, flags);
    }
}

}  // namespace seqik
