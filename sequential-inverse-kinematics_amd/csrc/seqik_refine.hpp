// seqik_refine.hpp -- whole-leg refinement (include/seqik_refine.h): the device rule of one leg-frame, host-runnable.
//
// From a start q (normally the sequential fit's angles) a bounded Levenberg-Marquardt minimises c(q) = r . r over all
// seven angles at once, r = (w_k (f_k(q) - t_k)), k = 1..4: f_k the key points of the chain (FK rows 4, 6, 7, 8,
// leg-local), t_k = pose[k] - pose[0], w_k the key-point weights.  The header states the rule; this file fixes its
// arithmetic so that the rule run on the host and the kernel agree bit for bit (-ffp-contract=off, correctly rounded
// sqrt and /):
//
//   chain     seq_chain_walk of seqik_leg_chain.hpp: world axes a_j, key points f_k.
//   residual  r[k][c] = w_k * (f_k[c] - t_k[c]);  c = ((r_1 . r_1 + r_2 . r_2) + r_3 . r_3) + r_4 . r_4, every dot product
//             (x0 y0 + x1 y1) + x2 y2.  A key point with w_k == 0 is not read: t_k = 0, r_k = 0.
//   J, A, g   key point by key point, and within a key point column by column: the column of DOF j for key point k is
//             w_k * (a_j x (f_k - o_j)) (jac_column; only where it is not a structural zero, j < 2 k, stage 4: j < 7).
//             It adds J_j . r_k to g_j and J_i . J_j to A_ji for the columns i <= j of the same key point, which are
//             the only ones held: 21 entries of J at most, never the 84.  Sums run over k ascending.
//   held      DOF j is held when (q_j <= lb_j and g_j > 0) or (q_j >= ub_j and g_j < 0).
//   step      M = A with d_j = (A_jj <= 0 ? DBL_MIN : A_jj) times lambda added to the diagonal; the rows and columns of held
//             DOFs are replaced by those of the identity and their right-hand side by 0, so that the 7 x 7 Cholesky
//             factorisation below, in one fixed order with compile-time indices, solves exactly the system of the free
//             DOFs (the products with the masked entries are zeros) and leaves delta = 0 for the held ones:
//                 for j:  s = M_jj - sum_{k<j} L_jk^2 (k ascending);  not s > 0: rejection;  L_jj = sqrt(s)
//                         for i > j:  L_ij = (M_ij - sum_{k<j} L_ik L_jk) / L_jj
//                 y_i = (b_i - sum_{k<i} L_ik y_k) / L_ii;   delta_i = (y_i - sum_{k>i} L_ki delta_k) / L_ii  (k ascending)
//             q'_j = clamp(q_j + delta_j) for free j.  A trial with an angle outside the domain of seqik_fk.hpp (only
//             possible with limits that wide) or a cost that is not smaller (a NaN is not smaller) is a rejection.
//
//   stall     a trial that moved (q' != q) and whose cost is not smaller but within ftol * c of the current one ends the
//             lane with reason 1 at the current point: the cost no longer tells the two points apart.  Without this the
//             rule mislabels converged lanes.  Convergence is linear here (the residual does not vanish), so the step
//             after a decrease just above ftol * c is worth ~1e-15 c at the default ftol = 1e-14 -- the size of the
//             cost's own rounding (2 r . df with the chain's |df| ~ 1e-16) -- and whether it is accepted is chance;
//             when it is not, no lambda helps and the lane would report reason 2 at scipy's cost (measured: 3 of the 575
//             frames of the shipped recording the tests use).
//
// Order of the stop tests at the top of an iteration, after g and the held set of the current point are known (they give
// the held bits of `info` whatever the reason): an accepted step whose decrease was <= ftol * c (reason 1), max_iter
// accepted steps (reason 4), the gradient test (reason 0).  Damping exhausted (reason 2) leaves from the retry loop.
// The retry loop ends: lambda grows fourfold from >= 1e-12 to > 1e12 in at most 40 rejections.
#pragma once
#include <stdint.h>
#include <utility>

#include "seqik_leg_chain.hpp"

namespace seqik {

constexpr int kRefineCost = 2;
constexpr int32_t REFINE_STOP_GRADIENT = 0, REFINE_STOP_DECREASE = 1, REFINE_STOP_DAMPING = 2, REFINE_STOP_MAX_ITER = 4;
constexpr int32_t REFINE_BAD_INPUT = 1 << 24;
constexpr double kRefineLambda0 = 1e-3, kRefineLambdaMin = 1e-12, kRefineLambdaMax = 1e12;
constexpr double kRefineTiny = 2.2250738585072014e-308;  // the smallest normal double

struct RefineOptions {
    double gtol, ftol;
    int32_t max_iter, pad_;
};

SEQIK_HD double refine_clamp(double x, double lb, double ub) { return x < lb ? lb : (x > ub ? ub : x); }

// r = w (f - t) and c = r . r
SEQIK_HD double refine_residual(const JacChain &ch, const double (&t)[4][3], const double *w, double (&r)[4][3])
{
    double c = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int i = 0; i < 3; ++i) r[k][i] = w[k] * (ch.p[k][i] - t[k][i]);
        const double s = chain_dot(r[k], r[k]);
        c = k == 0 ? s : c + s;
    }
    return c;
}

// Column D of key point K0 + 1 into Jk[D], its share of g[D] and of row D of A (lower triangle, A[D][i], i <= D).
template <int K0, int D>
SEQIK_HD void refine_column(const JacChain &ch, double w, const double *rk, double (&Jk)[7][3], double (&A)[7][7], double *g)
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
        const double a = chain_dot(Jk[i], Jk[D]);
        A[D][i] = FIRST ? a : A[D][i] + a;
    }
}

template <int K0, int... D>
SEQIK_HD void refine_key_point(const JacChain &ch, double w, const double *rk, double (&A)[7][7], double *g,
                               std::integer_sequence<int, D...>)
{
    double Jk[7][3];
    (refine_column<K0, D>(ch, w, rk, Jk, A, g), ...);
}

// A = J^T J (lower triangle) and g = J^T r at the chain `ch`
SEQIK_HD void refine_normal_equations(const JacChain &ch, const double *w, const double (&r)[4][3], double (&A)[7][7],
                                      double *g)
{
    refine_key_point<0>(ch, w[0], r[0], A, g, std::make_integer_sequence<int, 2>{});
    refine_key_point<1>(ch, w[1], r[1], A, g, std::make_integer_sequence<int, 4>{});
    refine_key_point<2>(ch, w[2], r[2], A, g, std::make_integer_sequence<int, 6>{});
    refine_key_point<3>(ch, w[3], r[3], A, g, std::make_integer_sequence<int, 7>{});
}

// (A + lambda diag(d)) delta = -g on the DOFs that are not in `held` -> whether every pivot was positive
SEQIK_HD bool refine_solve(const double (&A)[7][7], const double *g, int held, double lambda, double *delta)
{
    double M[7][7], y[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const bool fi = !((held >> i) & 1);
#pragma unroll
        for (int j = 0; j < i; ++j) M[i][j] = (fi && !((held >> j) & 1)) ? A[i][j] : 0.0;
        const double d = A[i][i] <= 0.0 ? kRefineTiny : A[i][i];
        M[i][i] = fi ? A[i][i] + lambda * d : 1.0;
        y[i] = fi ? -g[i] : 0.0;
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
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        double v = y[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v = v - M[i][k] * y[k];
        y[i] = v / M[i][i];
    }
#pragma unroll
    for (int i = 6; i >= 0; --i) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < 7; ++k) v = v - M[k][i] * delta[k];
        delta[i] = v / M[i][i];
    }
    return pd;
}

// One leg-frame.  ang [7], pose [5][3], kp_weight [4] nullable; ang_out [7] (may be ang), cost [2] nullable, info [1]
// nullable.
SEQIK_HD void refine_leg_frame(const FkLeg &fl, const LegBounds &sb, const double *ang, const double *pose,
                               const double *kp_weight, const RefineOptions &opt, double *ang_out, double *cost,
                               int32_t *info)
{
    double q[7], w[4], t[4][3];
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
        const double nan = __builtin_nan("");
#pragma unroll
        for (int d = 0; d < 7; ++d) ang_out[d] = nan;
        if (cost) cost[0] = cost[1] = nan;
        if (info) *info = REFINE_BAD_INPUT;
        return;
    }
#pragma unroll
    for (int d = 0; d < 7; ++d) q[d] = refine_clamp(q[d], sb.lb[d], sb.ub[d]);
    JacChain ch;
    double r[4][3];
    seq_chain_walk(fl, q, ch);
    double c = refine_residual(ch, t, w, r);
    const double c0 = c;
    const double len = ((fl.nseg[0] + fl.nseg[1]) + fl.nseg[2]) + fl.nseg[3];  // minus the leg length; only its square is used
    const double gbar = opt.gtol * (len * len);
    double lambda = kRefineLambda0;
    int32_t iters = 0, reason, held;
    bool last = false;
#pragma unroll 1
    for (;;) {
        double A[7][7], g[7];
        refine_normal_equations(ch, w, r, A, g);
        held = 0;
        bool small = true;  // of the free DOFs' gradient entries (none free: true)
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const bool h = (q[j] <= sb.lb[j] && g[j] > 0.0) || (q[j] >= sb.ub[j] && g[j] < 0.0);
            held |= h ? 1 << j : 0;
            small = small && (h || fabs(g[j]) <= gbar);
        }
        if (last) {
            reason = REFINE_STOP_DECREASE;
            break;
        }
        if (iters >= opt.max_iter) {
            reason = REFINE_STOP_MAX_ITER;
            break;
        }
        if (small) {
            reason = REFINE_STOP_GRADIENT;
            break;
        }
        bool accepted = false, stalled = false;
#pragma unroll 1
        while (!accepted && !stalled && lambda <= kRefineLambdaMax) {
            double delta[7], qn[7];
            bool usable = refine_solve(A, g, held, lambda, delta), moved = false;
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                qn[j] = ((held >> j) & 1) ? q[j] : refine_clamp(q[j] + delta[j], sb.lb[j], sb.ub[j]);
                usable = usable && angle_in_domain(qn[j]);
                moved = moved || qn[j] != q[j];
            }
            if (usable) {
                JacChain cn;
                double rn[4][3];
                seq_chain_walk(fl, qn, cn);
                const double c_new = refine_residual(cn, t, w, rn);
                if (c_new < c) {
                    accepted = true;
                    last = c - c_new <= opt.ftol * c;
                    c = c_new;
                    ch = cn;
#pragma unroll
                    for (int j = 0; j < 7; ++j) q[j] = qn[j];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
#pragma unroll
                        for (int i = 0; i < 3; ++i) r[k][i] = rn[k][i];
                    }
                } else {
                    stalled = moved && c_new - c <= opt.ftol * c;  // the cost no longer tells the two points apart
                }
            }
            if (accepted) {
                ++iters;
                lambda = lambda / 3.0;
                lambda = lambda < kRefineLambdaMin ? kRefineLambdaMin : lambda;
            } else if (!stalled) {
                lambda = lambda * 4.0;
            }
        }
        if (!accepted) {
            reason = stalled ? REFINE_STOP_DECREASE : REFINE_STOP_DAMPING;
            break;
        }
    }
#pragma unroll
    for (int d = 0; d < 7; ++d) ang_out[d] = q[d];
    if (cost) {
        cost[0] = c0;
        cost[1] = c;
    }
    if (info) *info = held | (reason << 8) | (iters << 16);
}

}  // namespace seqik
