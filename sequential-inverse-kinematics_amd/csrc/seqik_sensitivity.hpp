// seqik_sensitivity.hpp -- how the angles of the sequential leg fit move when the key points they were fitted to move
// (include/seqik_sensitivity.h): the device rule of one leg-frame, host-runnable.
//
// The sequential fit is four small least-squares solves.  Stage s = 1..4 fits key point s (f_s: FK row 4 / 6 / 7 / 8,
// leg-local) to the target t_s = pose[s] - pose[0] over its own DOFs D_s = {0,1}, {2,3}, {4,5}, {6}, with the DOFs before
// them (E_s) held at what the earlier stages found.  At the optimum J_F^T r = 0 (r = f_s - t_s, F = the own DOFs that are
// free); differentiating that condition gives
//     S_F = G_FF^-1 ( J_F^T [on key point s]  -  G_FE S_E ),
//     G_ab = J_a . J_b + r . (a_i x (a_j x (f_s - o_j))),   i = min(a, b), j = max(a, b)
// with J_a = a_a x (f_s - o_a) the Jacobian column of seqik_leg_chain.hpp (a_a the world axis of DOF a, o_a its origin).
// G is the exact Hessian of the stage's cost: 3 equations fit 2 unknowns, the residual does not vanish, and the second
// term -- the exact second derivative of a revolute chain -- is not small next to the first.
//
// Held joints.  With g_a = J_a . r, own DOF a is held when (q_a - lb_a <= tol and g_a > 0) or (ub_a - q_a <= tol and
// g_a < 0): it sits on a limit and the cost pushes it outwards.  Its row of S is +0.0 and it is no member of F.
// tol <= 0 (or NaN) switches the rule off; a NaN limit never holds.
//
// The solve is the 1 x 1 or 2 x 2 closed form, plain products, sums, `/`:
//     det = G_aa G_bb - G_ab G_ab,   x_a = (G_bb y_a - G_ab y_b) / det,   x_b = (G_aa y_b - G_ab y_a) / det
// G_FF not positive definite (leading entry <= 0 or det <= 0; for one free DOF its diagonal entry <= 0; a NaN fails the
// test too): the rows of F are NaN and flag bit 8 + (s - 1) is set.  Later stages inherit the NaN through G_FE S_E for
// the key points before their own; the column of their own key point does not depend on S_E.  Every NaN stored is the
// one quiet NaN of __builtin_nan(""), so that records compare bit for bit across host and device.
//
// S[7][4][3] = d angle / d (aligned key point k, component c); block lower triangular: the row of a stage-s DOF holds +0.0
// for the key points after s, stored and never computed (sens_nonzero).  Every dot product is (x0 y0 + x1 y1) + x2 y2,
// every cross product that of seqik_leg_chain.hpp, G_FE S_E is summed over E ascending and only where S_E is not a
// structural zero.  std_j = sqrt(sum_k sigma_k^2 ((S_jk0^2 + S_jk1^2) + S_jk2^2)), k ascending up to the DOF's stage.
//
// Domain: an angle outside the domain of seqik_fk.hpp, a non-finite key-point coordinate or -- when std is asked for -- a
// non-finite sigma makes the 84 + 7 values NaN and the flags exactly SENS_FLAG_BAD_INPUT.  sqrt and / are the correctly
// rounded ones of host and device, so with -ffp-contract=off the rule run on the host and the kernel agree bit for bit.
#pragma once
#include <stdint.h>
#include <utility>

#include "seqik_jacobian.hpp"

namespace seqik {

constexpr int kSensRow = 84;  // doubles of sensitivity per leg-frame: 7 DOFs x 4 key points x 3 components
constexpr int kSensStd = 7;   // doubles of standard deviation per leg-frame
constexpr int kSensQuad = kSensRow / 4;  // 21 doubles: the quarter of a record one lane of the staged path holds
constexpr int32_t SENS_FLAG_NOT_PD0 = 1 << 8;      // << (stage - 1)
constexpr int32_t SENS_FLAG_BAD_INPUT = 1 << 16;

constexpr int sens_stage_of(int dof) { return dof / 2 + 1; }                        // 1..4
constexpr bool sens_nonzero(int dof, int k0) { return k0 < sens_stage_of(dof); }    // k0 = key point - 1

// G_ab of the stage whose residual is r, a <= b: J_a . J_b + r . (a_a x J_b)
SEQIK_HD double sens_hessian(const double *Ja, const double *Jb, const double *axis_a, const double *r)
{
    double h[3];
    chain_cross(h, axis_a, Jb);
    return chain_dot(Ja, Jb) + chain_dot(r, h);
}

SEQIK_HD bool sens_held(double q, double lb, double ub, double g, double tol)
{
    return tol > 0.0 && ((q - lb <= tol && g > 0.0) || (ub - q <= tol && g < 0.0));
}

// Stage ST = 1..4: fills the rows of its own DOFs in S (key points 1..ST) from the rows of the earlier stages -> the
// stage's flag bits.
template <int ST>
SEQIK_HD int32_t sens_stage(const JacChain &ch, const LegBounds &sb, const double *q, const double *pose, double tol,
                            double (&S)[7][4][3])
{
    constexpr int K0 = ST - 1, A = 2 * K0, B = A + 1, NE = A;
    constexpr bool TWO = ST < 4;
    const double nan = __builtin_nan("");
    double r[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = ch.p[K0][c] - (pose[3 * ST + c] - pose[c]);
    double Ja[3], Jb[3] = {0.0, 0.0, 0.0};
    jac_column<K0, A>(Ja, ch);
    if constexpr (TWO) jac_column<K0, B>(Jb, ch);
    // G_ae, G_be for the earlier DOFs e (the larger index is the own DOF's)
    double Gae[NE > 0 ? NE : 1], Gbe[NE > 0 ? NE : 1];
    if constexpr (NE > 0) {
        double Je[NE][3];
        if constexpr (NE > 0) jac_column<K0, 0>(Je[0], ch);
        if constexpr (NE > 1) jac_column<K0, 1>(Je[1], ch);
        if constexpr (NE > 2) jac_column<K0, 2>(Je[2], ch);
        if constexpr (NE > 3) jac_column<K0, 3>(Je[3], ch);
        if constexpr (NE > 4) jac_column<K0, 4>(Je[4], ch);
        if constexpr (NE > 5) jac_column<K0, 5>(Je[5], ch);
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            Gae[e] = sens_hessian(Je[e], Ja, ch.ax[e], r);
            Gbe[e] = TWO ? sens_hessian(Je[e], Jb, ch.ax[e], r) : 0.0;
        }
    }
    const double Gaa = sens_hessian(Ja, Ja, ch.ax[A], r);
    const double Gab = TWO ? sens_hessian(Ja, Jb, ch.ax[A], r) : 0.0;
    const double Gbb = TWO ? sens_hessian(Jb, Jb, ch.ax[TWO ? B : A], r) : 0.0;
    const bool held_a = sens_held(q[A], sb.lb[A], sb.ub[A], chain_dot(Ja, r), tol);
    const bool held_b = TWO ? sens_held(q[TWO ? B : A], sb.lb[TWO ? B : A], sb.ub[TWO ? B : A], chain_dot(Jb, r), tol) : true;
    const bool both = !held_a && !held_b;
    const double det = Gaa * Gbb - Gab * Gab;
    // positive definite on the free DOFs (nothing free: nothing to test)
    const bool pd = both ? (Gaa > 0.0 && det > 0.0) : !held_a ? Gaa > 0.0 : !held_b ? Gbb > 0.0 : true;
#pragma unroll
    for (int k = 0; k <= K0; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double ya, yb;
            if (k == K0) {
                ya = Ja[c];
                yb = Jb[c];
            } else {  // - G_FE S_E over the earlier DOFs whose row holds key point k + 1: e >= 2 k
                double sa = 0.0, sb_ = 0.0;
#pragma unroll
                for (int e = 2 * k; e < NE; ++e) {
                    sa = e == 2 * k ? Gae[e] * S[e][k][c] : sa + Gae[e] * S[e][k][c];
                    sb_ = e == 2 * k ? Gbe[e] * S[e][k][c] : sb_ + Gbe[e] * S[e][k][c];
                }
                ya = -sa;
                yb = -sb_;
            }
            const double xa = both ? (Gbb * ya - Gab * yb) / det : ya / Gaa;
            S[A][k][c] = held_a ? 0.0 : (pd && xa == xa) ? xa : nan;  // one NaN: inherited ones differ in sign and payload
            if constexpr (TWO) {
                const double xb = both ? (Gaa * yb - Gab * ya) / det : yb / Gbb;
                S[B][k][c] = held_b ? 0.0 : (pd && xb == xb) ? xb : nan;
            }
        }
    }
    int32_t flags = held_a ? 1 << A : 0;
    if constexpr (TWO) flags |= held_b ? 1 << B : 0;
    return flags | (pd ? 0 : SENS_FLAG_NOT_PD0 << K0);
}

// What one leg-frame's rule leaves behind: the computed part of S (the structural zeros are never touched), the flags
// and whether the inputs were inside the domain.
struct SensResult {
    double S[7][4][3];
    int32_t flags;
    bool finite;
};

// ang [7], pose [5][3], kp_sigma [4] nullable (read for the domain test only: given exactly when std is wanted).
SEQIK_HD void sens_leg_frame_rule(const FkLeg &fl, const LegBounds &sb, const double *ang, const double *pose,
                                  const double *kp_sigma, double tol, SensResult &res)
{
    double x[7], kp[15];
    bool finite = true;
#pragma unroll
    for (int d = 0; d < 7; ++d) {
        x[d] = ang[d];
        finite = finite && angle_in_domain(x[d]);
    }
#pragma unroll
    for (int i = 0; i < 15; ++i) {
        kp[i] = pose[i];
        finite = finite && is_finite(kp[i]);
    }
    if (kp_sigma) {
#pragma unroll
        for (int k = 0; k < 4; ++k) finite = finite && is_finite(kp_sigma[k]);
    }
    if (!finite) {
#pragma unroll
        for (int d = 0; d < 7; ++d) x[d] = 0.0;
    }
    JacChain ch;
    seq_chain_walk(fl, x, ch);
    int32_t flags = sens_stage<1>(ch, sb, x, kp, tol, res.S);
    flags |= sens_stage<2>(ch, sb, x, kp, tol, res.S);
    flags |= sens_stage<3>(ch, sb, x, kp, tol, res.S);
    flags |= sens_stage<4>(ch, sb, x, kp, tol, res.S);
    res.flags = finite ? flags : SENS_FLAG_BAD_INPUT;
    res.finite = finite;
}

template <int IDX, class Sink>
SEQIK_HD void sens_emit_one(Sink &sink, const SensResult &res)
{
    constexpr int D = IDX / 12, K0 = (IDX % 12) / 3, C = IDX % 3;
    const double nan = __builtin_nan("");
    if constexpr (sens_nonzero(D, K0)) sink.template put<IDX>(res.finite ? res.S[D][K0][C] : nan);
    else sink.template put<IDX>(res.finite ? 0.0 : nan);
}

// Hands the record to `sink.template put<IDX>(v)`, IDX = 12 * DOF + 3 * (k - 1) + component, each IDX once and in
// increasing order (the sinks of seqik_leg_chain.hpp).
template <class Sink, int... IDX>
SEQIK_HD void sens_emit_all(Sink &sink, const SensResult &res, std::integer_sequence<int, IDX...>)
{
    (sens_emit_one<IDX>(sink, res), ...);
}

template <class Sink>
SEQIK_HD void sens_emit(Sink &sink, const SensResult &res)
{
    sens_emit_all(sink, res, std::make_integer_sequence<int, kSensRow>{});
}

// std [7] from the computed part of S and the four sigmas
SEQIK_HD void sens_std(const SensResult &res, const double *kp_sigma, double *out)
{
    const double nan = __builtin_nan("");
#pragma unroll
    for (int d = 0; d < 7; ++d) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < d / 2 + 1) {
                const double *s = res.S[d][k];
                const double t = (kp_sigma[k] * kp_sigma[k]) * ((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
                acc = k == 0 ? t : acc + t;
            }
        }
        const double sd = sqrt(acc);
        out[d] = (res.finite && sd == sd) ? sd : nan;
    }
}

// One leg-frame.  sens [7][4][3], std [7], flags [1]: each nullable (std needs kp_sigma).
SEQIK_HD void sens_leg_frame(const FkLeg &fl, const LegBounds &sb, const double *ang, const double *pose,
                             const double *kp_sigma, double tol, double *sens, double *std_out, int32_t *flags)
{
    SensResult res;
    sens_leg_frame_rule(fl, sb, ang, pose, std_out ? kp_sigma : nullptr, tol, res);
    if (sens) {
        ArraySink sink{sens};
        sens_emit(sink, res);
    }
    if (std_out) sens_std(res, kp_sigma, std_out);
    if (flags) *flags = res.flags;
}

}  // namespace seqik
