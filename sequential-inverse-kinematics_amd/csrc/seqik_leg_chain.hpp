// seqik_leg_chain.hpp -- what the units built on the cumulative frames of the nine-link leg chain share: link frames
// (seqik_frames.hpp), leg Jacobians (seqik_jacobian.hpp), fit sensitivity (seqik_sensitivity.hpp) and whole-leg
// refinement (seqik_refine.hpp).  Device rules, host-runnable, no HIP runtime.  Frames and Jacobians keep their own walks:
// on a shared one two per-lane kernels lost a third of their rate (EXPERIMENTS.md, "Leg maps: one column, ...").
// Arithmetic: (a x d)_c = a[c+1] d[c+2] - a[c+2] d[c+1], cyclic; x . y = (x0 y0 + x1 y1) + x2 y2; plain products, no fma.
#pragma once
#include "seqik_fk.hpp"

namespace seqik {

// ---- what Jacobians, sensitivity and refinement keep of the chain, leg-local: the world axis of every DOF and the four
// key points (the header of seqik_jacobian.hpp says what they are) ----
struct JacChain {
    double ax[7][3];  // by DOF
    double p[4][3];   // key points 1..4
};

template <int AXIS>
SEQIK_HD void jac_axis(double *ax, const Frame &f)
{
#pragma unroll
    for (int i = 0; i < 3; ++i) ax[i] = f.r[3 * i + AXIS];
}

// The walk of the sequential chain for sensitivity and refinement: leg_jacobian_walk<FK_KIND_SEQ> (seqik_jacobian.hpp)
// without its prologue and its 84 entries, the same frame_mul_link calls in the same order.  x [7] inside the angle domain.
SEQIK_HD void seq_chain_walk(const FkLeg &fl, const double *x, JacChain &ch)
{
    double sn, cs;
    Frame a, b;
    frame_identity(a);
    sincos_cw(x[SEQIK_DOF_THC_YAW], sn, cs);
    frame_mul_link<AXIS_X>(b, a, sn, cs, 0.0);
    jac_axis<AXIS_X>(ch.ax[SEQIK_DOF_THC_YAW], b);
    sincos_cw(x[SEQIK_DOF_THC_PITCH], sn, cs);
    frame_mul_link<AXIS_Y>(a, b, sn, cs, 0.0);
    jac_axis<AXIS_Y>(ch.ax[SEQIK_DOF_THC_PITCH], a);
    sincos_cw(x[SEQIK_DOF_THC_ROLL], sn, cs);
    frame_mul_link<AXIS_Z>(b, a, sn, cs, 0.0);
    jac_axis<AXIS_Z>(ch.ax[SEQIK_DOF_THC_ROLL], b);
    sincos_cw(x[SEQIK_DOF_CTR_PITCH], sn, cs);
    frame_mul_link<AXIS_Y>(a, b, sn, cs, fl.nseg[0]);
    jac_axis<AXIS_Y>(ch.ax[SEQIK_DOF_CTR_PITCH], a);
#pragma unroll
    for (int k = 0; k < 3; ++k) ch.p[0][k] = a.t[k];  // coxa end; CTr_roll (translation 0) sits in it too
    sincos_cw(x[SEQIK_DOF_CTR_ROLL], sn, cs);
    frame_mul_link<AXIS_Z>(b, a, sn, cs, 0.0);
    jac_axis<AXIS_Z>(ch.ax[SEQIK_DOF_CTR_ROLL], b);
    sincos_cw(x[SEQIK_DOF_FTI_PITCH], sn, cs);
    frame_mul_link<AXIS_Y>(a, b, sn, cs, fl.nseg[1]);
    jac_axis<AXIS_Y>(ch.ax[SEQIK_DOF_FTI_PITCH], a);
#pragma unroll
    for (int k = 0; k < 3; ++k) ch.p[1][k] = a.t[k];  // femur end
    sincos_cw(x[SEQIK_DOF_TITA_PITCH], sn, cs);
    frame_mul_link<AXIS_Y>(b, a, sn, cs, fl.nseg[2]);
    jac_axis<AXIS_Y>(ch.ax[SEQIK_DOF_TITA_PITCH], b);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ch.p[2][k] = b.t[k];                                // tibia end
        ch.p[3][k] = b.r[3 * k + 2] * fl.nseg[3] + b.t[k];  // claw (it does not rotate)
    }
}

template <int C>
SEQIK_HD double chain_cross_entry(const double *a, const double *d)
{
    constexpr int C1 = (C + 1) % 3, C2 = (C + 2) % 3;
    return a[C1] * d[C2] - a[C2] * d[C1];
}

SEQIK_HD void chain_cross(double *out, const double *a, const double *d)
{
    out[0] = chain_cross_entry<0>(a, d);
    out[1] = chain_cross_entry<1>(a, d);
    out[2] = chain_cross_entry<2>(a, d);
}

SEQIK_HD double chain_dot(const double *x, const double *y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

// The column of DOF D for key point K0 + 1 is a_D x (p_k - o_D), third index in SEQIK_DOF_* order for BOTH kinds.  The
// lever arm p_k - o_D: the three thorax-coxa joints sit at the chain's base (o = 0: the lever arm is p_k itself),
// CTr_pitch and CTr_roll at p_1, FTi_pitch at p_2, TiTa_pitch at p_3.
template <int K0, int D>
SEQIK_HD void jac_lever(double *lev, const JacChain &ch)
{
    constexpr int O = D <= SEQIK_DOF_THC_ROLL ? -1 : D <= SEQIK_DOF_CTR_ROLL ? 0 : D == SEQIK_DOF_FTI_PITCH ? 1 : 2;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if constexpr (O < 0) lev[c] = ch.p[K0][c];
        else lev[c] = ch.p[K0][c] - ch.p[O][c];
    }
}

// Component C of that column, and all three; only called where the entry is not a structural zero.
template <int K0, int C, int D>
SEQIK_HD double jac_entry(const JacChain &ch)
{
    double lev[3];
    jac_lever<K0, D>(lev, ch);
    return chain_cross_entry<C>(ch.ax[D], lev);
}

template <int K0, int D>
SEQIK_HD void jac_column(double *J, const JacChain &ch)
{
    double lev[3];
    jac_lever<K0, D>(lev, ch);
    chain_cross(J, ch.ax[D], lev);
}

// ---- what sensitivity and refinement read of a leg besides the segment lengths: the limits of the seven DOFs ----
struct LegBounds {
    double lb[7], ub[7];
};

inline void make_leg_bounds(const SeqikLegParams &lp, LegBounds &lb)
{
    for (int d = 0; d < 7; ++d) {
        lb.lb[d] = lp.bounds[d][0];
        lb.ub[d] = lp.bounds[d][1];
    }
}

// (the names of the two while only the sensitivity unit had them: host harnesses written against them still build)
using SensBounds = LegBounds;
inline void make_sens_bounds(const SeqikLegParams &lp, SensBounds &sb) { make_leg_bounds(lp, sb); }

struct LegBoundsTable {
    LegBounds b[kFkMaxLegs];  // entries past n_legs repeat leg 0
    void fill(int32_t n_legs, const SeqikLegParams *legs)
    {
        for (int l = 0; l < kFkMaxLegs; ++l) make_leg_bounds(legs[l < n_legs ? l : 0], b[l]);
    }
};

// ---- record sinks: a rule hands every value of its record to `sink.template put<IDX>(v)`, each IDX exactly once and in
// increasing order, and the sink decides where it goes: an array or global memory, value by value ----
struct ArraySink {
    double *out;
    template <int IDX> SEQIK_HD void put(double v) { out[IDX] = v; }
};

// Keeps quarter `q` of a record of 4 * QUAD doubles, [QUAD q, QUAD q + QUAD): the sink of the staged path, where four lanes
// share a record (staged_quad_passes, seqik_leg_map.hpp).  IDX is a constant at every call: one select per value, no indexing.
template <int QUAD>
struct QuadSink {
    int q;
    double buf[QUAD];
    template <int IDX> SEQIK_HD void put(double v)
    {
        constexpr int Q = IDX / QUAD, J = IDX % QUAD;
        if constexpr (Q == 0) buf[J] = v;  // the first value offered for slot J; a later quarter's replaces it
        else buf[J] = (q == Q) ? v : buf[J];
    }
};

}  // namespace seqik
