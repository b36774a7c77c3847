// seqik_jacobian.hpp -- the key-point Jacobian of one leg-frame from its joint angles, the conditioning of the stage solves
// and the key-point velocities (include/seqik_jacobian.h).
//
// The chain of seqik_frames.hpp is walked once, leg-local (no origin: the Jacobian does not depend on it), with
// frame_mul_link in its link order.  Every joint j leaves two things behind: its world axis a_j -- the column of its axis
// in the rotation block of link j's frame, which the link's own rotation does not change -- and its origin o_j, the
// frame's translation column.  The key points p_1 .. p_4 are the translation columns of links 4, 6, 7 and the claw (FK
// rows 4, 6, 7, 8).  The column of joint j for key point k is
//     jac[k - 1][.][dof(j)] = a_j x (p_k - o_j),      (a x d)_0 = a_1 d_2 - a_2 d_1, cyclic; plain products, no fma
// with the third index in SEQIK_DOF_* order for BOTH kinds (not link order).  The three thorax-coxa joints sit at the chain's
// base (o = 0: the lever arm is p_k itself), CTr_pitch and CTr_roll at p_1, FTi_pitch at p_2, TiTa_pitch at p_3.
//
// Structural zeros are +0.0 and never computed (kJacNonzero, bit d of row k - 1): the joints behind key point k; (k = 1,
// ThC_roll) of the sequential chain, (k = 2, CTr_roll) and (k = 3, TiTa_pitch) of both -- a roll about the segment that
// ends in the key point, or a joint that sits in it.
//
// sigma[8].  Sequential chain: per stage s = 1..4 the pair (sigma_max, sigma_min) of the block its solve sees, key point
// s by the stage's own DOFs (yaw, pitch), (ThC_roll, CTr_pitch), (CTr_roll, FTi_pitch), (TiTa_pitch).  For a 3 x 2 block
// [u v]:  sigma_max^2 = (|u|^2 + |v|^2) / 2 + sqrt(((|u|^2 - |v|^2) / 2)^2 + (u.v)^2),  sigma_min = |u x v| / sigma_max
// (0 when sigma_max is 0): the product of the two singular values is the area |u x v|, which keeps sigma_min down to
// u * sigma_max where the small eigenvalue of the Gram matrix is lost below sqrt(u) * sigma_max.  Stage 4 has one column:
// both entries are its norm.  Generic chain: sigma[0..2] = the singular values of the claw's 3 x 7 block, descending, by
// one-sided (Hestenes) Jacobi on its three rows: kJacobiSweeps = 6 sweeps of the pairs (0,1), (0,2), (1,2), always all of
// them, no convergence test; sigma[3..7] = NaN.
//
// vel[4][3] = J . qdot, summed over the nonzero pattern only, DOFs ascending, plain products and sums.
//
// Domain: an angle outside the domain of seqik_fk.hpp makes all 84 + 8 + 12 values NaN; a non-finite qdot entry makes the
// 12 velocities NaN and nothing else.  sqrt and / are the correctly rounded ones of host and device, so with
// -ffp-contract=off the rule run on the host and the kernel agree bit for bit.
#pragma once
#include <utility>

#include "seqik_leg_chain.hpp"

namespace seqik {

constexpr int kJacRow = 84;     // doubles of Jacobian per leg-frame: 4 key points x 3 components x 7 DOFs
constexpr int kJacSigma = 8;    // doubles of conditioning per leg-frame
constexpr int kJacVel = 12;     // doubles of key-point velocity per leg-frame
constexpr int kJacobiSweeps = 6;

// nonzero pattern: bit d of [kind][k - 1] is set where (key point k, DOF d) is not a structural zero
constexpr int kJacNonzero[2][4] = {{0x03, 0x0F, 0x3F, 0x7F}, {0x07, 0x0F, 0x3F, 0x7F}};
constexpr bool jac_nonzero(int kind, int k0, int d) { return (kJacNonzero[kind][k0] >> d) & 1; }

template <int KIND, int IDX, class Sink>
SEQIK_HD void jac_emit_one(Sink &sink, const JacChain &ch, bool finite)
{
    constexpr int K0 = IDX / 21, C = (IDX % 21) / 7, D = IDX % 7;
    const double nan = __builtin_nan("");
    if constexpr (jac_nonzero(KIND, K0, D)) sink.template put<IDX>(finite ? jac_entry<K0, C, D>(ch) : nan);
    else sink.template put<IDX>(finite ? 0.0 : nan);
}

template <int KIND, class Sink, int... IDX>
SEQIK_HD void jac_emit_all(Sink &sink, const JacChain &ch, bool finite, std::integer_sequence<int, IDX...>)
{
    (jac_emit_one<KIND, IDX>(sink, ch, finite), ...);
}

// Walks the chain and hands every value of the record to `sink.template put<IDX>(v)`, IDX = 21 * (k - 1) + 7 * component
// + DOF, each IDX exactly once and in increasing order (the sink decides where a value goes, as in link_frames_walk, so
// no caller has to hold 84 values).  Returns whether the angles lie inside the domain.
template <int KIND, class Sink>
SEQIK_HD bool leg_jacobian_walk(const FkLeg &fl, const double *ang, Sink &sink)
{
    double x[7];
    bool finite = true;
#pragma unroll
    for (int d = 0; d < 7; ++d) {
        x[d] = ang[d];
        finite = finite && angle_in_domain(x[d]);
    }
    if (!finite) {
#pragma unroll
        for (int d = 0; d < 7; ++d) x[d] = 0.0;
    }
    constexpr int AX1 = KIND == FK_KIND_SEQ ? AXIS_X : AXIS_Z;
    constexpr int AX2 = KIND == FK_KIND_SEQ ? AXIS_Y : AXIS_X;
    constexpr int AX3 = KIND == FK_KIND_SEQ ? AXIS_Z : AXIS_Y;
    constexpr int D1 = KIND == FK_KIND_SEQ ? SEQIK_DOF_THC_YAW : SEQIK_DOF_THC_ROLL;
    constexpr int D2 = KIND == FK_KIND_SEQ ? SEQIK_DOF_THC_PITCH : SEQIK_DOF_THC_YAW;
    constexpr int D3 = KIND == FK_KIND_SEQ ? SEQIK_DOF_THC_ROLL : SEQIK_DOF_THC_PITCH;
    JacChain ch;
    double sn, cs;
    Frame a, b;
    frame_identity(a);
    sincos_cw(x[D1], sn, cs);
    frame_mul_link<AX1>(b, a, sn, cs, 0.0);
    jac_axis<AX1>(ch.ax[D1], b);
    sincos_cw(x[D2], sn, cs);
    frame_mul_link<AX2>(a, b, sn, cs, 0.0);
    jac_axis<AX2>(ch.ax[D2], a);
    sincos_cw(x[D3], sn, cs);
    frame_mul_link<AX3>(b, a, sn, cs, 0.0);
    jac_axis<AX3>(ch.ax[D3], b);
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
    jac_emit_all<KIND>(sink, ch, finite, std::make_integer_sequence<int, kJacRow>{});
    return finite;
}

constexpr int kJacQuad = kJacRow / 4;  // 21 doubles: the quarter of a record one lane of the staged path holds
using JacArraySink = ArraySink;  // the unit's own names of the sinks: host harnesses written against them still build
using JacQuadSink = QuadSink<kJacQuad>;

SEQIK_HD double jac_dot7(const double *a, const double *b)
{
    double s = a[0] * b[0];
#pragma unroll
    for (int i = 1; i < 7; ++i) s = s + a[i] * b[i];
    return s;
}

// One Hestenes rotation of the rows p and q (7 entries each): afterwards they are orthogonal.
SEQIK_HD void jacobi_rotate_rows(double *p, double *q)
{
    const double alpha = jac_dot7(p, p), beta = jac_dot7(q, q), gamma = jac_dot7(p, q);
    const double zeta = (beta - alpha) / (2.0 * gamma);
    double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    t = (gamma == 0.0) ? 0.0 : t;  // already orthogonal (zeta is +-inf or NaN there)
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const double pi = p[i], qi = q[i];
        p[i] = c * pi - s * qi;
        q[i] = s * pi + c * qi;
    }
}

// (sigma_max, sigma_min) of the 3 x 2 block [u v]
SEQIK_HD void sigma_pair(const double *u, const double *v, double *out)
{
    const double uu = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2];
    const double vv = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    const double uv = (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2];
    const double m = (uu + vv) / 2.0, d = (uu - vv) / 2.0;
    const double smax = sqrt(m + sqrt(d * d + uv * uv));
    const double cx = u[1] * v[2] - u[2] * v[1], cy = u[2] * v[0] - u[0] * v[2], cz = u[0] * v[1] - u[1] * v[0];
    const double area = sqrt((cx * cx + cy * cy) + cz * cz);
    out[0] = smax;
    out[1] = (smax == 0.0) ? 0.0 : area / smax;
}

// Takes from the walk what sigma and vel need -- 21 entries and 12 running sums -- so that neither needs the record.
// blk: sequential chain [stage - 1][column][component] (stage 4: column 0 only); generic chain the claw's rows,
// [component][DOF].
template <int KIND>
struct JacReduceSink {
    double q[7];
    double blk[21];
    double vel[kJacVel];
    template <int IDX> SEQIK_HD void put(double v)
    {
        constexpr int K0 = IDX / 21, C = (IDX % 21) / 7, D = IDX % 7;
        if constexpr (KIND == FK_KIND_SEQ) {
            if constexpr (D == 2 * K0 || (D == 2 * K0 + 1 && K0 < 3)) blk[6 * K0 + 3 * (D - 2 * K0) + C] = v;
        } else {
            if constexpr (K0 == 3) blk[7 * C + D] = v;
        }
        if constexpr (jac_nonzero(KIND, K0, D)) {
            if constexpr (D == 0) vel[3 * K0 + C] = v * q[0];
            else vel[3 * K0 + C] = vel[3 * K0 + C] + v * q[D];
        }
    }
    // qdot nullable: no velocities wanted
    SEQIK_HD void begin(const double *qdot)
    {
#pragma unroll
        for (int d = 0; d < 7; ++d) q[d] = qdot ? qdot[d] : 0.0;
    }
    // sigma [8], vel_out [12]: each nullable
    SEQIK_HD void finish(bool finite, double *sigma, double *vel_out)
    {
        const double nan = __builtin_nan("");
        if (sigma) {
            double s[kJacSigma];
            if constexpr (KIND == FK_KIND_SEQ) {
#pragma unroll
                for (int st = 0; st < 3; ++st) sigma_pair(blk + 6 * st, blk + 6 * st + 3, s + 2 * st);
                const double *w = blk + 18;
                s[6] = s[7] = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
            } else {
#pragma unroll 1
                for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
                    jacobi_rotate_rows(blk, blk + 7);
                    jacobi_rotate_rows(blk, blk + 14);
                    jacobi_rotate_rows(blk + 7, blk + 14);
                }
                double s0 = sqrt(jac_dot7(blk, blk)), s1 = sqrt(jac_dot7(blk + 7, blk + 7));
                double s2 = sqrt(jac_dot7(blk + 14, blk + 14)), lo;
                lo = s0 < s1 ? s0 : s1; s0 = s0 < s1 ? s1 : s0; s1 = lo;
                lo = s1 < s2 ? s1 : s2; s1 = s1 < s2 ? s2 : s1; s2 = lo;
                lo = s0 < s1 ? s0 : s1; s0 = s0 < s1 ? s1 : s0; s1 = lo;
                s[0] = s0; s[1] = s1; s[2] = s2;
#pragma unroll
                for (int i = 3; i < kJacSigma; ++i) s[i] = nan;
            }
#pragma unroll
            for (int i = 0; i < kJacSigma; ++i) sigma[i] = finite ? s[i] : nan;
        }
        if (vel_out) {
            bool qfinite = finite;
#pragma unroll
            for (int d = 0; d < 7; ++d) qfinite = qfinite && is_finite(q[d]);
#pragma unroll
            for (int i = 0; i < kJacVel; ++i) vel_out[i] = qfinite ? vel[i] : nan;
        }
    }
};

// A record sink and the reduction in one walk (either may be compiled out).
template <int KIND, bool JAC, bool RED, class RecordSink>
struct JacBothSink {
    RecordSink rec;
    JacReduceSink<KIND> red;
    template <int IDX> SEQIK_HD void put(double v)
    {
        if constexpr (JAC) rec.template put<IDX>(v);
        if constexpr (RED) red.template put<IDX>(v);
    }
};

// One leg-frame.  ang [7] in DOFS order, qdot [7] nullable; jac [4][3][7], sigma [8], vel [4][3]: each nullable (vel needs
// qdot).
template <int KIND>
SEQIK_HD void leg_jacobian_leg_frame(const FkLeg &fl, const double *ang, const double *qdot, double *jac, double *sigma,
                                     double *vel)
{
    double scratch[kJacRow];
    JacBothSink<KIND, true, true, ArraySink> sink;
    sink.rec.out = jac ? jac : scratch;
    sink.red.begin(qdot);
    const bool finite = leg_jacobian_walk<KIND>(fl, ang, sink);
    sink.red.finish(finite, sigma, qdot ? vel : nullptr);
}

}  // namespace seqik
