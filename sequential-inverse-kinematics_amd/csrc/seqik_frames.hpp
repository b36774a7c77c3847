// seqik_frames.hpp -- the frames (position AND orientation) of all nine links of one leg-frame from its joint angles
// (include/seqik_frames.h).
//
// What IKPy's Chain.forward_kinematics(q, full_kinematics=True) returns for the whole-leg chain: frame i = the product of
// the link matrices 0 .. i, each T(0, 0, tz) . R(axis, angle).  Link order = the order of Chain.links:
//   seq     (create_leg_chain_stage_4): base, ThC_yaw (X), ThC_pitch (Y), ThC_roll (Z), CTr_pitch (Y, -coxa),
//           CTr_roll (Z), FTi_pitch (Y, -femur), TiTa_pitch (Y, -tibia), Claw (-tarsus)
//   generic (KinematicChainGeneric):    base, ThC_roll (Z), ThC_yaw (X), ThC_pitch (Y), then the same
// with the base and claw variables 0.  Per link the top three rows of its 4x4 frame are emitted, row-major: 12 values, 108
// per leg-frame (the fourth row is always 0 0 0 1).
//
// Contract with fk_leg_frame (seqik_fk.hpp), bit for bit: the translation column of link i is FK row i -- origin added,
// NaN rule included.  The chain is walked once with frame_mul_link, the one device function build_prefix<4>,
// frame_after_active<4> and generic_chain are made of, in their link order and with their translations, so every
// cumulative frame here IS the frame they pass through; the column takes the values fk_leg_frame stores (rows 0-3 the
// origin, row 5 the coxa end of row 4, the claw as r[.][2] * -tarsus + t) with the same `+ origin[a]`.  The rotation
// blocks do not depend on the origin.  An axis rotation appended on the right changes two columns of the block only,
// which is how frame_mul_link computes it.
#pragma once
#include "seqik_leg_chain.hpp"

namespace seqik {

constexpr int kFramesLinks = 9;
constexpr int kFramesRow = 108;  // doubles per leg-frame: 9 links x 3 rows x 4 columns

// Walks the chain and hands every value to `sink.template put<IDX>(v)`, IDX = 12 * link + 4 * row + column, each IDX
// exactly once and in increasing order.  The sink decides where a value goes (an array, global memory, the registers of
// the lane that owns that part of the record), so no caller has to hold 108 values at once.
template <int LINK, class Sink>
SEQIK_HD void frames_emit(Sink &sink, const Frame &f, const double *col, bool finite)
{
    const double nan = __builtin_nan("");
    sink.template put<12 * LINK + 0>(finite ? f.r[0] : nan);
    sink.template put<12 * LINK + 1>(finite ? f.r[1] : nan);
    sink.template put<12 * LINK + 2>(finite ? f.r[2] : nan);
    sink.template put<12 * LINK + 3>(finite ? col[0] : nan);
    sink.template put<12 * LINK + 4>(finite ? f.r[3] : nan);
    sink.template put<12 * LINK + 5>(finite ? f.r[4] : nan);
    sink.template put<12 * LINK + 6>(finite ? f.r[5] : nan);
    sink.template put<12 * LINK + 7>(finite ? col[1] : nan);
    sink.template put<12 * LINK + 8>(finite ? f.r[6] : nan);
    sink.template put<12 * LINK + 9>(finite ? f.r[7] : nan);
    sink.template put<12 * LINK + 10>(finite ? f.r[8] : nan);
    sink.template put<12 * LINK + 11>(finite ? col[2] : nan);
}

template <int KIND, class Sink>
SEQIK_HD void link_frames_walk(const FkLeg &fl, const double *ang, const double *origin, Sink &sink)
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
    const double o[3] = {origin ? origin[0] : 0.0, origin ? origin[1] : 0.0, origin ? origin[2] : 0.0};
    // thorax-coxa links 1-3: the DOF and the axis of each differ between the kinds, their translations are 0
    constexpr int AX1 = KIND == FK_KIND_SEQ ? AXIS_X : AXIS_Z;
    constexpr int AX2 = KIND == FK_KIND_SEQ ? AXIS_Y : AXIS_X;
    constexpr int AX3 = KIND == FK_KIND_SEQ ? AXIS_Z : AXIS_Y;
    constexpr int D1 = KIND == FK_KIND_SEQ ? SEQIK_DOF_THC_YAW : SEQIK_DOF_THC_ROLL;
    constexpr int D2 = KIND == FK_KIND_SEQ ? SEQIK_DOF_THC_PITCH : SEQIK_DOF_THC_YAW;
    constexpr int D3 = KIND == FK_KIND_SEQ ? SEQIK_DOF_THC_ROLL : SEQIK_DOF_THC_PITCH;
    double sn, cs, col[3], coxa_col[3];
    Frame a, b;
    frame_identity(a);
#pragma unroll
    for (int k = 0; k < 3; ++k) col[k] = 0.0 + o[k];  // FK rows 0-3
    frames_emit<0>(sink, a, col, finite);
    sincos_cw(x[D1], sn, cs);
    frame_mul_link<AX1>(b, a, sn, cs, 0.0);
    frames_emit<1>(sink, b, col, finite);
    sincos_cw(x[D2], sn, cs);
    frame_mul_link<AX2>(a, b, sn, cs, 0.0);
    frames_emit<2>(sink, a, col, finite);
    sincos_cw(x[D3], sn, cs);
    frame_mul_link<AX3>(b, a, sn, cs, 0.0);
    frames_emit<3>(sink, b, col, finite);
    sincos_cw(x[SEQIK_DOF_CTR_PITCH], sn, cs);
    frame_mul_link<AXIS_Y>(a, b, sn, cs, fl.nseg[0]);
#pragma unroll
    for (int k = 0; k < 3; ++k) coxa_col[k] = a.t[k] + o[k];  // FK rows 4 and 5
    frames_emit<4>(sink, a, coxa_col, finite);
    sincos_cw(x[SEQIK_DOF_CTR_ROLL], sn, cs);
    frame_mul_link<AXIS_Z>(b, a, sn, cs, 0.0);
    frames_emit<5>(sink, b, coxa_col, finite);
    sincos_cw(x[SEQIK_DOF_FTI_PITCH], sn, cs);
    frame_mul_link<AXIS_Y>(a, b, sn, cs, fl.nseg[1]);
#pragma unroll
    for (int k = 0; k < 3; ++k) col[k] = a.t[k] + o[k];  // FK row 6
    frames_emit<6>(sink, a, col, finite);
    sincos_cw(x[SEQIK_DOF_TITA_PITCH], sn, cs);
    frame_mul_link<AXIS_Y>(b, a, sn, cs, fl.nseg[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) col[k] = b.t[k] + o[k];  // FK row 7
    frames_emit<7>(sink, b, col, finite);
#pragma unroll
    for (int k = 0; k < 3; ++k) col[k] = (b.r[3 * k + 2] * fl.nseg[3] + b.t[k]) + o[k];  // FK row 8; the claw does not rotate
    frames_emit<8>(sink, b, col, finite);
}

constexpr int kFramesQuad = kFramesRow / 4;  // 27 doubles: the quarter of a record one lane of the staged path holds
using FramesQuadSink = QuadSink<kFramesQuad>;  // the unit's own name of it: host harnesses written against it still build

// One leg-frame.  ang [7] in DOFS order, origin [3] (nullable: leg-local positions), out [9][3][4].
// An angle outside the domain (non-finite, or |x| > SEQIK_ANGLE_MAX) makes all 108 values NaN.
template <int KIND>
SEQIK_HD void link_frames_leg_frame(const FkLeg &fl, const double *ang, const double *origin, double *out)
{
    ArraySink sink{out};
    link_frames_walk<KIND>(fl, ang, origin, sink);
}

}  // namespace seqik
