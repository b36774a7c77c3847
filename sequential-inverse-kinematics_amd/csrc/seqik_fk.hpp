// seqik_fk.hpp -- forward kinematics of one leg-frame from its joint angles (include/seqik_fk.h).
//
// The solvers write the stage-4 FK rows of a frame while they solve it (run_stage in seqik_core.hpp, run_generic in
// seqik_generic.hpp).  fk_leg_frame rebuilds the same 9x3 rows from the angles alone, with the same device functions in
// the same operation order, so that feeding a solver's angles back gives the solver's FK bit for bit:
//   rows 0-3  origin                       (leg_inverse_kinematics.py:279-282: the base and the inert links)
//   rows 4-5  coxa end  (after CTr_pitch)
//   row  6    femur end (after FTi_pitch)
//   row  7    tibia end (after TiTa_pitch)
//   row  8    claw
// each as `position + origin[a]`.  Both chain kinds share the layout; they differ in the order of the thorax-coxa links:
//   seq     (KinematicChainSeq, kinematic_chain.py:152-421):    yaw(X) pitch(Y) roll(Z) CTr_pitch CTr_roll FTi TiTa
//   generic (KinematicChainGeneric, kinematic_chain.py:442+):   roll(Z) yaw(X) pitch(Y) CTr_pitch CTr_roll FTi TiTa
#pragma once
#include "seqik_core.hpp"
#include "seqik_generic.hpp"
#include "../../include/seqik.h"
#include "../../include/seqik_fk.h"

namespace seqik {

enum : int { FK_KIND_SEQ = 0, FK_KIND_GENERIC = 1 };
constexpr int kFkMaxLegs = 8;  // the solver's kMaxLegs

// The angle domain of the entry points that take angles from outside (fk_leg_frame, link_frames_walk): finite and
// |x| <= SEQIK_ANGLE_MAX (include/seqik_fk.h).  sincos_cw turns rint(x * 2 / pi) into an int, which holds it only for
// |x| < 2^31 * pi / 2; inside the domain that number stays below 6.84e8.  The comparison is false for NaN and for
// +-inf, so it is the whole test.  The solvers do not need it: their angles lie inside validated bounds.
SEQIK_HD bool angle_in_domain(double x) { return fabs(x) <= SEQIK_ANGLE_MAX; }

// What the chains take from SeqikLegParams: the link translations, -seg[0..3] (negations, hence exactly the values
// make_leg_consts / make_generic_consts store).
struct FkLeg {
    double nseg[4];
};

inline void make_fk_leg(const SeqikLegParams &lp, FkLeg &fl)
{
    for (int i = 0; i < 4; ++i) fl.nseg[i] = -lp.seg[i];
}

// One leg-frame.  ang [7] in DOFS order, origin [3] (nullable: leg-local positions, origin 0), out [27].
// An angle outside the domain (non-finite, or |x| > SEQIK_ANGLE_MAX) makes all 27 values NaN (the chain itself is
// evaluated at 0 there).
template <int KIND>
SEQIK_HD void fk_leg_frame(const FkLeg &fl, const double *ang, const double *origin, double *out)
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
    double coxa_end[3], femur_end[3], tibia_end[3], claw[3];
    if constexpr (KIND == FK_KIND_SEQ) {
        // the translations of make_leg_consts (stage 1: 0, 0; stage 2: 0, -coxa; stage 3: 0, -femur; stage 4: -tibia,
        // last -tarsus); only these fields of the LegConst are read by build_prefix<4>
        LegConst lc;
        lc.st[0].tz_a = 0.0; lc.st[0].tz_b = 0.0;
        lc.st[1].tz_a = 0.0; lc.st[1].tz_b = fl.nseg[0];
        lc.st[2].tz_a = 0.0; lc.st[2].tz_b = fl.nseg[1];
        StageProblem<4> P;
        build_prefix<4>(P.pre, lc, x, 1, coxa_end);
        P.tz_a = fl.nseg[2]; P.tz_b = 0.0; P.tz_last = fl.nseg[3];
        double sa, ca;
        sincos_cw(x[SEQIK_DOF_TITA_PITCH], sa, ca);
        Frame after;
        frame_after_active<4>(P, sa, ca, 0.0, 1.0, after);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            femur_end[a] = P.pre.t[a];
            tibia_end[a] = after.t[a];
            claw[a] = after.r[3 * a + 2] * P.tz_last + after.t[a];
        }
    } else {
        GenericConst gc;
        gc.tz[0] = 0.0; gc.tz[1] = 0.0; gc.tz[2] = 0.0; gc.tz[3] = fl.nseg[0];
        gc.tz[4] = 0.0; gc.tz[5] = fl.nseg[1]; gc.tz[6] = fl.nseg[2];
        double sn[GN], cs[GN];
#pragma unroll
        for (int i = 0; i < GN; ++i) sincos_cw(x[generic_link_dof(i)], sn[i], cs[i]);  // = kGenericLinkDof[i]
        Frame e;
        generic_chain(gc, sn, cs, e, coxa_end, femur_end);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            tibia_end[a] = e.t[a];
            claw[a] = e.r[3 * a + 2] * fl.nseg[3] + e.t[a];
        }
    }
    const double nan = __builtin_nan("");
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int a = 0; a < 3; ++a) out[3 * i + a] = finite ? 0.0 + o[a] : nan;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        out[12 + a] = finite ? coxa_end[a] + o[a] : nan;
        out[15 + a] = finite ? coxa_end[a] + o[a] : nan;
        out[18 + a] = finite ? femur_end[a] + o[a] : nan;
        out[21 + a] = finite ? tibia_end[a] + o[a] : nan;
        out[24 + a] = finite ? claw[a] + o[a] : nan;
    }
}

// Euclidean distances of FK rows 4, 6, 7, 8 (as stored) from key points 1..4 of `pose` ([5][3]): numpy's
// np.linalg.norm order over three elements, sqrt((dx * dx + dy * dy) + dz * dz).
SEQIK_HD void fk_fit_distances(const double *fk, const double *pose, double *dist)
{
    const int rows[4] = {4, 6, 7, 8};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double dx = fk[3 * rows[k]] - pose[3 * (k + 1)];
        const double dy = fk[3 * rows[k] + 1] - pose[3 * (k + 1) + 1];
        const double dz = fk[3 * rows[k] + 2] - pose[3 * (k + 1) + 2];
        dist[k] = sqrt((dx * dx + dy * dy) + dz * dz);
    }
}

}  // namespace seqik
