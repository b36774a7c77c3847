/*
 * seqik_fk.h -- batched forward kinematics from joint angles (libseqik_hip.so, gfx950).
 *
 * The solvers of seqik.h write the forward kinematics of a frame while they solve it.  These entry points compute the
 * same rows from angles alone -- angles of an earlier run, resampled, filtered or edited angles -- one GPU lane per
 * leg-frame.  Fed a solver's own angles (and the same origin) they return the solver's FK bit for bit.
 *
 * Layouts are the solvers' own dense ones, so solver output can be passed straight back in:
 *   angles  [n_seq][n_legs][n_frames][7]     DOFS order (SEQIK_DOF_*)
 *   fk      [n_seq][n_legs][n_frames][9][3]  rows 0-3 origin, 4-5 coxa end, 6 femur end, 7 tibia end, 8 claw
 *   pose    [n_seq][n_legs][n_frames][5][3]  nullable: origin = key point 0 of each frame
 *   origin  [n_seq][n_legs][n_frames][3]     nullable: the origin of each leg-frame
 *   dist    [n_seq][n_legs][n_frames][4]     nullable, needs pose: |fk row 4, 6, 7, 8 - pose row 1, 2, 3, 4|
 * At most one of pose / origin; with neither the origin is 0 (leg-local positions).  With the fused alignment of the
 * solvers (SeqikAffine) their origin is template_coxa: pass it as `origin`.
 *
 * kind: 0 = the sequential chain (KinematicChainSeq: thorax-coxa links yaw(X), pitch(Y), roll(Z)), 1 = the generic
 * chain (KinematicChainGeneric: roll(Z), yaw(X), pitch(Y)).  The same angles give different positions under the two
 * kinds: pass the kind that produced them.  Only legs[i].seg is read.
 *
 * Angle domain: finite and |angle| <= SEQIK_ANGLE_MAX = 2^30 rad.  Inside it sin and cos of every angle are within
 * 2^-53 of the true values (within 1 ulp up to 1e7 rad), so unwrapped angles of any real recording are served as they
 * are.  A non-finite angle, or one beyond SEQIK_ANGLE_MAX, makes that leg-frame's 27 FK values (and its 4 distances)
 * NaN; it is not an error, and no other leg-frame is affected.  (Beyond 2^31 * pi / 2 the quadrant of the argument
 * reduction no longer fits its integer; the domain ends well before, at a power of two.)  sin(-0.0) is returned as
 * +0.0, so a zero entry of a result may differ in sign from numpy's; values never do.
 * Return codes and seqik_last_error() as in seqik.h.  SEQIK_ERR_BAD_ARG: n_legs outside 1..8, a negative size, null
 * angles / fk / legs, kind not 0 / 1, both pose and origin, dist without pose, a non-finite segment length.  A call
 * with no leg-frames returns SEQIK_OK without a launch.
 */
#ifndef SEQIK_FK_H
#define SEQIK_FK_H

#include "seqik.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SEQIK_FK_KIND_SEQ 0
#define SEQIK_FK_KIND_GENERIC 1
#define SEQIK_FK_MAX_LEGS 8
#define SEQIK_ANGLE_MAX 1073741824.0 /* 2^30 rad: the largest |angle| these entry points and seqik_frames.h evaluate */

/* Host buffers: copies in, launches on a pooled stream of `device` (-1 = the calling thread's current device),
 * copies out and synchronises. */
int seqik_forward_kinematics(const double *angles, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                             const SeqikLegParams *legs, int32_t kind, const double *pose, const double *origin,
                             double *fk, double *dist, int32_t device);

/* Device buffers: only enqueues the kernel on `hip_stream` (hipStream_t; NULL = the default stream) of the current
 * device; allocates nothing and does not synchronise. */
int seqik_forward_kinematics_device(const double *d_angles, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                                    const SeqikLegParams *legs, int32_t kind, const double *d_pose,
                                    const double *d_origin, double *d_fk, double *d_dist, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* SEQIK_FK_H */
