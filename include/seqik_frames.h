/*
 * seqik_frames.h -- batched link frames from joint angles (libseqik_hip.so, gfx950).
 *
 * seqik_fk.h gives the POSITION of every link of a leg from its joint angles.  These entry points give the whole frame
 * of every link, position and orientation: what IKPy's Chain.forward_kinematics(q, full_kinematics=True) returns for
 * the whole-leg chain, for whole batches, one GPU lane per leg-frame.
 *
 * Layouts (dense, the solvers' own for angles):
 *   angles  [n_seq][n_legs][n_frames][7]        DOFS order (SEQIK_DOF_*)
 *   origin  [n_seq][n_legs][n_frames][3]        nullable: the origin of each leg-frame; absent = 0 (leg-local frames)
 *   frames  [n_seq][n_legs][n_frames][9][3][4]  per link the top three rows of its 4x4 frame in the chain's base frame,
 *                                               row-major; the fourth row is always 0 0 0 1 and is not stored
 * Link order = the order of Chain.links of the chain the kind stands for (kind as in seqik_fk.h):
 *   0  sequential chain: base, ThC_yaw (X), ThC_pitch (Y), ThC_roll (Z), CTr_pitch (Y), CTr_roll (Z), FTi_pitch (Y),
 *                        TiTa_pitch (Y), Claw
 *   1  generic chain:    base, ThC_roll (Z), ThC_yaw (X), ThC_pitch (Y), then the same
 * Frame i is the product of the link matrices 0 .. i, each T(0, 0, tz) . R(axis, angle): tz = -seg[0] (coxa) for
 * CTr_pitch, -seg[1] (femur) for FTi_pitch, -seg[2] (tibia) for TiTa_pitch, -seg[3] (tarsus) for the claw, 0 for the
 * other links.  The base and claw variables are 0.  Only legs[i].seg is read.
 *
 * The translation column frames[..][i][a][3] equals row i, component a of seqik_forward_kinematics for the same angles,
 * kind and origin, bit for bit (the origin is added to the column; the rotation blocks do not depend on it).
 *
 * Angle domain as in seqik_fk.h: a non-finite angle, or one with |angle| > SEQIK_ANGLE_MAX (2^30 rad), makes that
 * leg-frame's 108 values NaN; it is not an error, and no other leg-frame is affected.  sin(-0.0) is returned as +0.0,
 * so a zero entry may differ in sign from IKPy's; values never do.
 * Return codes and seqik_last_error() as in seqik.h.  SEQIK_ERR_BAD_ARG: n_legs outside 1..8, a negative size, null
 * angles / frames / legs, kind not 0 / 1, a non-finite segment length, more leg-frames than 864 bytes each can be
 * addressed for.  A call with no leg-frames returns SEQIK_OK without a launch.
 */
#ifndef SEQIK_FRAMES_H
#define SEQIK_FRAMES_H

#include "seqik_fk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SEQIK_FRAMES_LINKS 9

/* Host buffers: copies in, launches on a pooled stream of `device` (-1 = the calling thread's current device),
 * copies out and synchronises. */
int seqik_link_frames(const double *angles, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                      const SeqikLegParams *legs, int32_t kind, const double *origin, double *frames, int32_t device);

/* Device buffers: only enqueues the kernel on `hip_stream` (hipStream_t; NULL = the default stream) of the current
 * device; allocates nothing and does not synchronise. */
int seqik_link_frames_device(const double *d_angles, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                             const SeqikLegParams *legs, int32_t kind, const double *d_origin, double *d_frames,
                             void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* SEQIK_FRAMES_H */
