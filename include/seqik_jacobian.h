/*
 * seqik_jacobian.h -- batched key-point Jacobians of the legs from joint angles, the conditioning of the stage solves and
 * the key-point velocities (libseqik_hip.so, gfx950).  Additive to ABI 7.
 *
 * seqik_fk.h answers "where is every key point, given the angles".  These entry points answer how the key points move
 * when the angles move (jac, and vel = jac . qdot for given joint rates), and how well each solve determined its angles
 * (sigma: the singular values of the block of jac the solve works with), one GPU lane per leg-frame.
 *
 * Layouts (dense, the solvers' own for angles; kind as in seqik_fk.h):
 *   angles  [n_seq][n_legs][n_frames][7]        DOFS order (SEQIK_DOF_*)
 *   qdot    [n_seq][n_legs][n_frames][7]        nullable: joint rates in the same order (read for vel only)
 *   jac     [n_seq][n_legs][n_frames][4][3][7]  nullable: [k - 1][component][DOF] = d (key point k) / d (angle of DOF);
 *                                               key points 1..4 = FK rows 4, 6, 7, 8 (coxa, femur, tibia end, claw);
 *                                               the last index is in SEQIK_DOF_* order for BOTH kinds, not in link order
 *   sigma   [n_seq][n_legs][n_frames][8]        nullable, see below
 *   vel     [n_seq][n_legs][n_frames][4][3]     nullable, needs qdot: the velocity of key point k, jac . qdot
 * At least one of jac, sigma, vel must be given.  Only legs[i].seg is read.
 *
 * jac[k - 1][.][dof(j)] = a_j x (p_k - o_j): a_j the world axis of joint j (the column of its axis in the rotation block
 * of link j's frame of seqik_frames.h), o_j that frame's translation column, p_k the translation column of link 4 / 6 /
 * 7 / 8, all leg-local: the Jacobian does not depend on the origin of the leg, and there is no origin parameter.
 * Entries that are zero for every angle are stored as +0.0: the joints behind key point k, and (k = 1, ThC_roll) for
 * kind 0, (k = 2, CTr_roll) and (k = 3, TiTa_pitch) for both kinds.  Nonzero pattern, row k by DOF:
 *   kind 0   1100000 / 1111000 / 1111110 / 1111111          kind 1   1110000 / 1111000 / 1111110 / 1111111
 *
 * sigma, kind 0: per stage s = 1..4 the pair (sigma_max, sigma_min) at [2 (s - 1)], [2 (s - 1) + 1] of the block stage s
 * of the sequential solve sees: key point s by the stage's own DOFs -- (ThC_yaw, ThC_pitch), (ThC_roll, CTr_pitch),
 * (CTr_roll, FTi_pitch), (TiTa_pitch); stage 4 has one column and both entries are its norm.  A sigma_min that is small
 * next to sigma_max says that the stage's two angles are not both determined by its key point (a kinematic singularity).
 * sigma_min is |u x v| / sigma_max of the block's columns u, v (0 when sigma_max is 0), which keeps it down to rounding
 * level.  sigma, kind 1: [0..2] the singular values of the claw's 3 x 7 block, descending (one-sided Jacobi, 6 sweeps);
 * [3..7] are NaN and carry no meaning.
 *
 * Angle domain as in seqik_fk.h: a non-finite angle, or one with |angle| > SEQIK_ANGLE_MAX, makes that leg-frame's 84 +
 * 8 + 12 values NaN.  A non-finite entry among a leg-frame's seven qdot values makes its 12 velocities NaN and nothing
 * else.  Neither is an error, and no other leg-frame is affected.
 * Return codes and seqik_last_error() as in seqik.h.  SEQIK_ERR_BAD_ARG, before anything touches HIP: n_legs outside
 * 1..8, a negative size, null angles / legs, no output requested, vel without qdot, kind not 0 / 1, a non-finite segment
 * length, more leg-frames than 672 bytes each can be addressed for.  A call with no leg-frames returns SEQIK_OK without a
 * launch.
 */
#ifndef SEQIK_JACOBIAN_H
#define SEQIK_JACOBIAN_H

#include "seqik_fk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SEQIK_JAC_KEY_POINTS 4

/* Host buffers: copies in, launches on a pooled stream of `device` (-1 = the calling thread's current device),
 * copies out and synchronises. */
int seqik_leg_jacobians(const double *angles, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                        const SeqikLegParams *legs, int32_t kind, const double *qdot, double *jac, double *sigma,
                        double *vel, int32_t device);

/* Device buffers: only enqueues the kernel on `hip_stream` (hipStream_t; NULL = the default stream) of the current
 * device; allocates nothing and does not synchronise. */
int seqik_leg_jacobians_device(const double *d_angles, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                               const SeqikLegParams *legs, int32_t kind, const double *d_qdot, double *d_jac,
                               double *d_sigma, double *d_vel, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* SEQIK_JACOBIAN_H */
