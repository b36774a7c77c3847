/*
 * seqik_sensitivity.h -- angle error bars: how the angles of the sequential leg fit move when the key points they were
 * fitted to move, the standard deviation that key-point noise gives every angle, and which joints sit on a limit
 * (libseqik_hip.so, gfx950).  Additive to ABI 7.
 *
 * seqik_jacobian.h answers how the key points move when the angles move.  These entry points answer the converse for
 * the sequential chain (kind 0): sens = d (fitted angle) / d (aligned key point), one GPU lane per leg-frame.  It is
 * NOT the pseudo-inverse of the Jacobian: the sequential fit is four small solves, in each of which 3 equations fit 2
 * unknowns (stage 4: 1), so the residual r does not vanish and the response of the optimum carries the residual-times-
 * curvature term of the Hessian; and a joint that sits on its limit does not move at all.
 *
 * Layouts (dense; kind as in seqik_fk.h):
 *   angles    [n_seq][n_legs][n_frames][7]        the solved angles, DOFS order (SEQIK_DOF_*), which for kind 0 is chain order
 *   pose      [n_seq][n_legs][n_frames][5][3]     the aligned key points the angles were fitted to (the solver's input)
 *   kp_sigma  [n_seq][n_legs][n_frames][4]        nullable: isotropic standard deviation of key points 1..4 (read for std)
 *   sens      [n_seq][n_legs][n_frames][7][4][3]  nullable: [DOF][k - 1][c] = d angle / d (aligned key point k, component c)
 *   std       [n_seq][n_legs][n_frames][7]        nullable, needs kp_sigma: std_j = sqrt(sum_k sigma_k^2 sum_c sens[j][k][c]^2)
 *   flags     [n_seq][n_legs][n_frames]           nullable, int32: bits 0..6 DOF held; bits 8..11 stage 1..4 not positive
 *                                                 definite; bit 16 non-finite input
 * At least one of sens, std, flags must be given.  legs[i].seg and legs[i].bounds are read.
 *
 * Definition.  Stage s = 1..4 fits f_s(q), key point s of the chain (FK rows 4, 6, 7, 8, leg-local), to the target t_s =
 * pose[s] - pose[0] over its own DOFs D_s = {0,1}, {2,3}, {4,5}, {6}; E_s is every DOF before them, r_s = f_s - t_s.  With
 * J_a = a_a x (f_s - o_a) as in seqik_jacobian.h and, for i = min(a, b), j = max(a, b),
 *     G_ab = J_a . J_b + r_s . (a_i x (a_j x (f_s - o_j)))          g_a = J_a . r_s
 *   1. own DOF a is HELD when (q_a - lb_a <= bound_tol and g_a > 0) or (ub_a - q_a <= bound_tol and g_a < 0); its row of
 *      sens is +0.0.  bound_tol <= 0 disables the rule.
 *   2. with F the own DOFs that are not held:  sens_F = G_FF^-1 (J_F^T [on key point s] - G_FE sens_E), by the 1 x 1 or 2 x 2
 *      closed form with plain / (host and device agree bit for bit).
 *   3. G_FF not positive definite (leading entry <= 0 or determinant <= 0): not a strict minimum; the rows of F are NaN
 *      and bit 8 + (s - 1) is set.  Later stages inherit the NaN through G_FE sens_E.
 * sens is block lower triangular: a stage-s DOF has +0.0 for key points > s, stored and never computed.  The values are
 * for the ALIGNED key points; for RAW key points the sensitivity is the alignment's scale x these values.
 * The full 7 x 7 covariance of a leg-frame is the caller's: sens diag(sigma^2) sens^T over the 12 coordinates.
 *
 * bound_tol: SEQIK_SENS_BOUND_TOL (1e-6 rad) is not derived; it sits in a gap of the distances to the nearest limit of
 * the solved angles of the shipped anipose recording (6000 frames per leg; tests/golden/anipose_shipped.npz):
 *     frames with an angle within   1e-3   1e-4   1e-6   1e-8   of a limit
 *     RF                             350    345    343    327
 *     LF                             243    243    242    182
 *
 * A leg-frame with a non-finite angle, key-point coordinate or (when std is given) sigma, or with |angle| >
 * SEQIK_ANGLE_MAX, gets 84 + 7 NaN and flags = bit 16 alone.  That is not an error and no other leg-frame is affected.
 * Return codes and seqik_last_error() as in seqik.h.  SEQIK_ERR_BAD_ARG, before anything touches HIP: n_legs outside
 * 1..8, a negative size, null angles / pose / legs, no output requested, std without kp_sigma, kind not 0 (kind 1, the
 * generic chain, fits seven angles to three coordinates: its optimum is not a function of the key points), a
 * non-finite segment length, more leg-frames than 672 bytes each can be addressed for.  A call with no leg-frames
 * returns SEQIK_OK without a launch.
 */
#ifndef SEQIK_SENSITIVITY_H
#define SEQIK_SENSITIVITY_H

#include "seqik_fk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SEQIK_SENS_BOUND_TOL 1e-6
#define SEQIK_SENS_FLAG_HELD(dof) (1 << (dof))
#define SEQIK_SENS_FLAG_NOT_PD(stage) (1 << (7 + (stage))) /* stage 1..4 */
#define SEQIK_SENS_FLAG_BAD_INPUT (1 << 16)

/* Host buffers: copies in, launches on a pooled stream of `device` (-1 = the calling thread's current device),
 * copies out and synchronises. */
int seqik_fit_sensitivity(const double *angles, const double *pose, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                          const SeqikLegParams *legs, int32_t kind, const double *kp_sigma, double bound_tol, double *sens,
                          double *std, int32_t *flags, int32_t device);

/* Device buffers: only enqueues the kernel on `hip_stream` (hipStream_t; NULL = the default stream) of the current
 * device; allocates nothing and does not synchronise. */
int seqik_fit_sensitivity_device(const double *d_angles, const double *d_pose, int64_t n_seq, int32_t n_legs,
                                 int64_t n_frames, const SeqikLegParams *legs, int32_t kind, const double *d_kp_sigma,
                                 double bound_tol, double *d_sens, double *d_std, int32_t *d_flags, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* SEQIK_SENSITIVITY_H */
