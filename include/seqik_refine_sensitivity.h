/*
 * seqik_refine_sensitivity.h -- error bars of the whole-leg refinement: how the angles that minimise the whole-leg fit
 * (seqik_refine.h) move when the key points move, the standard deviation that key-point noise gives every angle, which
 * joints are held on a limit, and whether the angles are a minimum at all (libseqik_hip.so, gfx950).  Additive to ABI 7.
 *
 * seqik_sensitivity.h answers the same questions for the sequential fit; its quantity is the response of four separate
 * one- or two-angle solves and is block lower triangular.  In the whole-leg fit every angle answers to every key point:
 * sens here is a full 7 x 12 matrix, and the optimum is a different function of the key points.  The values are the
 * whole-leg fit's response ONLY at angles that minimise that fit -- the output of seqik_refine_legs; `grad` tells whether
 * the angles passed in do.  One GPU lane per leg-frame, FP64; the sequential chain (kind 0) only.
 *
 * Layouts (dense; those of seqik_sensitivity.h and seqik_refine.h):
 *   angles     [n_seq][n_legs][n_frames][7]        the refined angles, DOFS order (SEQIK_DOF_*); they are NOT clamped
 *   pose       [n_seq][n_legs][n_frames][5][3]     the aligned key points the angles were fitted to
 *   kp_weight  [n_seq][n_legs][n_frames][4]        nullable (all weights 1): the weights w_k the fit was made with
 *   kp_sigma   [n_seq][n_legs][n_frames][4]        nullable: isotropic standard deviation of key points 1..4 (read for std)
 *   sens       [n_seq][n_legs][n_frames][7][4][3]  nullable: [DOF][k - 1][c] = d angle / d (aligned key point k, component c)
 *   std        [n_seq][n_legs][n_frames][7]        nullable, needs kp_sigma: std_j = sqrt(sum_k sigma_k^2 sum_c sens[j][k][c]^2)
 *   grad       [n_seq][n_legs][n_frames]           nullable: max_F |g_j| / (seg_0 + seg_1 + seg_2 + seg_3)^2, the left side of
 *                                                  the gradient test of seqik_refine.h at these angles (no DOF free: 0)
 *   flags      [n_seq][n_legs][n_frames]           nullable, int32: bits 0..6 DOF held; bit 8 not a strict minimum; bit
 *                                                  16 bad input
 * At least one of sens, std, grad, flags must be given.  legs[i].seg and legs[i].bounds are read.
 *
 * Definition.  t_k = pose[k] - pose[0], f_k(q) = key point k of the chain, r_k = w_k (f_k - t_k), J_k = w_k a_j x (f_k - o_j)
 * (3 x 7, structural zeros never computed) and g = J^T r = sum_k J_k^T r_k are exactly those of seqik_refine.h.  For
 * i = min(a, b), j = max(a, b),
 *     H_ab = sum_k [ J_ka . J_kb + w_k r_k . (a_i x (a_j x (f_k - o_j))) ]
 * the second term only where both DOFs move key point k (the structural pattern of seqik_refine.h); it is the exact
 * second derivative of a revolute chain of seqik_sensitivity.h.  H is the exact Hessian of r . r / 2: twelve equations
 * fit seven unknowns, the residual does not vanish, and the second term is not small next to the first.
 *   1. DOF a is HELD when (q_a - lb_a <= bound_tol and g_a > 0) or (ub_a - q_a <= bound_tol and g_a < 0) -- the wording of
 *      seqik_sensitivity.h, the same default SEQIK_SENS_BOUND_TOL; bound_tol = 0 disables the rule.  A held row of sens
 *      is +0.0 and its flag bit (0..6) is set.  F = the DOFs that are not held.
 *   2. At a minimum g_F = 0.  The target enters r_k as -w_k t_k, so d g / d t_k = -w_k J_k^T, and differentiating g_F = 0
 *      gives H_FF dq_F - w_k J_k,F^T dt_k = 0:
 *          sens_F[.][k][c] = H_FF^-1 (w_k J_k,F,c)
 *      (with all weights 1: H_FF^-1 J_F^T).  Multiplying every weight by the same factor leaves sens unchanged: H and the
 *      right-hand side both carry its square.
 *   3. H_FF is factored by Cholesky in the fixed order of seqik_refine.h (rows and columns of held DOFs replaced by the
 *      identity's), plain sqrt and /.  A pivot that is not positive: the angles are not a strict minimum; every entry of the
 *      rows of F is the one quiet NaN and bit 8 is set.
 *   4. A key point with weight exactly 0 is not read (it may be NaN); its columns of sens are +0.0 (in rows that are
 *      NaN by rule 3 they are NaN).
 *   5. std_j = sqrt(sum_k sigma_k^2 sum_c sens[j][k][c]^2), as in seqik_sensitivity.h: 0 for a held joint.
 *   6. Bad input: rule 1 of seqik_refine.h (a non-finite angle or |angle| > SEQIK_ANGLE_MAX, a non-finite or negative
 *      weight, a non-finite coordinate of pose[0] or of a key point whose weight is not 0), or -- when std is given -- a
 *      non-finite sigma.  sens, std and grad of that leg-frame are NaN, flags is bit 16 alone.  Not an error; no other
 *      leg-frame is affected.
 * Every NaN stored is the one quiet NaN, so records compare by bits.  The full covariance of a leg-frame's angles is the
 * caller's: sens diag(sigma^2) sens^T over the 12 coordinates.  The values are for the ALIGNED key points; for RAW key
 * points the sensitivity is the alignment's scale x these values.
 *
 * Return codes and seqik_last_error() as in seqik.h.  SEQIK_ERR_BAD_ARG, before anything touches HIP: n_legs outside
 * 1..8, a negative size, null angles / pose / legs, no output requested, std without kp_sigma, kind not 0 (kind 1, the
 * generic chain, fits seven angles to three coordinates: its optimum is not a function of the key points), a non-finite
 * segment length, a non-finite or negative bound_tol, more leg-frames than 672 bytes each can be addressed for.  A call
 * with no leg-frames returns SEQIK_OK without a launch.
 */
#ifndef SEQIK_REFINE_SENSITIVITY_H
#define SEQIK_REFINE_SENSITIVITY_H

#include "seqik_sensitivity.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SEQIK_REFSENS_FLAG_HELD(dof) (1 << (dof))
#define SEQIK_REFSENS_FLAG_NOT_PD (1 << 8)
#define SEQIK_REFSENS_FLAG_BAD_INPUT (1 << 16)

/* Host buffers: copies in, launches on a pooled stream of `device` (-1 = the calling thread's current device),
 * copies out and synchronises. */
int seqik_refine_sensitivity(const double *angles, const double *pose, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                             const SeqikLegParams *legs, int32_t kind, const double *kp_weight, const double *kp_sigma,
                             double bound_tol, double *sens, double *std, double *grad, int32_t *flags, int32_t device);

/* Device buffers: only enqueues the kernel on `hip_stream` (hipStream_t; NULL = the default stream) of the current
 * device; allocates nothing and does not synchronise.  `legs` is host memory. */
int seqik_refine_sensitivity_device(const double *d_angles, const double *d_pose, int64_t n_seq, int32_t n_legs,
                                    int64_t n_frames, const SeqikLegParams *legs, int32_t kind, const double *d_kp_weight,
                                    const double *d_kp_sigma, double bound_tol, double *d_sens, double *d_std,
                                    double *d_grad, int32_t *d_flags, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* SEQIK_REFINE_SENSITIVITY_H */
