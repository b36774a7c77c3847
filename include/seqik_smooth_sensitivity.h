/*
 * seqik_smooth_sensitivity.h -- error bars of the smoothed trajectory: how the angles that minimise the trajectory fit
 * (seqik_smooth.h) move when the key points of ANY frame move, the standard deviation that key-point noise in all frames
 * gives every angle, which joints are held on a limit, and whether the angles are a minimum at all (libseqik_hip.so,
 * gfx950).  Additive to ABI 7.
 *
 * seqik_refine_sensitivity.h answers these questions for the per-frame whole-leg fit.  The trajectory fit couples the
 * frames: the penalty makes an angle stiffer against the noise of its own frame and lets it answer to the noise of its
 * neighbours.  The Hessian of the fit is block tridiagonal, one 7 x 7 block row per frame; the blocks of its inverse and
 * the covariance of every frame's angles follow from serial sweeps over the frames, O(N) 7 x 7 operations, with no dense
 * N x N object and no truncation.  The values are the fit's response ONLY at angles that minimise it -- the output of
 * seqik_smooth_legs; `grad` tells whether the angles passed in do.  FP64; the sequential chain (kind 0) only.
 *
 * Layouts (dense), R = [n_seq][n_legs][n_frames], W = half_width (0..SEQIK_SMOOTHSENS_MAX_HALF_WIDTH):
 *   angles     R[7]               the smoothed angles, DOFS order (SEQIK_DOF_*); they are NOT clamped
 *   pose       R[5][3]            the aligned key points the angles were fitted to
 *   kp_weight  R[4]               nullable (all weights 1): the weights w_k the fit was made with
 *   kp_sigma   R[4]               nullable: isotropic standard deviation of key points 1..4 (read for std only)
 *   smooth     [7]                host memory, nullable (SEQIK_SMOOTH_DEFAULT each): the penalty the fit was made with
 *   sens       R[2W+1][7][4][3]   nullable: [t][d][j][k-1][c] = d (angle j of frame t) / d (component c of aligned key
 *                                 point k of frame t + d - W)
 *   std        R[7]               nullable, needs kp_sigma: the standard deviation of every angle under noise that is
 *                                 independent between frames, key points and components; it does not depend on W
 *   grad       R                  nullable: max_F |g_j| / len^2 of that frame, g the FULL gradient of step 2 of
 *                                 seqik_smooth.h (data plus penalty); its maximum over a trajectory is the left side of
 *                                 the gradient test of seqik_smooth.h (no DOF free: 0)
 *   flags      R                  nullable, int32: bits 0..6 DOF held; bit 8 not a strict minimum; bit 16 bad input;
 *                                 bit 17 bad sigma
 * At least one of sens, std, grad, flags must be given.  legs[i].seg and legs[i].bounds are read.
 *
 * Definition, per trajectory (one (sequence, leg) pair, frames t = 0..N-1; trajectories do not influence each other).
 * s_j = smooth[j] * len^2, len = ((seg0 + seg1) + seg2) + seg3, as in seqik_smooth.h.
 *   1. A frame is BAD under rule 1 of seqik_refine.h (angles, weights, pose[0], the key points with weight not 0; the
 *      sigmas are no part of it).  A PAIR (t-1, t) exists when both frames are good.  A bad frame is an identity row of the
 *      Hessian: it cuts the coupling exactly as in the fit.  Its std, grad and in-range blocks of sens are the one quiet
 *      NaN and its flags is bit 16 alone.
 *   2. g_t = the g of seqik_refine_sensitivity.h at frame t; then, for the previous neighbour u = t-1 first and then
 *      u = t+1, where that pair exists, for j ascending g_j = g_j + s_j (q_{t,j} - q_{u,j}): the bits of step 2 of
 *      seqik_smooth.h.  H_tt = the exact data Hessian of seqik_refine_sensitivity.h (J^T J plus the residual-curvature term),
 *      and H_jj = H_jj + s_j once per existing pair, in the same order.
 *   3. DOF j of frame t is HELD under the wording of seqik_refine_sensitivity.h (bound_tol, default SEQIK_SENS_BOUND_TOL,
 *      0 disables the rule) on this full gradient.  F_t = the DOFs of frame t that are not held.  A held DOF's row and
 *      column of H_tt are the identity's.  grad = max over F_t of |g_j|, divided by len^2.
 *   4. K_t = diag(k_j), k_j = s_j where the pair (t-1, t) exists and DOF j is held in neither frame, otherwise +0.0;
 *      H_{t,t-1} = H_{t-1,t} = -K_t.  A pair is COUPLED when some k_j is not 0.  A RUN is a maximal set of consecutive
 *      frames joined by coupled pairs: the diagonal blocks of H, and so the questions below, belong to one run each.
 *   5. B_t (7 x 12) has the columns w_k (w_k J_k,c) of seqik_refine_sensitivity.h (d g_t / d t_k = -w_k J_k^T; only frame
 *      t's g sees frame t's key points); a held row is 0.  A key point with weight exactly 0 is not read.
 *   6. Schur sweeps, serial over the frames.  Forward: Sf_t = H_tt where the pair (t-1, t) is not coupled, otherwise
 *      Sf_t[i][j] = H_tt[i][j] - k_i Pf_{t-1}[i][j] (lower triangle), Pf_t = Sf_t^-1 K_{t+1} column by column (stored
 *      where the pair (t, t+1) is coupled).  Backward: Sb_t = H_tt where (t, t+1) is not coupled, otherwise
 *      Sb_t[i][j] = H_tt[i][j] - k_i Pb_{t+1}[i][j] with the k of K_{t+1}, Pb_t = Sb_t^-1 K_t.  Each S is factored by
 *      Cholesky in the fixed order of seqik_refine.h and the columns are substituted as there (plain sqrt and /).  A pivot
 *      that is not positive in Sf poisons the frames from there to the end of its run, one in Sb the frames from there
 *      back to the start of its run.
 *   7. Combine, per frame: T = (Sf_t + Sb_t) - H_tt entry by entry (lower triangle), factored the same way; G_tt = T^-1.
 *      A pivot that is not positive poisons that frame.  The union of the three is the whole run exactly when H_FF of the
 *      run is not positive definite (the Schur complement onto one frame fails where both sides are positive definite and
 *      the whole is not: scalar blocks 1, 5, 1 with couplings 2 pass both sweeps at frame 1, and 1 + 1 - 5 < 0).  A
 *      poisoned frame has bit 8; its free rows of sens (blocks whose source lies in its run) and of std are NaN.
 *      sens0_t = the block at offset W = G_tt B_t: twelve right-hand sides substituted key point by key point as
 *      seqik_refine_sensitivity.h does; a held row is +0.0, a column of a key point with weight 0 is +0.0 (in rows that
 *      are NaN it is NaN).  In a frame no pair couples, T = H_tt and the block has the bits of seqik_refine_sensitivity.
 *      own_j = sum_k sigma_k^2 ((x_0^2 + x_1^2) + x_2^2) over that block, k ascending;
 *      Wt[i][j] = sum_k sigma_k^2 ((x_i0 x_j0 + x_i1 x_j1) + x_i2 x_j2), k ascending = sens0 diag(sigma^2) sens0^T.
 *   8. Off-centre blocks: the inverse's blocks obey G_ts = Pb_t G_{t-1,s} for t > s and G_ts = Pf_t G_{t+1,s} for t < s, so
 *      the block of frame t for the source s = t - m is Q_m sens0_s with Q_1 = Pb_t, Q_{m+1} = Q_m Pb_{t-m}, and for
 *      s = t + m with Q_1 = Pf_t, Q_{m+1} = Q_m Pf_{t+m}; every product entry is p_0, then + p_1, ... + p_6.  A block whose
 *      source frame lies outside 0..N-1 is +0.0.  A block whose source lies outside the run of t (a bad frame or an
 *      uncoupled pair in between) is +0.0.  Held rows are +0.0, columns of a source key point with weight 0 are +0.0.
 *   9. Covariance sweeps, serial: Lam_t = 0 where the pair (t-1, t) is not coupled, otherwise Pb_t (Lam_{t-1} + W_{t-1})
 *      Pb_t^T; Ups_t = 0 where (t, t+1) is not coupled, otherwise Pf_t (Ups_{t+1} + W_{t+1}) Pf_t^T (the product with P
 *      first, then with P^T, lower triangle, mirrored).  std_j = sqrt(own_j + (Lam_jj + Ups_jj)); a held joint has +0.0.
 *      This is the diagonal of H^-1 M H^-1 with M = B diag(sigma^2) B^T, NOT of H^-1: the penalty and the
 *      residual-curvature term stiffen the fit but are no noise model.
 *  10. Bad sigma: a non-finite or negative sigma of a key point with weight not 0 on a good frame sets bit 17 on that
 *      frame and makes the free rows of std NaN on every frame of its run; sens is untouched.  A poisoned frame does
 *      the same to the std of its run.  The sigma of a key point with weight exactly 0 is not read (it may be NaN) and
 *      counts as 0: it changes no bit of any output.
 * Every NaN stored is the one quiet NaN, so records compare by bits; host-run rule and kernels agree bit for bit.  The
 * values are for the ALIGNED key points; for RAW key points the sensitivity is the alignment's scale x these values.
 *
 * Workspace: seqik_smooth_sensitivity_workspace_bytes() bytes of device memory, 8-byte aligned: 1364 bytes per leg-frame
 * (H 224, Pf and Pb 392 each, Wt 224, the diagonals of Lam and Ups 56 each, five int32 words) plus at most 256 bytes of
 * padding for each of its eleven pieces; nothing per trajectory.  -1 (and seqik_last_error()) when the sizes are not valid.
 *
 * Return codes and seqik_last_error() as in seqik.h.  SEQIK_ERR_BAD_ARG, before anything touches HIP: n_legs outside
 * 1..8, a negative size, null angles / pose / legs, no output requested, std without kp_sigma, kind not 0, a non-finite
 * segment length, a non-finite or negative bound_tol, a smooth entry that is negative or not finite, half_width outside
 * 0..32, more leg-frames than can be addressed, and for the device entry a workspace that is null, misaligned or smaller
 * than asked for.  A call with no leg-frames returns SEQIK_OK without a launch.
 */
#ifndef SEQIK_SMOOTH_SENSITIVITY_H
#define SEQIK_SMOOTH_SENSITIVITY_H

#include "seqik_refine_sensitivity.h"
#include "seqik_smooth.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SEQIK_SMOOTHSENS_MAX_HALF_WIDTH 32
#define SEQIK_SMOOTHSENS_FLAG_HELD(dof) (1 << (dof))
#define SEQIK_SMOOTHSENS_FLAG_NOT_PD (1 << 8)
#define SEQIK_SMOOTHSENS_FLAG_BAD_INPUT (1 << 16)
#define SEQIK_SMOOTHSENS_FLAG_BAD_SIGMA (1 << 17)

int64_t seqik_smooth_sensitivity_workspace_bytes(int64_t n_seq, int32_t n_legs, int64_t n_frames, int32_t half_width);

/* Host buffers: copies in, takes the workspace from the pooled arena of `device` (-1 = the calling thread's current
 * device), launches on a pooled stream, copies out and synchronises. */
int seqik_smooth_sensitivity(const double *angles, const double *pose, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                             const SeqikLegParams *legs, int32_t kind, const double *kp_weight, const double *kp_sigma,
                             const double *smooth, double bound_tol, int32_t half_width, double *sens, double *std,
                             double *grad, int32_t *flags, int32_t device);

/* Device buffers and the caller's workspace on `hip_stream` (hipStream_t; NULL = the default stream) of the current
 * device.  UNLIKE seqik_smooth_legs_device THIS ENTRY ALLOCATES NOTHING AND WAITS FOR NOTHING: it enqueues a fixed number
 * of launches for a request (at most five: assemble, Schur sweeps, combine, covariance sweeps, finish) and returns, so it
 * can be captured into a graph.  `legs` and `smooth` are host memory. */
int seqik_smooth_sensitivity_device(const double *d_angles, const double *d_pose, int64_t n_seq, int32_t n_legs,
                                    int64_t n_frames, const SeqikLegParams *legs, int32_t kind, const double *d_kp_weight,
                                    const double *d_kp_sigma, const double *smooth, double bound_tol, int32_t half_width,
                                    double *d_sens, double *d_std, double *d_grad, int32_t *d_flags, void *d_workspace,
                                    int64_t workspace_bytes, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* SEQIK_SMOOTH_SENSITIVITY_H */
