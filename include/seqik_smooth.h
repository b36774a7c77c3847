/*
 * seqik_smooth.h -- trajectory refinement: the whole-leg fit of seqik_refine.h over ALL frames of a recording at once, with
 * a penalty on the change of every angle from frame to frame, inside the joint limits (libseqik_hip.so, gfx950).
 * Additive to ABI 7.
 *
 * seqik_refine_legs treats every leg-frame on its own; where a leg has two configurations that fit, neighbouring frames
 * land in different ones and the trajectory jumps.  These entry points couple the frames.  A TRAJECTORY is one (sequence,
 * leg) pair with its frames t = 0..N-1; trajectories do not influence each other.
 *
 * Layouts (dense; kind as in seqik_fk.h):
 *   angles     [n_seq][n_legs][n_frames][7]      the start, DOFS order (SEQIK_DOF_*)
 *   pose       [n_seq][n_legs][n_frames][5][3]   the aligned key points
 *   kp_weight  [n_seq][n_legs][n_frames][4]      nullable (all weights 1): the weight w_k of key points 1..4
 *   angles_out [n_seq][n_legs][n_frames][7]      required; may be the buffer of angles (every start is read before any
 *                                                result is written)
 *   frame_info [n_seq][n_legs][n_frames]         nullable, int32: bits 0..6 DOF held on a limit at exit
 *                                                (SEQIK_REFINE_HELD), bit 24 bad input (SEQIK_REFINE_BAD_INPUT)
 *   cost       [n_seq][n_legs][2]                nullable: C at the clamped start and at the result
 *   info       [n_seq][n_legs][3]                nullable, int32: why the trajectory stopped (SEQIK_REFINE_STOP_*), its
 *                                                accepted steps, its rejected trials
 * legs[i].seg and legs[i].bounds are read.
 *
 * Problem, per trajectory.  c_t(q) is the data term of seqik_refine.h for frame t: the same targets, kp_weight and
 * residual order; a key point with weight exactly 0 is not read.  A frame is BAD under rule 1 of seqik_refine.h; its
 * angles_out are NaN, its frame_info is bit 24 alone, and it takes no part in the fit.  A PAIR (t-1, t) exists when both
 * frames are good, so a bad frame cuts the coupling there (the NaN frames of skip mode split a recording into
 * trajectories of their own).  s_j = smooth[j] * len^2 with len = ((seg0 + seg1) + seg2) + seg3; smooth[j] is
 * dimensionless, one value per DOF.
 *     C(Q) = sum_t c_t(q_t) + sum_pairs sum_j s_j (q_{t,j} - q_{t-1,j})^2      subject to lb <= q_t <= ub.
 *
 * Rule: ONE bounded Levenberg-Marquardt per trajectory -- one lambda and one accept / reject decision for all its
 * frames.  The constants 1e-3, / 3, * 4, 1e-12 and 1e12, the held rule, the gradient bar gtol * len^2, the ftol stop and
 * the stall stop are those of seqik_refine.h, each applied to the whole trajectory.
 *   1. Start: q_t = clamp(angles_t).
 *   2. Assemble, per good frame: A_t = J^T J and g_t = J^T r of seqik_refine.h; for each existing pair, the previous
 *      neighbour u = t-1 first and then u = t+1: g_j += s_j (q_{t,j} - q_{u,j}), A_jj += s_j.  DOF j of frame t is HELD
 *      when (q <= lb and g > 0) or (q >= ub and g < 0) on this full gradient.
 *   3. Stop tests, in this order: the last accepted step's decrease was <= ftol C (reason 1); max_iter accepted steps
 *      (reason 4); every free |g| <= gtol len^2 over the whole trajectory (reason 0).
 *   4. Step: the block-tridiagonal system with one 7 x 7 block row per frame, D_t = A_t + lambda diag(d_t) (d_j = A_jj,
 *      an entry <= 0 replaced by DBL_MIN), L_t = -diag(s) where the pair (t-1, t) exists and otherwise 0, U_t = L_{t+1}^T,
 *      b_t = -g_t.  Held DOFs are masked as seqik_refine.h masks them: their row and column of D are the identity's,
 *      their rows and columns of L and U and their entry of b are 0.  Bad frames are identity rows with b = 0.  Solved
 *      by PARALLEL CYCLIC REDUCTION, strides h = 1, 2, 4, ... while h < N: every row u is normalised (Cholesky of D_u in
 *      the fixed order of seqik_refine.h, reading the lower triangle; EL_u = D_u^-1 L_u, EU_u = D_u^-1 U_u, eb_u =
 *      D_u^-1 b_u), then every row t is reduced: D'_t = (D_t - L_t EU_{t-h}) - U_t EL_{t+h}, L'_t = -(L_t EL_{t-h}),
 *      U'_t = -(U_t EU_{t+h}), b'_t = (b_t - L_t eb_{t-h}) - U_t eb_{t+h}; a term whose neighbour lies outside 0..N-1 is
 *      left out.  Finally delta_t = D_t^-1 b_t.  A pivot that is not positive, in any row at any stride, makes the trial
 *      a rejection.
 *   5. Trial: q'_t = q_t on held DOFs, clamp(q_t + delta_t) on the others.  e_t = c_t(q'_t) + sum_j s_j (q'_{t,j} -
 *      q'_{t-1,j})^2 (j ascending, only where the pair exists; 0 for a bad frame); C' = the sum of e_0..e_{N-1} over the
 *      aligned binary tree after padding with +0.0 to a power of two.  The starting cost is formed the same way.  An
 *      angle outside the domain of seqik_fk.h, or a C' that is NaN, is a rejection.
 *   6. Decide: accepted when C' < C: lambda = max(lambda / 3, 1e-12), and when C - C' <= ftol C the next stop test ends
 *      the trajectory.  A trial that moved (any q' != q) with C' - C <= ftol C stops with reason 1 at q.  Otherwise
 *      lambda *= 4 and the same A, g and held set are tried again; above 1e12 the trajectory stops with reason 2.
 * By construction cost[1] <= cost[0], every good frame's output lies inside [lb, ub] exactly, and a trajectory that
 * already meets the gradient test comes back as its clamped bits with 0 steps.  A trajectory with no good frame gets
 * reason 0, 0 steps and cost 0.
 *
 * smooth all zero is allowed and decouples the frames, but it is NOT seqik_refine_legs: there is still one lambda and one
 * decision per trajectory, so a frame that would have accepted its own step waits for the others.
 *
 * Like every local method this one ends in the minimum its start leads to; with a weak penalty (smooth = 0.01) and a
 * start that jumps, that can be another one than scipy's trust-region method finds from the same start.
 *
 * Workspace: seqik_smooth_workspace_bytes(n_seq, n_legs, n_frames) bytes of device memory, at most 3940 per leg-frame
 * plus 48 per trajectory plus 3072; -1 (and seqik_last_error()) when the sizes are not valid.
 *
 * Options: NULL = the defaults below (smooth = SEQIK_SMOOTH_DEFAULT for every DOF).  Return codes and seqik_last_error()
 * as in seqik.h.  SEQIK_ERR_BAD_ARG, before anything touches HIP: those of seqik_refine.h (max_iter: 1..1000 here), a
 * smooth entry that is negative or not finite, and for the device entry a workspace that is null or smaller than asked
 * for.  A call with no leg-frames returns SEQIK_OK without a launch.
 */
#ifndef SEQIK_SMOOTH_H
#define SEQIK_SMOOTH_H

#include "seqik_refine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SEQIK_SMOOTH_DEFAULT 0.1
#define SEQIK_SMOOTH_MAX_ITER 300

typedef struct SeqikSmoothOptions {
    double smooth[7]; /* the penalty of every DOF, relative to the squared leg length; finite, >= 0 */
    int32_t max_iter; /* accepted steps at most, 1..1000 */
    double gtol;      /* as SeqikRefineOptions (SEQIK_REFINE_GTOL) */
    double ftol;      /* as SeqikRefineOptions (SEQIK_REFINE_FTOL) */
} SeqikSmoothOptions;

int64_t seqik_smooth_workspace_bytes(int64_t n_seq, int32_t n_legs, int64_t n_frames);

/* Host buffers: copies in, allocates the workspace from the pooled arena of `device` (-1 = the calling thread's current
 * device), runs the rounds on a pooled stream, copies out and synchronises. */
int seqik_smooth_legs(const double *angles, const double *pose, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                      const SeqikLegParams *legs, int32_t kind, const double *kp_weight, const SeqikSmoothOptions *opt,
                      double *angles_out, int32_t *frame_info, double *cost, int32_t *info, int32_t device);

/* Device buffers and the caller's workspace (8-byte aligned) on `hip_stream` (hipStream_t; NULL = the default stream) of
 * the current device; allocates nothing.  UNLIKE THE OTHER _device ENTRY POINTS THIS ONE SYNCHRONISES THE STREAM: once
 * per trial round it waits for the stream and reads the number of trajectories still running (4 bytes); the rows of
 * stopped trajectories are skipped from then on.  It returns with the last launch enqueued, not waited for.  It cannot be
 * captured into a graph.  `legs` and `opt` are host memory. */
int seqik_smooth_legs_device(const double *d_angles, const double *d_pose, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                             const SeqikLegParams *legs, int32_t kind, const double *d_kp_weight,
                             const SeqikSmoothOptions *opt, double *d_angles_out, int32_t *d_frame_info, double *d_cost,
                             int32_t *d_info, void *d_workspace, int64_t workspace_bytes, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* SEQIK_SMOOTH_H */
