/*
 * seqik_refine.h -- whole-leg refinement: from the angles of the sequential leg fit, minimise the distance to all four
 * key points together, inside the joint limits (libseqik_hip.so, gfx950).  Additive to ABI 7.
 *
 * The sequential fit is greedy: stage s fits key point s with its own one or two angles and no stage looks back, so the
 * error accumulates towards the claw.  These entry points start from that answer (or any other) and run, one GPU lane per
 * leg-frame, a small bounded Levenberg-Marquardt on all seven angles and all twelve coordinates at once.  Every leg-frame
 * is refined on its own, from its own start: nothing couples a frame to its neighbours.  It is a solver of its own, not
 * a port of scipy's TRF; on the shipped recording it reaches scipy's final cost.
 *
 * Layouts (dense; kind as in seqik_fk.h):
 *   angles     [n_seq][n_legs][n_frames][7]      the start, DOFS order (SEQIK_DOF_*)
 *   pose       [n_seq][n_legs][n_frames][5][3]   the aligned key points
 *   kp_weight  [n_seq][n_legs][n_frames][4]      nullable (all weights 1): the weight w_k of key points 1..4
 *   angles_out [n_seq][n_legs][n_frames][7]      required; may be the buffer of angles (a lane reads its seven values
 *                                                before it writes them)
 *   cost       [n_seq][n_legs][n_frames][2]      nullable: the weighted sum of squares at the clamped start, at the result
 *   info       [n_seq][n_legs][n_frames]         nullable, int32: bits 0..6 DOF held on a limit at exit; bits 8..10 why
 *                                                it stopped (SEQIK_REFINE_STOP_*); bits 16..23 accepted iterations; bit
 *                                                24 non-finite input
 * legs[i].seg and legs[i].bounds are read.
 *
 * Definition.  For a leg-frame t_k = pose[k] - pose[0], f_k(q) = key point k of the chain (FK rows 4, 6, 7, 8, leg-local),
 * r = (w_k (f_k - t_k)), 12 values, c = r . r, lb / ub = legs[].bounds.
 *   1. Bad input: a non-finite angle or |angle| > SEQIK_ANGLE_MAX, a non-finite segment length, a non-finite or negative
 *      weight, a non-finite coordinate of pose[0], a non-finite coordinate of a key point whose weight is not exactly 0.
 *      angles_out and cost are NaN, info is bit 24 alone.  Not an error; no other leg-frame is affected.  A key point
 *      with weight exactly 0 is not read: it may hold NaN (a single missing key point).
 *   2. Start: q = clamp(angles, lb, ub), lambda = 1e-3.
 *   3. Each iteration: J (12 x 7) = w_k a_j x (f_k - o_j) as in seqik_jacobian.h (structural zeros never computed), g =
 *      J^T r.  DOF j is HELD when (q_j <= lb_j and g_j > 0) or (q_j >= ub_j and g_j < 0); F = the DOFs not held.  Stop with
 *      reason 0 when F is empty or max_F |g_j| <= gtol (seg_0 + seg_1 + seg_2 + seg_3)^2.
 *   4. Step: A = J_F^T J_F, d = diag(A) with entries <= 0 replaced by the smallest normal double; solve (A + lambda
 *      diag(d)) delta = -g_F by Cholesky (plain sqrt and /, fixed order; a pivot that is not positive counts as a
 *      rejection); q' = q with q'_F = clamp(q_F + delta).  Accepted when c(q') < c(q): lambda = max(lambda / 3, 1e-12), and
 *      when the decrease is <= ftol c(q) stop with reason 1.  A trial that moved (q' != q) and is not accepted, but whose
 *      cost lies within ftol c(q) of c(q), also stops with reason 1, at q: the cost no longer tells the two points apart
 *      (at the default ftol that is the rounding of c itself; without this a converged lane ends up in reason 2).
 *      Otherwise lambda *= 4 and the same J is tried again; when lambda > 1e12 stop with reason 2.
 *   5. Stop with reason 4 after max_iter accepted iterations.
 * By construction cost[1] <= cost[0], every output angle lies inside [lb, ub] exactly, and a start that already meets
 * the gradient test comes back as its clamped bits with 0 iterations.  The held bits are those of the rule of step 3 at
 * the result.  Frames are independent: where a leg has two configurations that fit, neighbouring frames may land in
 * different ones, and an angle may move by more than a radian from its start.
 *
 * Options: NULL = the defaults below.  Return codes and seqik_last_error() as in seqik.h.  SEQIK_ERR_BAD_ARG, before
 * anything touches HIP: n_legs outside 1..8, a negative size, null legs / angles / pose / angles_out, kind not 0 (kind 1,
 * the generic chain, is not built), a non-finite segment length, max_iter outside 1..255, a tolerance that is negative
 * or not finite, more leg-frames than 120 bytes each can be addressed for.  A call with no leg-frames returns SEQIK_OK
 * without a launch.
 */
#ifndef SEQIK_REFINE_H
#define SEQIK_REFINE_H

#include "seqik_fk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SEQIK_REFINE_MAX_ITER 200
#define SEQIK_REFINE_GTOL 1e-10
#define SEQIK_REFINE_FTOL 1e-14

#define SEQIK_REFINE_HELD(dof) (1 << (dof))
#define SEQIK_REFINE_STOP(info) (((info) >> 8) & 7)
#define SEQIK_REFINE_STOP_GRADIENT 0
#define SEQIK_REFINE_STOP_DECREASE 1
#define SEQIK_REFINE_STOP_DAMPING 2
#define SEQIK_REFINE_STOP_MAX_ITER 4
#define SEQIK_REFINE_ITERATIONS(info) (((info) >> 16) & 255)
#define SEQIK_REFINE_BAD_INPUT (1 << 24)

typedef struct SeqikRefineOptions {
    int32_t max_iter; /* accepted iterations at most, 1..255 */
    double gtol;      /* gradient test, relative to the squared leg length */
    double ftol;      /* relative cost decrease below which an accepted step is the last */
} SeqikRefineOptions;

/* Host buffers: copies in, launches on a pooled stream of `device` (-1 = the calling thread's current device),
 * copies out and synchronises. */
int seqik_refine_legs(const double *angles, const double *pose, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                      const SeqikLegParams *legs, int32_t kind, const double *kp_weight, const SeqikRefineOptions *opt,
                      double *angles_out, double *cost, int32_t *info, int32_t device);

/* Device buffers: only enqueues the kernel on `hip_stream` (hipStream_t; NULL = the default stream) of the current
 * device; allocates nothing and does not synchronise.  `legs` and `opt` are host memory. */
int seqik_refine_legs_device(const double *d_angles, const double *d_pose, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                             const SeqikLegParams *legs, int32_t kind, const double *d_kp_weight,
                             const SeqikRefineOptions *opt, double *d_angles_out, double *d_cost, int32_t *d_info,
                             void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* SEQIK_REFINE_H */
