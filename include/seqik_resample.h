/*
 * seqik_resample.h -- resampling joint-angle series with a shape-preserving cubic (PCHIP) on the GPU, optionally
 * bridging missing frames (libseqik_hip.so, gfx950).
 *
 * The reference's pipeline ends with utils.interpolate_joint_angles: every series goes through
 * scipy.interpolate.pchip_interpolate from the camera's time step to the consumer's.  These entry points do the same for
 * records y[chain][n_frames][width] of float64 (width 1..16: 7 is a solver's angle block, 1 a plain series) and write
 * out[chain][n_out][width].  The solvers of seqik.h are not involved and not changed.
 *
 *   knot j      x_j = j * original_ts                      (j < n_frames; one float64 multiplication)
 *   sample i    u_i = i * new_ts                           (i < n_out)
 *   n_out       ceil((n_frames * original_ts) / new_ts) in float64: len(np.arange(0, n_frames * original_ts, new_ts))
 *   interval    the largest j with x_j <= u_i, at most n_frames - 2: the up to original_ts / new_ts samples behind the
 *               last knot are evaluated with the last interval's cubic (scipy: extrapolate=True)
 *   derivatives scipy's PchipInterpolator._find_derivatives: 0 where the two secant slopes differ in sign or one is 0,
 *               else their weighted harmonic mean; the three-point rule at both ends; two knots give a straight line
 *   value       the cubic Hermite polynomial of the interval; a sample that sits on a knot is that knot's value, bit for
 *               bit (the last knot closes its interval instead of opening one: its value is returned, not evaluated)
 *
 * DEFAULT MODE checks nothing per frame: a sample whose stencil (knots j-1 .. j+2, as far as they exist) holds a
 * non-finite value in its column is NaN, and no other sample is affected.
 *
 * BRIDGE MODE (SEQIK_RESAMPLE_BRIDGE).  A knot is MISSING when any of the `width` values of its record is non-finite
 * (what skip mode, seqik_gaps.h, writes).  Every chain is resampled as pchip_interpolate(x[valid], y[valid], u) would:
 * spacings and slopes run between neighbouring valid knots, the end rules apply at the first and last valid knot.  A
 * sample in front of the first valid knot, or at or behind x_last_valid + original_ts, is NaN.  A chain with fewer than
 * two valid knots is NaN throughout.  max_gap (negative = unlimited): a sample strictly inside an interval that spans
 * more than max_gap missing knots is NaN; derivatives are not affected by max_gap.  Bridge mode needs a workspace of
 * seqik_resample_workspace_bytes(): int32 prev[n_chains][n_frames] (the last valid knot <= j, -1 = none), then int32
 * next[n_chains][n_frames] (the first valid knot >= j, n_frames = none).
 *
 * Return codes and seqik_last_error() as in seqik.h.  SEQIK_ERR_BAD_ARG (before any launch): null buffers, a negative
 * n_chains, n_frames < 2 or >= 2^31, width outside 1..16, time steps that are not finite and positive (or outside
 * 2^-500 .. 2^500), an n_out that is not seqik_resample_count(), unknown flags, a missing workspace in bridge mode.
 * A call with n_chains == 0 returns SEQIK_OK without a launch.
 */
#ifndef SEQIK_RESAMPLE_H
#define SEQIK_RESAMPLE_H

#include <stddef.h>

#include "seqik.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SEQIK_RESAMPLE_BRIDGE 1

/* Samples per chain (host only, no GPU needed), or a negative SEQIK_ERR_* (n_frames < 2, bad time steps, a count of
 * 2^31 or more). */
int64_t seqik_resample_count(int64_t n_frames, double original_ts, double new_ts);

/* Bytes of d_workspace seqik_resample_pchip_device needs: 8 per knot in bridge mode, else 0. */
size_t seqik_resample_workspace_bytes(int64_t n_chains, int64_t n_frames, int32_t flags);

/* Host buffers, blocking, on `device` (-1 = the calling thread's current device). */
int seqik_resample_pchip(const double *y, int64_t n_chains, int64_t n_frames, int32_t width, double original_ts,
                         double new_ts, int32_t flags, int32_t max_gap, double *out, int64_t n_out, int32_t device);

/* Device buffers, only enqueues on `hip_stream` (hipStream_t; NULL = the default stream) of the current device: no
 * allocation, no synchronisation.  d_workspace: see above (NULL allowed in default mode). */
int seqik_resample_pchip_device(const double *d_y, int64_t n_chains, int64_t n_frames, int32_t width,
                                double original_ts, double new_ts, int32_t flags, int32_t max_gap, double *d_out,
                                int64_t n_out, void *d_workspace, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* SEQIK_RESAMPLE_H */
