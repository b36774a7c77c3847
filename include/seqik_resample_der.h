/*
 * seqik_resample_der.h -- joint-angle velocities and accelerations: the first and second derivative of the PCHIP
 * interpolant of seqik_resample.h, with or without its value, on the GPU (libseqik_hip.so, gfx950).
 *
 * Knots, samples, n_out, intervals, knot derivatives, default mode, bridge mode, max_gap and the workspace are those of
 * seqik_resample.h; scipy's counterpart is pchip_interpolate(x, y, u, der=1 | 2 | [0, 1, 2]).  A sample at
 * s = u - x_A lies on the interval's cubic c0 s^3 + c1 s^2 + d_A s + y_A (d_A: the derivative at knot A):
 *
 *   value              as seqik_resample_pchip[_device] writes it, bit for bit
 *   first derivative   fma(fma(3 c0, s, 2 c1), s, d_A), in units of y per unit of original_ts.  A sample on a knot gets that
 *                      knot's derivative d_A bit for bit (s = 0); the sample on the last (valid) knot gets that knot's
 *                      derivative d_B, returned and not evaluated, as its value is
 *   second derivative  fma(6 c0, s, 2 c1): on an interior knot the RIGHT interval's 2 c1 (scipy's half-open intervals),
 *                      on the last knot the last interval's at s = h
 *
 * The samples behind the last knot continue the last cubic in every order.  Every order is NaN exactly where the value
 * is NaN: in default mode where the sample's stencil holds a non-finite value; in bridge mode in front of the first
 * valid knot, at or behind x_last_valid + original_ts, strictly inside a gap of more than max_gap missing knots, and
 * throughout a chain with fewer than two valid knots.  (A derivative can overflow where the value does not, beyond
 * about 2^1000 / original_ts^3.)
 *
 * Each output plane is [chain][n_out][width] float64.  A NULL plane is neither computed nor written; the knots are
 * staged once per tile whatever number of planes is asked for.  Return codes and seqik_last_error() as in seqik.h;
 * SEQIK_ERR_BAD_ARG (before any launch): all three planes NULL, and everything seqik_resample_pchip[_device] refuses.
 * n_out is seqik_resample_count(), d_workspace holds seqik_resample_workspace_bytes().  The entry points are additive:
 * seqik_abi_version() is unchanged.
 */
#ifndef SEQIK_RESAMPLE_DER_H
#define SEQIK_RESAMPLE_DER_H

#include "seqik_resample.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host buffers, blocking, on `device` (-1 = the calling thread's current device). */
int seqik_resample_der(const double *y, int64_t n_chains, int64_t n_frames, int32_t width, double original_ts,
                       double new_ts, int32_t flags, int32_t max_gap, double *out_value, double *out_d1, double *out_d2,
                       int64_t n_out, int32_t device);

/* Device buffers, only enqueues on `hip_stream` (hipStream_t; NULL = the default stream) of the current device: no
 * allocation, no synchronisation.  d_workspace as for seqik_resample_pchip_device (NULL allowed in default mode). */
int seqik_resample_der_device(const double *d_y, int64_t n_chains, int64_t n_frames, int32_t width, double original_ts,
                              double new_ts, int32_t flags, int32_t max_gap, double *d_value, double *d_d1, double *d_d2,
                              int64_t n_out, void *d_workspace, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* SEQIK_RESAMPLE_DER_H */
