/*
 * seqik_head_align.h -- antenna alignment on the GPU (libseqik_hip.so, gfx950): the whole-recording statistics of
 * AlignPose.align_head and its per-frame map fused into the head / antenna angle kernel.
 *
 * AlignPose.align_head (seqikpy/alignment.py:489-555) is, per side S in {R, L}, with head = <S>_head [n][2][3] (antenna
 * base, antenna tip) and mid = 0.5 * (Thorax[:, 0] + Thorax[:, last]):
 *   d[t]    = |head[t][0] - mid[t]|        = sqrt((dx*dx + dy*dy) + dz*dz), every operation rounded on its own
 *   len[t]  = |head[t][1] - head[t][0]|      (same form)
 *   stat    = { i in [0, n-3] : (d[i+2] - d[i+1]) - (d[i+1] - d[i]) < threshold }     signed; a NaN compares false
 *   origin[a]  = meanq(head[stat][0][a]),   meanq = mean of the 0.45 and 0.55 quantiles
 *   scale_base = body_size["Antenna_mid_thorax"] / meanq(d[stat])
 *   scale_tip  = body_size["Antenna"]            / meanq(len[:])
 *   aligned[t][0] = (head[t][0] - origin) * scale_base + template_base
 *   aligned[t][1] = (head[t][1] - origin) * scale_tip  + template_base      subtract, multiply, add: three roundings
 *
 * Statistics.  Five series per side: base x, y, z over stat, d over stat, len over all n frames.  The size of stat is
 * only known after the selection, and the quantile ranks depend on it: hence two calls.
 *   seqik_head_align_stats_select  extracts the ten series and returns n_stat[2] (R, L) and the number of non-finite
 *                                  series values it saw (a caller that gets a non-zero count takes its host path: a
 *                                  sort would push a NaN to the end where numpy's quantile returns NaN);
 *   seqik_head_align_stats_pick    sorts each series (exact order statistics) and returns the requested ranks:
 *                                  out[side][series][rank], series 0..3 picked with ranks_stat[side][.] (clamped to
 *                                  n_stat[side] - 1), series 4 with ranks_all[.] (clamped to n - 1).
 * The caller applies numpy's own quantile interpolation to the order statistics; the constants then equal the host
 * path's bit for bit.  _select takes the WHOLE recording: the second difference crosses slab seams, so there is no
 * slab-wise accumulation here (seqik_align_stats_add has one for the legs, whose series are per frame).
 *
 * Fused map.  seqik_head_angles_raw[_device] are seqik_head_angles_ex[_device] (seqik.h) on RAW r_head / l_head: the
 * kernel's prologue applies the two maps above to every frame (three rounded operations each) and then runs the same
 * closed forms, so the angles equal, bit for bit, those of seqik_head_angles_ex on the host-aligned points.  With
 * n_points == 1 only the antenna base is mapped (and compute_ant must be 0).  r_aligned / l_aligned, nullable
 * [n][2][3] (n_points >= 2; [n][1][3] for n_points == 1): the aligned key points (what AlignPose.align_head returns).
 * Records of more than two key points per side are read with their stride; only points 0 and 1 are used.
 *
 * Return codes and seqik_last_error() as in seqik.h.
 */
#ifndef SEQIK_HEAD_ALIGN_H
#define SEQIK_HEAD_ALIGN_H

#include "seqik.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Constants of AlignPose.align_head for one side. */
typedef struct SeqikHeadAffine {
    double origin[3];        /* fixed antenna origin (quantile statistics over the stationary frames) */
    double scale_base;       /* applied to the antenna base */
    double scale_tip;        /* applied to the antenna tip */
    double template_base[3]; /* body_template["<S>_Antenna_base"] */
} SeqikHeadAffine;

typedef struct SeqikHeadAlignStats SeqikHeadAlignStats;

/* Room for recordings of up to capacity_frames frames (80 B of device memory per frame).  opt: only `device` is read. */
int seqik_head_align_stats_open(SeqikHeadAlignStats **out, int64_t capacity_frames, const SeqikOptions *opt);

/* r_head, l_head [n][n_points][3] (n_points >= 2), thorax [n][n_thorax_points][3] (points 0 and last are read); host
 * pointers, or device pointers of the handle's device when on_device != 0 (their contents must be complete: the call
 * runs on a stream of its own).  3 <= n <= capacity.  Synchronises.  n_stat[2]: frames selected for R, L;
 * n_nonfinite: non-finite values among the 10 n series values (before the selection). */
int seqik_head_align_stats_select(SeqikHeadAlignStats *s, const double *r_head, const double *l_head,
                                  const double *thorax, int32_t on_device, int64_t n, int32_t n_points,
                                  int32_t n_thorax_points, double threshold, int64_t *n_stat, int64_t *n_nonfinite);

/* After a _select.  ranks_stat [2][n_ranks], ranks_all [n_ranks], out [2][5][n_ranks] (host).  1 <= n_ranks <= 16.
 * SEQIK_ERR_BAD_ARG when a side selected no frame.  Synchronises. */
int seqik_head_align_stats_pick(SeqikHeadAlignStats *s, const int64_t *ranks_stat, const int64_t *ranks_all,
                                int32_t n_ranks, double *out);

int seqik_head_align_stats_close(SeqikHeadAlignStats *s);

/* Host buffers: arguments of seqik_head_angles_ex with RAW r_head / l_head, affine[2] = R, L. */
int seqik_head_angles_raw(const double *r_head, const double *l_head, int64_t n_frames, int32_t n_points,
                          const double *neck, int64_t neck_stride, double rest_head_pitch, double rest_antenna_pitch,
                          int32_t compute_ant, const double *head_roll, const SeqikHeadAffine *affine, double *angles,
                          double *r_aligned, double *l_aligned, const SeqikOptions *opt);

/* Device buffers: only enqueues the kernel on `hip_stream` of the current device; does not synchronise.  A fault that
 * an earlier launch left in the stream's fault word (seqik_check_faults_stream) is reported on entry. */
int seqik_head_angles_raw_device(const double *d_r_head, const double *d_l_head, int64_t n_frames, int32_t n_points,
                                 const double *d_neck, int64_t neck_stride, double rest_head_pitch,
                                 double rest_antenna_pitch, int32_t compute_ant, const double *d_head_roll,
                                 const SeqikHeadAffine *affine, double *d_angles, double *d_r_aligned,
                                 double *d_l_aligned, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* SEQIK_HEAD_ALIGN_H */
