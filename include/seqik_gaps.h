/*
 * seqik_gaps.h -- solving recordings with missing key points by skipping the gap frames (libseqik_hip.so, gfx950).
 *
 * Triangulation pipelines (Anipose, DeepFly3D) write NaN where a key point was not found.  The solvers of seqik.h refuse
 * nothing and check nothing per frame: a non-finite key point makes that solve run to max_nfev and return the warm start.
 * These entry points add an OPT-IN "skip" mode with an exact contract; the solvers themselves are not changed.
 *
 * A leg-frame is MISSING when a coordinate of a key point the solver reads for it is non-finite (NaN, +-inf):
 *   sequential chain (seqik_solve_seq)      rows 0-4;  with the fused alignment (SeqikAffine) rows 1-4
 *   generic chain    (seqik_solve_generic)  rows 0, 4; with the fused alignment row 4
 * (the fused alignment replaces row 0 by template_coxa).  Every chain (sequence, leg) is solved as if its missing frames
 * were not in the recording: frame t is warm-started from the last non-missing frame before it, the first non-missing
 * frame from the seeds (or init_angles).  Precisely, the outputs of a non-missing leg-frame are bit for bit those of the
 * existing solver, with the same options, on the COMPACTED AND PADDED recording: the chain's non-missing frames in
 * order, then copies of its last non-missing frame up to n_frames.  The serial walk being causal, that is also the solve
 * of the recording with the missing frames deleted; the frame-chunk geometry depends on n_frames alone, so chunked
 * results are pinned as well.  A missing leg-frame gets NaN angles and FK, status SEQIK_STATUS_MISSING (every stage
 * entry), nfev 0.  A chain without any non-missing frame is solved on a finite filler (the straight leg: key point k at
 * (0, 0, -(seg[0] + ... + seg[k-1])), which is -0.0 for key point 0) and all its outputs are then missing; the call still
 * returns SEQIK_OK.
 *
 * Layouts are the dense ones of seqik.h:
 *   pose, cpose  [n_seq][n_legs][n_frames][5][3]
 *   map          int32 [n_seq][n_legs][n_frames]: compact slot of each original frame, -1 = missing
 *   n_valid      int32 [n_seq][n_legs]: non-missing frames per chain
 *   angles [..][n_frames][7], fk [..][n_frames][9][3], status / nfev int32 [..][n_frames][4] (seq) or [..][n_frames]
 *   (generic): the solvers' own.
 *
 * Only runs of all four stages on the dense layout are supported; frame sharding (frame_lead, chunk_resume,
 * chunk_states) and the per-chunk report (chunk_flags) are not; the slab-streaming pipeline has skip mode through the
 * entry points of seqik_stream_gaps.h.  SeqikOptions.chunk_stats (HOST memory here) reports the
 * chunks of the compacted recording.  Return codes and seqik_last_error() as in seqik.h.  SEQIK_ERR_BAD_ARG: null
 * buffers, n_legs outside 1..8, a negative size, n_frames >= 2^31, unknown flags, a stage subset, unsupported options.
 * A call with no leg-frames returns SEQIK_OK without a launch.
 */
#ifndef SEQIK_GAPS_H
#define SEQIK_GAPS_H

#include "seqik.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status of a missing leg-frame; scipy's statuses are -1..4 */
#define SEQIK_STATUS_MISSING (-100)

/* flags: the solver the pose is for, and whether its fused alignment (SeqikAffine) is used */
#define SEQIK_GAPS_SEQ 0
#define SEQIK_GAPS_GENERIC 1
#define SEQIK_GAPS_AFFINE 2

/* Device buffers, only enqueues on `hip_stream` (hipStream_t; NULL = the default stream) of the current device and does
 * not synchronise.  Writes d_cpose (every slot), d_map and d_n_valid.  `legs` (host, [n_legs]): only seg is read, for the
 * filler of a chain without any non-missing frame. */
int seqik_gaps_compact_device(const double *d_pose, int64_t n_seq, int32_t n_legs, int64_t n_frames, int32_t flags,
                              const SeqikLegParams *legs, double *d_cpose, int32_t *d_map, int32_t *d_n_valid,
                              void *hip_stream);

/* Device buffers, enqueue only: out[frame] = compact[map[frame]] for every non-missing frame, and NaN angles / NaN FK /
 * SEQIK_STATUS_MISSING / nfev 0 for the missing ones.  flags: SEQIK_GAPS_SEQ (status / nfev have 4 entries per
 * leg-frame) or SEQIK_GAPS_GENERIC (1 entry); the affine bit is ignored.  Each of fk, status and nfev is nullable, as a
 * pair (compact and expanded both given, or both NULL). */
int seqik_gaps_expand_device(const int32_t *d_map, int64_t n_seq, int32_t n_legs, int64_t n_frames, int32_t flags,
                             const double *d_cangles, const double *d_cfk, const int32_t *d_cstatus,
                             const int32_t *d_cnfev, double *d_angles, double *d_fk, int32_t *d_status, int32_t *d_nfev,
                             void *hip_stream);

/* Host buffers, blocking: copies in, then compact -> seqik_solve_seq_device -> expand on a pooled stream of opt->device,
 * copies out.  Arguments as for seqik_solve_seq (first_stage / last_stage must be 1 / 4; angles is output only);
 * n_valid nullable. */
int seqik_solve_seq_gaps(const double *pose, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                         const SeqikLegParams *legs, int32_t first_stage, int32_t last_stage, double *angles,
                         double *fk, int32_t *status, int32_t *nfev, const double *init_angles,
                         const SeqikAffine *affine, const SeqikOptions *opt, int32_t *n_valid);

/* The same with seqik_solve_generic_device. */
int seqik_solve_generic_gaps(const double *pose, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                             const SeqikLegParams *legs, double *angles, double *fk, int32_t *status, int32_t *nfev,
                             const double *init_angles, const SeqikAffine *affine, const SeqikOptions *opt,
                             int32_t *n_valid);

#ifdef __cplusplus
}
#endif

#endif /* SEQIK_GAPS_H */
