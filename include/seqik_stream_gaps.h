/*
 * seqik_stream_gaps.h -- skip mode (seqik_gaps.h) for the slab-streaming pipeline (seqik.h, "Streaming"): recordings
 * that do not fit in HBM, or arrive in pieces, with missing key points (libseqik_hip.so, gfx950).
 *
 * Additive to ABI 7.  seqik_stream_open_skip opens a SeqikStream whose seqik_stream_submit runs, per slab and on the
 * slot's compute stream: seqik_gaps_compact_device -> the solver's device entry on the compacted slab -> (carried
 * streams) the carry selection -> seqik_gaps_expand_device into the slot's angle and FK buffers -> the copy to the host
 * as before.  Which leg-frames are MISSING is decided by the rules of seqik_gaps.h (rows 0-4, generic rows 0 and 4; row 0
 * is ignored with the fused alignment); they arrive on the host as NaN angles and NaN FK.  Every other call of the
 * stream (submit, wait, set_carry, reset_carry, close) is the one of seqik.h.
 *
 * Contract.  state_k is [n_seq][n_legs][7] joint angles in DOF order.
 *   - Slab k of a skip stream returns what seqik_solve_seq_gaps / seqik_solve_generic_gaps returns for that slab with the
 *     same options; on a carried stream with init_angles = state_k.
 *   - state_{k+1}[chain] is the slab's angles at the chain's last non-missing frame, or state_k[chain] when the slab has
 *     none.  state_0 is the SEED STATE (seqik_stream_seed_state), or what seqik_stream_set_carry gave;
 *     seqik_stream_reset_carry goes back to the seed state.
 *   - The seed state is bit-equivalent to "no init_angles": a solver reads init_angles only in place of the start values
 *     of each stage's active joints, and the seed state holds exactly those.  Hence, with frame_chunk = 0, a carried
 *     skip stream over consecutive time slabs equals seqik_solve_*_gaps of the unsplit recording bit for bit, and a skip
 *     stream without carry equals seqik_solve_*_gaps of the unsplit batch bit for bit.
 *   - A chain with no non-missing frame in a slab is solved on the straight-leg filler (seqik_gaps.h) and reported NaN
 *     throughout.
 *   - A stream opened with seqik_stream_open behaves exactly as before.
 *
 * Only the dense layout is supported.  Each slot additionally owns the compacted pose, the frame map, n_valid and the
 * compact angles and FK (allocated at open): 180 B more per leg-frame, 396 B with FK, + 4 B per chain.
 */
#ifndef SEQIK_STREAM_GAPS_H
#define SEQIK_STREAM_GAPS_H

#include "seqik_gaps.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Parameters as for seqik_stream_open (frame_chunk, frame_halo and chunk_tol of `opt` included).  layout must be NULL:
 * SEQIK_ERR_BAD_ARG otherwise, before any device is touched. */
int seqik_stream_open_skip(SeqikStream **out, int32_t n_legs, const SeqikLegParams *legs, const SeqikAffine *affine,
                           int64_t slab_seq, int64_t n_frames, const SeqikLayout *layout, int32_t want_fk,
                           int32_t n_slots, int32_t carry, int32_t generic, const SeqikOptions *opt);

/* state: host [n_legs][7].  The init_angles that are bit-equivalent to none: for the sequential chain
 * seeds[1, 2, 7, 8, 15, 16, 25] (the active joints of stages 1-4), for the generic chain (generic != 0) the seeds of its
 * seven joints, seeds[19 .. 25], in DOF order.  Host code only; needs no GPU. */
int seqik_stream_seed_state(const SeqikLegParams *legs, int32_t n_legs, int32_t generic, double *state);

/* state: host [n_seq][n_legs][7], n_seq in 1..slab_seq.  Blocking: waits for the slabs submitted so far and returns the
 * state the next slab of a carried stream would start from (in skip mode the last frame of a slab may be missing, so
 * the state cannot be read off the angles).  Works on carried streams of seqik_stream_open too.  SEQIK_ERR_BAD_ARG on a
 * stream opened without carry, and on a carried stream of seqik_stream_open that has no state yet. */
int seqik_stream_get_carry(SeqikStream *s, double *state, int64_t n_seq);

#ifdef __cplusplus
}
#endif

#endif /* SEQIK_STREAM_GAPS_H */
