// seqik_gaps.hpp -- the per-frame rules of skip mode (include/seqik_gaps.h), host and device.
//
// The kernels of seqik_gaps.hip and the host test harness (tests/harness/gaps_harness.hip) share these functions:
//   gaps_rows / gaps_frame_missing   which key points a solver reads, and the mask test on one 5x3 record
//   gaps_slot                        where an original frame's record goes in the compacted and padded recording
//   gaps_pad_value                   what a padding slot holds: the chain's last non-missing record, or the filler
//   gaps_expand_value                what an output element of an original frame holds after the solve
// gaps_compact_chain / gaps_expand_chain apply them to one chain frame by frame: the host restatement of the contract.
// Streams in skip mode (include/seqik_stream_gaps.h, seqik_stream.hip) add two rules about the state a chain carries
// from one time slab to the next:
//   gaps_carry_slot                  which compact slot of a solved slab is the chain's new state, or none
//   stream_seed_state                the state that stands for "no init_angles": every stage's start values
#pragma once
#include "seqik_core.hpp"
#include "seqik_generic.hpp"
#include "../../include/seqik_gaps.h"

namespace seqik {

constexpr int kGapsRec = 15;  // doubles per key-point record (5 rows x 3)

// The filler of a chain without any non-missing frame: the straight leg, key point k at (0, 0, -(seg[0] + .. + seg[k-1])).
struct GapsLeg {
    double z[5];
};

inline void make_gaps_leg(const SeqikLegParams &lp, GapsLeg &gl)
{
    // z[k] = -(seg[0] + .. + seg[k-1]); the empty sum of key point 0 is negated too: -0.0, as numpy's -cumsum gives it
    double s = 0.0;
    for (int k = 0; k < 5; ++k) {
        gl.z[k] = -s;
        if (k < 4) s += lp.seg[k];
    }
}

// bit k set = key point k is read by the solver: seq rows 0-4, generic rows 0 and 4; the fused alignment drops row 0
SEQIK_HD unsigned gaps_rows(int flags)
{
    const unsigned rows = (flags & SEQIK_GAPS_GENERIC) ? 0x11u : 0x1fu;
    return (flags & SEQIK_GAPS_AFFINE) ? (rows & ~1u) : rows;
}

// element e (0..14) of a record counts for the mask
SEQIK_HD bool gaps_element_read(unsigned rows, int e) { return (rows >> (e / 3)) & 1u; }

SEQIK_HD bool gaps_frame_missing(const double *rec, unsigned rows)
{
    bool missing = false;
#pragma unroll
    for (int e = 0; e < kGapsRec; ++e) missing = missing || (gaps_element_read(rows, e) && !is_finite(rec[e]));
    return missing;
}

// original frame t with valid-rank r (non-missing frames before it) in a chain with n_valid non-missing frames
SEQIK_HD int64_t gaps_slot(bool missing, int64_t t, int64_t r, int64_t n_valid)
{
    return missing ? n_valid + (t - r) : r;
}

// element e of a padding slot: the last non-missing record (nullable when the chain has none: the filler)
SEQIK_HD double gaps_pad_value(const double *last, const GapsLeg &gl, int e)
{
    double z = gl.z[0];
#pragma unroll
    for (int k = 1; k < 5; ++k) z = (e / 3 == k) ? gl.z[k] : z;  // static indices: no private array on the device
    return last ? last[e] : (e % 3 == 2 ? z : 0.0);
}

// element k of an expanded record: the compact record of slot m, or `fill` for a missing frame (m < 0)
template <typename T>
SEQIK_HD T gaps_expand_value(const T *compact, int32_t m, int width, int k, T fill)
{
    return m >= 0 ? compact[(int64_t)m * width + k] : fill;
}

// Carried streams: the compact slot whose angles are the chain's state after a slab with n_valid non-missing frames --
// the last non-missing frame (the slots behind it are padding, re-solves of that frame from its own solution) -- or -1:
// the slab had no such frame and the chain keeps the state it came with.
SEQIK_HD int64_t gaps_carry_slot(int64_t n_valid) { return n_valid > 0 ? n_valid - 1 : -1; }

// One chain's carry on the host: cangles [N][7] of the solved compact slab -> state [7] (left alone without a valid frame).
inline void gaps_carry_chain(const double *cangles, int64_t n_valid, double *state)
{
    const int64_t slot = gaps_carry_slot(n_valid);
    if (slot < 0) return;
    for (int d = 0; d < 7; ++d) state[d] = cangles[slot * 7 + d];
}

// The init_angles [7] (DOF order of the ABI) that are bit-equivalent to none.  A solver kernel reads init only where it
// would otherwise read a seed, and reads it raw, as it reads the seed:
//   sequential chain  stage s starts its active links from init[first DOF of the stage ..] in place of
//                     seeds[kSeedOffset[s] + kFirstActive[s] + j] (seqik_consts.hpp): seeds 1, 2 | 7, 8 | 15, 16 | 25
//   generic chain     link i (0..6) starts from init[generic_link_dof(i)] in place of seeds[19 + i]
inline void stream_seed_state(const SeqikLegParams &lp, bool generic, double *state)
{
    static const int seq_seed[7] = {1, 2, 7, 8, 15, 16, 25};
    for (int i = 0; i < 7; ++i) {
        if (generic) state[generic_link_dof(i)] = lp.seeds[19 + i];
        else state[i] = lp.seeds[seq_seed[i]];
    }
}

// One chain on the host: pose [N][15] -> cpose [N][15], map [N]; returns n_valid.
inline int64_t gaps_compact_chain(const double *pose, int64_t N, unsigned rows, const GapsLeg &gl, double *cpose,
                                  int32_t *map)
{
    int64_t n_valid = 0, last = -1;
    for (int64_t t = 0; t < N; ++t)
        if (!gaps_frame_missing(pose + t * kGapsRec, rows)) { ++n_valid; last = t; }
    const double *last_rec = last >= 0 ? pose + last * kGapsRec : nullptr;
    int64_t r = 0;
    for (int64_t t = 0; t < N; ++t) {
        const bool missing = gaps_frame_missing(pose + t * kGapsRec, rows);
        const int64_t s = gaps_slot(missing, t, r, n_valid);
        for (int e = 0; e < kGapsRec; ++e)
            cpose[s * kGapsRec + e] = missing ? gaps_pad_value(last_rec, gl, e) : pose[t * kGapsRec + e];
        map[t] = missing ? -1 : (int32_t)r;
        if (!missing) ++r;
    }
    return n_valid;
}

// One chain on the host: compact [N][width] -> out [N][width] in original frame order.
template <typename T>
void gaps_expand_chain(const int32_t *map, int64_t N, const T *compact, int width, T fill, T *out)
{
    for (int64_t t = 0; t < N; ++t)
        for (int k = 0; k < width; ++k) out[t * width + k] = gaps_expand_value(compact, map[t], width, k, fill);
}

}  // namespace seqik
