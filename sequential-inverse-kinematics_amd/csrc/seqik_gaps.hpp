// seqik_gaps.hpp -- the per-frame rules of skip mode (include/seqik_gaps.h), host and device.
//
// The kernels of seqik_gaps.hip and the host test harness (tests/harness/gaps_harness.hip) share these functions:
//   gaps_rows / gaps_frame_missing   which key points a solver reads, and the mask test on one 5x3 record
//   gaps_slot                        where an original frame's record goes in the compacted and padded recording
//   gaps_pad_value                   what a padding slot holds: the chain's last non-missing record, or the filler
//   gaps_expand_value                what an output element of an original frame holds after the solve
// gaps_compact_chain / gaps_expand_chain apply them to one chain frame by frame: the host restatement of the contract.
#pragma once
#include "seqik_core.hpp"
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
