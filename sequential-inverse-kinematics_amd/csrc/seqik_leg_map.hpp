// seqik_leg_map.hpp -- what the units that map joint angles (S, L, N, 7) to one record per leg-frame share: forward
// kinematics (seqik_fk.hip), link frames (seqik_frames.hip), leg Jacobians (seqik_jacobian.hip), fit sensitivity
// (seqik_sensitivity.hip) and refinement (seqik_refine.hip).  The tail of their kernel arguments, the argument checks they
// have in common, the launch plan with its environment switches, and the quarter-record staged store path of frames,
// Jacobians and sensitivity.  The kernels' outer loops, their reductions and their own pointer rules stay in the units;
// the device rules they share are in seqik_leg_chain.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "seqik_leg_chain.hpp"
#include "seqik_runtime.hpp"

namespace seqik {

// ---- the tail of FkArgs / FramesArgs / JacArgs: which leg a flat leg-frame index belongs to ----
struct LegFrameIndex {
    int64_t n_frames;  // leg-frame i belongs to leg (i / n_frames) % n_legs
    int64_t n_total;   // n_seq * n_legs * n_frames
    int32_t n_legs;
    int32_t pad_;
    FkLeg legs[kFkMaxLegs];  // entries past n_legs repeat leg 0: all eight hold finite values

    void fill(int64_t total, int32_t legs_given, int64_t frames, const SeqikLegParams *lp)
    {
        n_frames = frames; n_total = total; n_legs = legs_given; pad_ = 0;
        for (int l = 0; l < kFkMaxLegs; ++l) make_fk_leg(lp[l < n_legs ? l : 0], legs[l]);
    }
    __device__ __forceinline__ int leg_of(int64_t i) const { return (int)((i / n_frames) % n_legs); }
};

// ---- the checks the entry points share, made before anything touches HIP ----
// `row`: doubles of the widest per-leg-frame array of the call; *n_total receives n_seq * n_legs * n_frames, whose byte
// count at that width must fit in 63 bits.  The units add their own pointer rules.
inline int check_leg_map(const char *who, int64_t n_seq, int32_t n_legs, int64_t n_frames, const SeqikLegParams *legs,
                         int32_t kind, int row, int64_t *n_total)
{
    if (n_legs < 1 || n_legs > kFkMaxLegs) return bad_arg(who, "n_legs must lie in 1..8");
    if (n_seq < 0 || n_frames < 0) return bad_arg(who, "negative n_seq or n_frames");
    if (!legs) return bad_arg(who, "legs must not be null");
    if (kind != SEQIK_FK_KIND_SEQ && kind != SEQIK_FK_KIND_GENERIC)
        return bad_arg(who, "kind must be 0 (sequential chain) or 1 (generic chain)");
    if (int rc = check_segments(who, legs, n_legs)) return rc;
    return leg_frames_fit(who, n_seq, n_legs, n_frames, n_total, row);
}

// ---- the launch plan ----
// One leg-frame per lane, grid-stride.  Three switches per unit select variants for measurements and tests; they are
// read per call, so that one process can run them all (prefix: SEQIK_FK, SEQIK_FRAMES, SEQIK_JAC, SEQIK_SENS, SEQIK_REFINE):
//   <prefix>_STAGED  0 / 1: the per-lane or the LDS-staged kernel (default 1, where the unit allows staging at all)
//   <prefix>_BLOCK   threads per workgroup: a multiple of 64 from 64 to the unit's maximum, anything else means 256; a
//                    staged launch takes at most the unit's staged maximum (its LDS per workgroup)
//   <prefix>_GRID    a cap on the number of workgroups (>= 1), so that a test reaches the grid-stride loop at a small size
struct LegMapPlan {
    bool staged;
    int block;
    int64_t blocks;
    size_t lds_bytes;
};

inline int leg_map_switch(const char *prefix, const char *name, int absent)
{
    char var[48];
    snprintf(var, sizeof var, "%s%s", prefix, name);
    const char *v = getenv(var);
    return v ? atoi(v) : absent;
}

inline LegMapPlan plan_leg_map(const char *prefix, int64_t n_total, bool staged_allowed, int max_block_per_lane,
                               int max_block_staged, int lds_doubles_per_wave)
{
    LegMapPlan p;
    p.staged = staged_allowed && leg_map_switch(prefix, "_STAGED", 1) != 0;
    p.block = leg_map_switch(prefix, "_BLOCK", 256);
    if (p.block < 64 || p.block > max_block_per_lane || p.block % 64) p.block = 256;
    if (p.staged && p.block > max_block_staged) p.block = max_block_staged;
    p.blocks = (n_total + p.block - 1) / p.block;
    if (p.blocks > 256 * 64) p.blocks = 256 * 64;  // grid-stride beyond 64 workgroups per CU (as seqik_head.hip)
    const int cap = leg_map_switch(prefix, "_GRID", 0);
    if (cap >= 1 && p.blocks > cap) p.blocks = cap;
    p.lds_bytes = p.staged ? sizeof(double) * lds_doubles_per_wave * (p.block / 64) : 0;
    return p;
}

// SEQIK_OK, or the error of the launch
template <typename Args>
int launch_leg_map(void (*kernel)(Args), const LegMapPlan &p, const Args &a, void *hip_stream)
{
    hipLaunchKernelGGL(kernel, dim3((unsigned)p.blocks), dim3(p.block), p.lds_bytes, static_cast<hipStream_t>(hip_stream), a);
    return launched();
}

// ---- the staged store path of frames, Jacobians and sensitivity (the per-lane path stores through ArraySink) ----
constexpr int kSubTile = 16;  // leg-frames per pass: four lanes share a record, each keeps a quarter of it

// One pass: every lane writes its quarter (QUAD doubles) to the wavefront's LDS at lane * QUAD (<= 63 * QUAD + QUAD - 1,
// inside the 64 * QUAD doubles at `st`), then the wavefront stores the kSubTile records at `global_row0` as QUAD fully
// coalesced rows of 64 doubles (non-temporal: written once).
template <int QUAD>
__device__ __forceinline__ void store_quad_pass(double *st, int lane, const double *buf, double *global_row0)
{
#pragma unroll
    for (int j = 0; j < QUAD; ++j) st[lane * QUAD + j] = buf[j];
    wave_lds_fence();
#pragma unroll
    for (int k = 0; k < QUAD; ++k) __builtin_nontemporal_store(st[k * 64 + lane], global_row0 + k * 64 + lane);
    wave_lds_fence();  // the next pass's LDS writes stay behind these reads
}

// The 64 records (4 * QUAD doubles each, at `out`) of a whole wavefront from leg-frame w0 (w0 + 64 <= n_total), in four
// passes of kSubTile through `st` (64 * QUAD doubles of LDS): `rule(rec, sink)` hands record rec to the lane's QuadSink.
template <int QUAD, class Rule>
__device__ __forceinline__ void staged_quad_passes(double *st, int lane, int64_t w0, double *out, Rule rule)
{
#pragma unroll 1
    for (int p = 0; p < 64 / kSubTile; ++p) {
        const int64_t r0 = w0 + p * kSubTile, rec = r0 + (lane >> 2);  // rec < w0 + 64
        QuadSink<QUAD> sink;
        sink.q = lane & 3;
        rule(rec, sink);
        store_quad_pass<QUAD>(st, lane, sink.buf, out + r0 * (4 * QUAD));
    }
}

}  // namespace seqik
