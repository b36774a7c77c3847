// seqik_gaps.hip -- skip mode for missing key points: kernels and C ABI entry points (include/seqik_gaps.h).
//
// Compaction is a stable partition of every chain's frames into "non-missing, in order" and "padding", in four
// launches over the dense pose [chain][frame][5][3]:
//   count    one wavefront per TILE of F = 64 k frames of one chain (k = 1 unless a chain has more than 65 536 frames,
//            then as small as keeps a chain at <= 1024 tiles).  The wavefront brings 64 records at a time into LDS with
//            15 fully coalesced loads, marks the frames that hold a non-finite key point the solver reads, and counts the
//            others with a 64-bit ballot.  The tile count goes into the first map word of the tile (or, for one tile per
//            chain, straight into n_valid).
//   scan     (only with more than one tile per chain) one wavefront per chain: exclusive scan of its <= 1024 tile counts
//            (16 rows of 64, shuffle scan with carry), written back in place; n_valid.
//   permute  the count pass again, and then every non-missing frame of rank r writes its record to slot r: the ranks of
//            a wavefront's valid frames are consecutive, so the wavefront gathers them in LDS and stores one contiguous
//            block with coalesced stores.  map = r or -1.
//   pad      slots n_valid .. N-1 of every chain (the slots of the missing frames) receive the chain's last non-missing
//            record -- slot n_valid - 1 of the compacted recording, complete once permute has run -- or the filler.
// Expansion is one lane per original leg-frame: a wavefront's 64 frames read a contiguous run of compact slots, which it
// loads coalesced into LDS; each lane picks its record (or the fill value) and the block is stored coalesced.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "seqik_gaps.hpp"
#include "seqik_runtime.hpp"
#include "../../include/seqik_gaps.h"

namespace {

using seqik::bad_arg;
using seqik::kFkRow;
using seqik::kGapsRec;
using seqik::kMaxTiles;  // tiles per chain (scan: 16 rows of 64 lanes)
using seqik::wave_lds_fence;

constexpr int kMaxLegs = 8;
constexpr int kBlock = 256;            // threads per workgroup: 4 independent wavefronts
constexpr int kWaves = kBlock / 64;

struct GapsGeom {
    int64_t n_frames;  // N
    int64_t n_chains;  // C = n_seq * n_legs
    int64_t tile;      // F, frames per tile
    int64_t tiles;     // T, tiles per chain
    int32_t n_legs;
    uint32_t rows;     // seqik::gaps_rows(flags)
};

struct CompactArgs {
    GapsGeom g;
    const double *pose;
    double *cpose;
    int32_t *map;
    int32_t *n_valid;
    seqik::GapsLeg legs[kMaxLegs];
};

__device__ __forceinline__ uint64_t lanes_below(int lane) { return (1ull << lane) - 1ull; }

// Brings the records of frames [0, nf) (nf <= 64) at `src` into rec (64 x 15 doubles) with coalesced loads and returns
// whether this lane's frame is non-missing (KEEP false: only the test, rec is not written).  bad: 64 ints of LDS.
template <bool KEEP>
__device__ __forceinline__ bool stage_records(const double *src, int nf, uint32_t rows, double *rec, int *bad, int lane)
{
    bad[lane] = 0;
    wave_lds_fence();
    const int n = nf * kGapsRec;
#pragma unroll
    for (int k = 0; k < kGapsRec; ++k) {
        const int e = k * 64 + lane;
        if (e < n) {
            const double v = __builtin_nontemporal_load(src + e);
            if (KEEP) rec[e] = v;
            if (seqik::gaps_element_read(rows, e % kGapsRec) && !seqik::is_finite(v)) bad[e / kGapsRec] = 1;
        }
    }
    wave_lds_fence();
    return lane < nf && !bad[lane];
}

__device__ __forceinline__ void tile_of(const GapsGeom &g, int64_t wid, int64_t &c, int64_t &f0, int64_t &f1)
{
    c = wid / g.tiles;
    f0 = (wid % g.tiles) * g.tile;
    f1 = f0 + g.tile < g.n_frames ? f0 + g.tile : g.n_frames;
}

__global__ void __launch_bounds__(kBlock) seqik_gaps_count_kernel(CompactArgs a)
{
    __shared__ int s_bad[kWaves][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t wid = (int64_t)blockIdx.x * kWaves + wave;
    if (wid >= a.g.n_chains * a.g.tiles) return;
    int64_t c, f0, f1;
    tile_of(a.g, wid, c, f0, f1);
    const double *base = a.pose + c * a.g.n_frames * kGapsRec;
    int32_t cnt = 0;
    for (int64_t b = f0; b < f1; b += 64) {
        const int nf = (int)(f1 - b < 64 ? f1 - b : 64);
        const bool valid = stage_records<false>(base + b * kGapsRec, nf, a.g.rows, nullptr, s_bad[wave], lane);
        cnt += __popcll(__ballot(valid));
    }
    if (lane == 0) {
        if (a.g.tiles == 1) a.n_valid[c] = cnt;
        else a.map[c * a.g.n_frames + f0] = cnt;
    }
}

// one wavefront per chain: tile counts (first map word of each tile) -> exclusive prefix in place, n_valid
__global__ void __launch_bounds__(kBlock) seqik_gaps_scan_kernel(CompactArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c = (int64_t)blockIdx.x * kWaves + wave;
    if (c >= a.g.n_chains) return;
    int32_t *words = a.map + c * a.g.n_frames;
    int32_t v[kMaxTiles / 64];
#pragma unroll
    for (int i = 0; i < kMaxTiles / 64; ++i) {
        const int64_t j = (int64_t)i * 64 + lane;
        v[i] = j < a.g.tiles ? words[j * a.g.tile] : 0;
    }
    int32_t carry = 0;
#pragma unroll
    for (int i = 0; i < kMaxTiles / 64; ++i) {
        int32_t x = v[i];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        const int64_t j = (int64_t)i * 64 + lane;
        if (j < a.g.tiles) words[j * a.g.tile] = carry + x - v[i];
        carry += __shfl(x, 63, 64);
    }
    if (lane == 0) a.n_valid[c] = carry;
}

__global__ void __launch_bounds__(kBlock) seqik_gaps_permute_kernel(CompactArgs a)
{
    __shared__ double s_rec[kWaves][64 * kGapsRec];
    __shared__ int s_bad[kWaves][64];
    __shared__ int s_pos[kWaves][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t wid = (int64_t)blockIdx.x * kWaves + wave;
    if (wid >= a.g.n_chains * a.g.tiles) return;
    int64_t c, f0, f1;
    tile_of(a.g, wid, c, f0, f1);
    const int64_t N = a.g.n_frames;
    const double *base = a.pose + c * N * kGapsRec;
    int32_t *map = a.map + c * N;
    double *cbase = a.cpose + c * N * kGapsRec;
    // the tile's first rank (read by every lane before lane 0 overwrites that word with a map entry below)
    int64_t r = a.g.tiles == 1 ? 0 : map[f0];
    double *rec = s_rec[wave];
    int *pos = s_pos[wave];
    for (int64_t b = f0; b < f1; b += 64) {
        const int nf = (int)(f1 - b < 64 ? f1 - b : 64);
        const bool valid = stage_records<true>(base + b * kGapsRec, nf, a.g.rows, rec, s_bad[wave], lane);
        const uint64_t mask = __ballot(valid);
        const int cv = __popcll(mask);
        const int rank = __popcll(mask & lanes_below(lane));
        if (valid) pos[rank] = lane;
        if (lane < nf) map[b + lane] = valid ? (int32_t)(r + rank) : -1;
        wave_lds_fence();
        double *dst = cbase + r * kGapsRec;
        for (int e = lane; e < cv * kGapsRec; e += 64) {
            const int f = e / kGapsRec;
            dst[e] = rec[pos[f] * kGapsRec + (e - f * kGapsRec)];
        }
        r += cv;
        wave_lds_fence();  // the next block's LDS writes stay behind these reads
    }
}

// slots [n_valid, N) of every chain: one workgroup per chain and block of kBlock slots
__global__ void __launch_bounds__(kBlock) seqik_gaps_pad_kernel(CompactArgs a, int64_t blocks_per_chain)
{
    const int64_t c = blockIdx.x / blocks_per_chain;
    const int64_t s0 = (blockIdx.x % blocks_per_chain) * kBlock;
    const int64_t N = a.g.n_frames;
    const int64_t s1 = s0 + kBlock < N ? s0 + kBlock : N;
    const int64_t nv = a.n_valid[c];
    if (s1 <= nv) return;
    double *cbase = a.cpose + c * N * kGapsRec;
    const double *last = nv > 0 ? cbase + (nv - 1) * kGapsRec : nullptr;
    // this chain's filler, copied with static indices (a dynamically indexed kernel argument would go to scratch)
    const int leg = (int)(c % a.g.n_legs);
    seqik::GapsLeg gl = a.legs[0];
#pragma unroll
    for (int l = 1; l < kMaxLegs; ++l)
        if (l == leg) gl = a.legs[l];
    double *dst = cbase + s0 * kGapsRec;
    const int n = (int)(s1 - s0) * kGapsRec;
    for (int e = threadIdx.x; e < n; e += kBlock) {
        const int f = e / kGapsRec;
        if (s0 + f >= nv) dst[e] = seqik::gaps_pad_value(last, gl, e - f * kGapsRec);
    }
}

struct ExpandArgs {
    const int32_t *map;
    const double *cangles, *cfk;
    const int32_t *cstatus, *cnfev;
    double *angles, *fk;
    int32_t *status, *nfev;
    int64_t n_frames, n_chains, blocks_per_chain;
    int32_t status_width;  // 4 (seq: one entry per stage) or 1 (generic)
};

// A wavefront's nf frames take the nv consecutive compact records from `src` (LDS-staged), the others `fill`.
template <typename T, int W>
__device__ __forceinline__ void expand_block(const T *src, T *dst, int nv, int nf, const int *lrank, T *stage, T fill,
                                             int lane)
{
    for (int e = lane; e < nv * W; e += 64) stage[e] = src[e];
    wave_lds_fence();
    for (int e = lane; e < nf * W; e += 64) {
        const int f = e / W;
        dst[e] = seqik::gaps_expand_value<T>(stage, lrank[f], W, e - f * W, fill);
    }
    wave_lds_fence();
}

template <int SW>
__global__ void __launch_bounds__(kBlock) seqik_gaps_expand_kernel(ExpandArgs a)
{
    __shared__ double s_stage[kWaves][64 * kFkRow];
    __shared__ int s_rank[kWaves][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t wid = (int64_t)blockIdx.x * kWaves + wave;
    if (wid >= a.n_chains * a.blocks_per_chain) return;
    const int64_t c = wid / a.blocks_per_chain, f0 = (wid % a.blocks_per_chain) * 64;
    const int nf = (int)(a.n_frames - f0 < 64 ? a.n_frames - f0 : 64);
    const int64_t i0 = c * a.n_frames + f0;  // first leg-frame of this wavefront
    const int32_t m = lane < nf ? a.map[i0 + lane] : -1;
    const uint64_t mask = __ballot(m >= 0);
    const int nv = __popcll(mask);
    const int32_t r0 = __shfl(m, nv ? __builtin_ctzll(mask) : 0, 64);  // the slots of a wavefront are consecutive
    s_rank[wave][lane] = m >= 0 ? m - r0 : -1;
    wave_lds_fence();
    const int64_t s0 = c * a.n_frames + (nv ? r0 : 0);  // first compact leg-frame
    const double nan = __builtin_nan("");
    double *st = s_stage[wave];
    expand_block<double, 7>(a.cangles + s0 * 7, a.angles + i0 * 7, nv, nf, s_rank[wave], st, nan, lane);
    if (a.fk) expand_block<double, kFkRow>(a.cfk + s0 * kFkRow, a.fk + i0 * kFkRow, nv, nf, s_rank[wave], st, nan, lane);
    int32_t *sti = reinterpret_cast<int32_t *>(st);
    if (a.status)
        expand_block<int32_t, SW>(a.cstatus + s0 * SW, a.status + i0 * SW, nv, nf, s_rank[wave], sti,
                                  (int32_t)SEQIK_STATUS_MISSING, lane);
    if (a.nfev)
        expand_block<int32_t, SW>(a.cnfev + s0 * SW, a.nfev + i0 * SW, nv, nf, s_rank[wave], sti, (int32_t)0, lane);
}

// sizes shared by every entry point; *n_total receives n_seq * n_legs * n_frames
int check_sizes(const char *who, int64_t n_seq, int32_t n_legs, int64_t n_frames, int32_t flags, int64_t *n_total)
{
    if (n_legs < 1 || n_legs > kMaxLegs) return bad_arg(who, "n_legs must lie in 1..8");
    if (n_seq < 0 || n_frames < 0) return bad_arg(who, "negative n_seq or n_frames");
    if (n_frames > INT32_MAX) return bad_arg(who, "n_frames must be below 2^31 (the frame map is int32)");
    if (flags & ~(SEQIK_GAPS_GENERIC | SEQIK_GAPS_AFFINE))
        return bad_arg(who, "unknown flags (SEQIK_GAPS_SEQ / _GENERIC, | SEQIK_GAPS_AFFINE)");
    return seqik::leg_frames_fit(who, n_seq, n_legs, n_frames, n_total);
}

}  // namespace

extern "C" {

int seqik_gaps_compact_device(const double *d_pose, int64_t n_seq, int32_t n_legs, int64_t n_frames, int32_t flags,
                              const SeqikLegParams *legs, double *d_cpose, int32_t *d_map, int32_t *d_n_valid,
                              void *hip_stream)
{
    const char *who = "seqik_gaps_compact_device";
    int64_t n = 0;
    int rc = check_sizes(who, n_seq, n_legs, n_frames, flags, &n);
    if (rc != SEQIK_OK) return rc;
    if (!d_pose || !d_cpose || !d_map || !d_n_valid || !legs)
        return bad_arg(who, "pose, cpose, map, n_valid and legs must not be null");
    if ((rc = seqik::check_segments(who, legs, n_legs)) != SEQIK_OK) return rc;
    if (n == 0) return SEQIK_OK;
    CompactArgs a;
    memset(&a, 0, sizeof(a));
    a.g.n_frames = n_frames;
    a.g.n_chains = n_seq * n_legs;
    seqik::tile_geometry(n_frames, &a.g.tile, &a.g.tiles);
    a.g.n_legs = n_legs;
    a.g.rows = seqik::gaps_rows(flags);
    a.pose = d_pose; a.cpose = d_cpose; a.map = d_map; a.n_valid = d_n_valid;
    for (int l = 0; l < kMaxLegs; ++l) seqik::make_gaps_leg(legs[l < n_legs ? l : 0], a.legs[l]);
    const int64_t tile_blocks = seqik::blocks_for(a.g.n_chains * a.g.tiles, kWaves);
    const int64_t pad_per_chain = (n_frames + kBlock - 1) / kBlock;
    if (tile_blocks > UINT32_MAX || a.g.n_chains * pad_per_chain > UINT32_MAX)
        return bad_arg(who, "too many leg-frames for one launch");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    hipLaunchKernelGGL(seqik_gaps_count_kernel, dim3((unsigned)tile_blocks), dim3(kBlock), 0, s, a);
    HIP_TRY(hipGetLastError());
    if (a.g.tiles > 1) {
        hipLaunchKernelGGL(seqik_gaps_scan_kernel, dim3((unsigned)seqik::blocks_for(a.g.n_chains, kWaves)), dim3(kBlock), 0, s, a);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(seqik_gaps_permute_kernel, dim3((unsigned)tile_blocks), dim3(kBlock), 0, s, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(seqik_gaps_pad_kernel, dim3((unsigned)(a.g.n_chains * pad_per_chain)), dim3(kBlock), 0, s, a,
                       pad_per_chain);
    return seqik::launched();
}

int seqik_gaps_expand_device(const int32_t *d_map, int64_t n_seq, int32_t n_legs, int64_t n_frames, int32_t flags,
                             const double *d_cangles, const double *d_cfk, const int32_t *d_cstatus,
                             const int32_t *d_cnfev, double *d_angles, double *d_fk, int32_t *d_status, int32_t *d_nfev,
                             void *hip_stream)
{
    const char *who = "seqik_gaps_expand_device";
    int64_t n = 0;
    int rc = check_sizes(who, n_seq, n_legs, n_frames, flags, &n);
    if (rc != SEQIK_OK) return rc;
    if (!d_map || !d_cangles || !d_angles)
        return bad_arg(who, "map, compact angles and angles must not be null");
    if (!d_cfk != !d_fk || !d_cstatus != !d_status || !d_cnfev != !d_nfev)
        return bad_arg(who, "fk, status and nfev are pairs: compact and expanded both given or both null");
    if (n == 0) return SEQIK_OK;
    ExpandArgs a;
    a.map = d_map; a.cangles = d_cangles; a.cfk = d_cfk; a.cstatus = d_cstatus; a.cnfev = d_cnfev;
    a.angles = d_angles; a.fk = d_fk; a.status = d_status; a.nfev = d_nfev;
    a.n_frames = n_frames;
    a.n_chains = n_seq * n_legs;
    a.blocks_per_chain = (n_frames + 63) / 64;
    const bool generic = flags & SEQIK_GAPS_GENERIC;
    a.status_width = generic ? 1 : 4;
    const int64_t blocks = seqik::blocks_for(a.n_chains * a.blocks_per_chain, kWaves);
    if (blocks > UINT32_MAX) return bad_arg(who, "too many leg-frames for one launch");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (generic) hipLaunchKernelGGL(seqik_gaps_expand_kernel<1>, dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL(seqik_gaps_expand_kernel<4>, dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
    return seqik::launched();
}

}  // extern "C"

namespace {

// The host-buffer skip-mode solve of either chain kind: copies in, compact -> solver's device entry -> expand, copies out.
int solve_gaps(bool generic, const double *pose, int64_t n_seq, int32_t n_legs, int64_t n_frames,
               const SeqikLegParams *legs, int32_t first_stage, int32_t last_stage, double *angles, double *fk,
               int32_t *status, int32_t *nfev, const double *init_angles, const SeqikAffine *affine,
               const SeqikOptions *opt, int32_t *n_valid)
{
    const char *who = generic ? "seqik_solve_generic_gaps" : "seqik_solve_seq_gaps";
    const int32_t flags = (generic ? SEQIK_GAPS_GENERIC : SEQIK_GAPS_SEQ) | (affine ? SEQIK_GAPS_AFFINE : 0);
    int64_t n = 0;
    int rc = check_sizes(who, n_seq, n_legs, n_frames, flags, &n);
    if (rc != SEQIK_OK) return rc;
    if (!pose || !angles || !legs) return bad_arg(who, "pose, angles and legs must not be null");
    if (first_stage != 1 || last_stage != 4)
        return bad_arg(who, "skip mode runs all four stages (first_stage 1, last_stage 4)");
    if (opt && (opt->frame_lead || opt->chunk_resume || opt->chunk_states || opt->chunk_flags))
        return bad_arg(who, "frame_lead, chunk_resume, chunk_states and chunk_flags are not supported in skip mode");
    if ((rc = seqik::check_segments(who, legs, n_legs)) != SEQIK_OK) return rc;
    if (n == 0) return SEQIK_OK;
    const size_t n_lf = (size_t)n, n_ch = (size_t)n_seq * n_legs;
    const size_t sw = generic ? 1 : 4;  // status / nfev entries per leg-frame
    seqik::HostCall call;
    double *d_pose, *d_init, *d_cpose, *d_cang, *d_cfk, *d_ang, *d_fk;
    int32_t *d_map, *d_cst, *d_cnf, *d_stats, *d_st, *d_nf, *d_nv;
    call.upload(d_pose, kGapsRec * n_lf, pose);
    call.upload(d_init, 7 * n_ch, init_angles);
    call.scratch(d_cpose, kGapsRec * n_lf);
    call.scratch(d_map, n_lf);
    call.scratch(d_cang, 7 * n_lf);
    call.scratch(d_cfk, fk ? kFkRow * n_lf : 0);
    // as the solvers' host entry points: statuses start at -1, counts at 0
    call.scratch(d_cst, status ? sw * n_lf : 0).filled(0xff);
    call.scratch(d_cnf, nfev ? sw * n_lf : 0).filled(0);
    call.download(d_stats, 16, opt ? opt->chunk_stats : nullptr).filled(0);  // stays zero when the call is not chunked
    call.download(d_ang, 7 * n_lf, angles);
    call.download(d_fk, kFkRow * n_lf, fk);
    call.download(d_st, sw * n_lf, status);
    call.download(d_nf, sw * n_lf, nfev);
    // (the compaction needs the counts whether or not the caller wants them)
    call.produce(d_nv, n_ch, n_valid);
    if ((rc = call.begin(opt ? opt->device : -1)) != SEQIK_OK) return rc;
    hipStream_t stream = call.stream();
    SeqikOptions dev_opt;
    if (opt) dev_opt = *opt; else memset(&dev_opt, 0, sizeof(dev_opt));
    dev_opt.chunk_stats = d_stats;
    rc = seqik_gaps_compact_device(d_pose, n_seq, n_legs, n_frames, flags, legs, d_cpose, d_map, d_nv, stream);
    if (rc == SEQIK_OK)
        rc = generic ? seqik_solve_generic_device(d_cpose, n_seq, n_legs, n_frames, legs, d_cang, d_cfk, d_cst, d_cnf,
                                                  d_init, nullptr, affine, opt ? &dev_opt : nullptr, stream)
                     : seqik_solve_seq_device(d_cpose, n_seq, n_legs, n_frames, legs, 1, 4, d_cang, d_cfk, d_cst, d_cnf,
                                              d_init, nullptr, affine, opt ? &dev_opt : nullptr, stream);
    if (rc == SEQIK_OK)
        rc = seqik_gaps_expand_device(d_map, n_seq, n_legs, n_frames, flags, d_cang, d_cfk, d_cst, d_cnf, d_ang, d_fk, d_st,
                                      d_nf, stream);
    rc = call.finish(rc);
    return rc ? rc : seqik_check_faults_stream(stream);
}

}  // namespace

extern "C" {

int seqik_solve_seq_gaps(const double *pose, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                         const SeqikLegParams *legs, int32_t first_stage, int32_t last_stage, double *angles,
                         double *fk, int32_t *status, int32_t *nfev, const double *init_angles,
                         const SeqikAffine *affine, const SeqikOptions *opt, int32_t *n_valid)
{
    return solve_gaps(false, pose, n_seq, n_legs, n_frames, legs, first_stage, last_stage, angles, fk, status, nfev,
                      init_angles, affine, opt, n_valid);
}

int seqik_solve_generic_gaps(const double *pose, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                             const SeqikLegParams *legs, double *angles, double *fk, int32_t *status, int32_t *nfev,
                             const double *init_angles, const SeqikAffine *affine, const SeqikOptions *opt,
                             int32_t *n_valid)
{
    return solve_gaps(true, pose, n_seq, n_legs, n_frames, legs, 1, 4, angles, fk, status, nfev, init_angles, affine,
                      opt, n_valid);
}

}  // extern "C"
