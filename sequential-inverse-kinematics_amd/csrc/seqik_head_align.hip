// seqik_head_align.hip -- antenna alignment on the GPU: kernels and C ABI entry points (include/seqik_head_align.h).
//
// AlignPose.align_head (seqikpy/alignment.py:489-555) is a per-frame affine map whose constants are quantile statistics
// of the whole recording, four of the five series per side restricted to the frames where the antenna-base-to-thorax
// distance is stationary.  On the host that is four passes over the recording and five sorts per side in front of a
// kernel that takes half a millisecond for 16 M frames, plus a second, aligned copy of the key points that is uploaded
// to be read once.  Here:
//   * seqik_head_align_extract_kernel writes the ten series from the RAW key points (rules: seqik_head_align.hpp);
//   * each series is radix-sorted at full length with hipCUB and the requested ranks are returned -- a frame that was
//     not selected holds +inf in the four restricted series, so rank r < n_stat of the full-length sort IS rank r of
//     the subset and no compaction is needed (order statistics do not depend on the order of the subset);
//   * seqik_head_raw_kernel is the head / antenna angle kernel of seqik_head.hip with the map in its prologue.
// Shared with the older units: the handle's open / close, the sort loop and the pick kernel with seqik_align.hip
// (seqik_order_stats.hpp); the host side of the angle launch with seqik_head.hip (seqik_head_launch.hpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "seqik_core.hpp"
#include "seqik_head_align.hpp"
#include "seqik_head_launch.hpp"
#include "seqik_order_stats.hpp"

namespace {

using seqik::bad_arg;
using seqik::kHeadSeries;
using seqik::wave_lds_fence;

typedef double d2 __attribute__((ext_vector_type(2)));

// ---- statistics ------------------------------------------------------------------------------------------------------

constexpr int kTile = 256;  // frames per workgroup pass = threads per workgroup
constexpr int kHalo = 2;    // the test of frame i reads d[i + 1] and d[i + 2]

struct ExtractArgs {
    const double *r_head, *l_head;  // [n][rec / 3][3]
    const double *thorax;           // [n][th_rec / 3][3]
    int64_t n, rec, th_rec, th_last;  // th_last: offset of the last thorax key point within a frame's record
    double threshold;
    double *series;                 // [2][5][n]: side R, L; base x, y, z, d (+inf where not selected), len
    unsigned long long *counters;   // n_stat R, n_stat L, non-finite series values
};

__device__ __forceinline__ double frame_d(const ExtractArgs &a, const double *head, int64_t t)
{
    const double *th = a.thorax + t * a.th_rec;
    return seqik::head_base_to_thorax(head + t * a.rec, th, th + a.th_last);
}

// One frame per lane, a tile of 256 consecutive frames per workgroup pass, grid-stride over the tiles.  A frame's test
// needs d of the two frames behind it: every lane puts its own d into LDS, lanes 0 and 1 add the two frames behind the
// tile (the HALO: their key points are the only ones loaded twice, 2 in 256), and after one barrier each lane reads its
// three distances from LDS.  Recomputing the neighbours per lane instead would load every key point three times.  The
// loads are per-lane records (48 B / 72 B apart: a wavefront's loads cover whole lines, as in the leg extraction kernel
// of seqik_align.hip), the ten stores of a wavefront are each one contiguous 512 B run.
__global__ void __launch_bounds__(kTile) seqik_head_align_extract_kernel(ExtractArgs a)
{
    __shared__ double s_d[2][kTile + kHalo];
    __shared__ unsigned int s_cnt[3];
    const int tid = threadIdx.x;
    if (tid < 3) s_cnt[tid] = 0;  // (ordered in front of the atomics below by the barriers of the loop, or the one behind it)
    const int64_t tiles = (a.n + kTile - 1) / kTile;
    const double inf = __builtin_huge_val();
    unsigned int bad = 0;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // (uniform per workgroup: barriers inside are safe)
        const int64_t t0 = tile * kTile, t = t0 + tid;
        double base[2][3] = {}, d[2] = {}, len[2] = {};
        if (t < a.n) {
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                const double *head = side == 0 ? a.r_head : a.l_head;
                const double *p = head + t * a.rec;
#pragma unroll
                for (int c = 0; c < 3; ++c) base[side][c] = p[c];
                d[side] = frame_d(a, head, t);
                len[side] = seqik::head_antenna_length(p, p + 3);
                s_d[side][tid] = d[side];  // tid <= 255
            }
        }
        if (tid < kHalo) {
            const int64_t h = t0 + kTile + tid;
            if (h < a.n) {
                s_d[0][kTile + tid] = frame_d(a, a.r_head, h);  // kTile + tid <= 257 < kTile + kHalo
                s_d[1][kTile + tid] = frame_d(a, a.l_head, h);
            }
        }
        __syncthreads();
        if (t < a.n) {
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                // t + 2 < n: frames t + 1 and t + 2 exist, so slots tid + 1, tid + 2 (<= 257) were written above
                const bool sel = t + kHalo < a.n &&
                                 seqik::head_is_stationary(s_d[side][tid], s_d[side][tid + 1], s_d[side][tid + 2], a.threshold);
                double *out = a.series + (int64_t)side * kHeadSeries * a.n + t;  // < 10 n doubles: t < n
#pragma unroll
                for (int c = 0; c < 3; ++c) out[c * a.n] = sel ? base[side][c] : inf;
                out[3 * a.n] = sel ? d[side] : inf;
                out[4 * a.n] = len[side];
                bad += !isfinite(base[side][0]) + !isfinite(base[side][1]) + !isfinite(base[side][2]) + !isfinite(d[side]) +
                       !isfinite(len[side]);
                if (sel) atomicAdd(&s_cnt[side], 1u);
            }
        }
        __syncthreads();  // the next tile's distances stay behind these reads
    }
    if (bad) atomicAdd(&s_cnt[2], bad);
    __syncthreads();
    if (tid < 3 && s_cnt[tid]) atomicAdd(&a.counters[tid], (unsigned long long)s_cnt[tid]);
}

// ---- fused map + head / antenna angles -------------------------------------------------------------------------------

struct HeadRawArgs {
    seqik::HeadArgs h;            // r_head / l_head are RAW
    SeqikHeadAffine affine[2];    // R, L
    double *r_aligned, *l_aligned;  // nullable [n][out_rec / 3][3]
    int32_t n_points, out_rec;    // out_rec: 6, or 3 for single-point records
};

// seqik_head_kernel (seqik_head.hip) with the alignment in front: the same grid-stride loop, the same LDS staging of a
// wavefront's 64 records (three coalesced 16-byte-per-lane loads per array), the same non-temporal stores of the seven
// rows.  The sixteen constants of the two maps arrive in the kernel argument block (scalar registers); per frame the map
// costs 12 subtractions, 12 multiplications and 12 additions next to 96 B + 56 B of traffic.  ALIGNED_OUT: the aligned
// records are written too (an instantiation of its own: the plain one keeps neither the pointers nor the stores); in the
// staged path they go back through the wavefront's LDS block -- each lane overwrites the record it alone read -- and
// leave as three coalesced 16-byte-per-lane stores per array.
template <bool STAGED, bool GIVEN_ROLL, bool ALIGNED_OUT>
__global__ void __launch_bounds__(256) seqik_head_raw_kernel(HeadRawArgs k)
{
    __shared__ d2 s_stage[STAGED ? 4 * 384 : 1];  // per wavefront: 2 arrays x 3072 B = 384 x 16 B
    const seqik::HeadArgs &a = k.h;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, n = a.n_frames;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool ant = a.compute_ant != 0;
    const int n_out = ant ? 7 : 3;
    for (int64_t t0 = (int64_t)blockIdx.x * blockDim.x; t0 < n; t0 += stride) {
        const int64_t t = t0 + threadIdx.x;
        const int64_t w0 = t0 + wave * 64;  // first frame of this wavefront
        double out[7], ra[6], la[6];
        if (STAGED && w0 + 64 <= n) {  // (the launcher takes STAGED only for two-point records and aligned pointers)
            d2 *st = s_stage + wave * 384;
            const d2 *gr = reinterpret_cast<const d2 *>(a.r_head + w0 * 6);
            const d2 *gl = reinterpret_cast<const d2 *>(a.l_head + w0 * 6);
            const d2 r0 = __builtin_nontemporal_load(gr + lane), r1 = __builtin_nontemporal_load(gr + 64 + lane),
                     r2 = __builtin_nontemporal_load(gr + 128 + lane);
            const d2 l0 = __builtin_nontemporal_load(gl + lane), l1 = __builtin_nontemporal_load(gl + 64 + lane),
                     l2 = __builtin_nontemporal_load(gl + 128 + lane);
            st[lane] = r0; st[64 + lane] = r1; st[128 + lane] = r2;
            st[192 + lane] = l0; st[256 + lane] = l1; st[320 + lane] = l2;
            wave_lds_fence();
            double *sd = reinterpret_cast<double *>(st);  // 768 doubles: R records at lane * 6, L records at 384 + lane * 6
            seqik::head_angles_raw_compute(sd + lane * 6, sd + 384 + lane * 6, 2, k.affine, a.neck + t * a.neck_stride,
                                           a.rest_head_pitch, a.rest_antenna_pitch, ant, out,
                                           GIVEN_ROLL ? a.roll_in + t : nullptr, ra, la);
            if (ALIGNED_OUT) {
#pragma unroll
                for (int j = 0; j < 6; ++j) { sd[lane * 6 + j] = ra[j]; sd[384 + lane * 6 + j] = la[j]; }  // <= 384 + 63 * 6 + 5 = 767
                wave_lds_fence();
                if (k.r_aligned) {
                    d2 *g = reinterpret_cast<d2 *>(k.r_aligned + w0 * 6);  // 64 records = 192 x 16 B, w0 + 64 <= n
#pragma unroll
                    for (int q = 0; q < 3; ++q) __builtin_nontemporal_store(st[q * 64 + lane], g + q * 64 + lane);
                }
                if (k.l_aligned) {
                    d2 *g = reinterpret_cast<d2 *>(k.l_aligned + w0 * 6);
#pragma unroll
                    for (int q = 0; q < 3; ++q) __builtin_nontemporal_store(st[192 + q * 64 + lane], g + q * 64 + lane);
                }
            }
            wave_lds_fence();  // the next iteration's LDS writes stay behind these reads
#pragma unroll
            for (int j = 0; j < 7; ++j)
                if (j < n_out) __builtin_nontemporal_store(out[j], a.angles + j * n + t);
        } else if (t < n) {
            seqik::head_angles_raw_compute(a.r_head + t * a.rec, a.l_head + t * a.rec, k.n_points, k.affine,
                                           a.neck + t * a.neck_stride, a.rest_head_pitch, a.rest_antenna_pitch, ant, out,
                                           GIVEN_ROLL ? a.roll_in + t : nullptr, ra, la);
            if (ALIGNED_OUT) {
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    if (j < k.out_rec) {
                        if (k.r_aligned) k.r_aligned[t * k.out_rec + j] = ra[j];
                        if (k.l_aligned) k.l_aligned[t * k.out_rec + j] = la[j];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 7; ++j)
                if (j < n_out) a.angles[j * n + t] = out[j];
        }
    }
}

// [aligned records wanted][seqik::HeadVariant: per-lane loads + given roll, staged, per-lane]
const seqik::HeadKernel<HeadRawArgs> kRawKernels[2][3] = {
    {seqik_head_raw_kernel<false, true, false>, seqik_head_raw_kernel<true, false, false>, seqik_head_raw_kernel<false, false, false>},
    {seqik_head_raw_kernel<false, true, true>, seqik_head_raw_kernel<true, false, true>, seqik_head_raw_kernel<false, false, true>}};

constexpr const char *kWhoRaw = "seqik_head_angles_raw";

}  // namespace

struct SeqikHeadAlignStats : seqik::SeriesHandle {  // d_series: [2][5][n] of the last _select, within [10 * capacity]
    int64_t capacity = 0;
    int64_t n = 0;  // frames of the last _select (0: none yet)
    int64_t n_stat[2] = {0, 0};
};

extern "C" {

int seqik_head_align_stats_open(SeqikHeadAlignStats **out, int64_t capacity_frames, const SeqikOptions *opt)
{
    const char *who = "seqik_head_align_stats_open";
    if (!out) return bad_arg(who, "null handle pointer");
    *out = nullptr;
    if (capacity_frames < 3 || capacity_frames > 0x7fffffffLL)
        return bad_arg(who, "capacity_frames must lie in 3 .. 2^31 - 1");
    if (int rc = seqik::open_series(who, opt, 2 * kHeadSeries * (size_t)capacity_frames, out)) return rc;
    (*out)->capacity = capacity_frames;
    return SEQIK_OK;
}

int seqik_head_align_stats_select(SeqikHeadAlignStats *s, const double *r_head, const double *l_head,
                                  const double *thorax, int32_t on_device, int64_t n, int32_t n_points,
                                  int32_t n_thorax_points, double threshold, int64_t *n_stat, int64_t *n_nonfinite)
{
    const char *who = "seqik_head_align_stats_select";
    if (!s || !r_head || !l_head || !thorax || !n_stat || !n_nonfinite) return bad_arg(who, "null pointer");
    if (n < 3) return bad_arg(who, "the stationary-frame test needs at least 3 frames");
    if (n > s->capacity) return bad_arg(who, "more frames than the capacity");
    if (n_points < 2 || n_points > 64) return bad_arg(who, "n_points must lie in 2..64 (antenna base and tip)");
    if (n_thorax_points < 1 || n_thorax_points > 64) return bad_arg(who, "n_thorax_points must lie in 1..64");
    if (threshold != threshold) return bad_arg(who, "the threshold is NaN");
    s->n = 0;
    seqik::HostCall call;
    double *d_r = nullptr, *d_l = nullptr, *d_t = nullptr;
    unsigned long long *d_cnt = nullptr, h_cnt[3] = {0, 0, 0};
    if (!on_device) {
        call.upload(d_r, 3 * (size_t)n_points * (size_t)n, r_head);
        call.upload(d_l, 3 * (size_t)n_points * (size_t)n, l_head);
        call.upload(d_t, 3 * (size_t)n_thorax_points * (size_t)n, thorax);
    }
    call.download(d_cnt, 3, h_cnt).filled(0);
    if (int rc = call.begin(s->device)) return rc;
    ExtractArgs a;
    a.r_head = on_device ? r_head : d_r; a.l_head = on_device ? l_head : d_l; a.thorax = on_device ? thorax : d_t;
    a.n = n; a.rec = 3 * (int64_t)n_points; a.th_rec = 3 * (int64_t)n_thorax_points; a.th_last = a.th_rec - 3;
    a.threshold = threshold; a.series = s->d_series; a.counters = d_cnt;
    int64_t blocks = (n + kTile - 1) / kTile;
    if (blocks > 256 * 16) blocks = 256 * 16;  // grid-stride over the tiles beyond 16 workgroups per CU
    hipLaunchKernelGGL(seqik_head_align_extract_kernel, dim3((unsigned)blocks), dim3(kTile), 0, call.stream(), a);
    if (int rc = call.finish(seqik::launched())) return rc;
    s->n = n;
    for (int i = 0; i < 2; ++i) n_stat[i] = s->n_stat[i] = (int64_t)h_cnt[i];
    *n_nonfinite = (int64_t)h_cnt[2];
    return SEQIK_OK;
}

int seqik_head_align_stats_pick(SeqikHeadAlignStats *s, const int64_t *ranks_stat, const int64_t *ranks_all,
                                int32_t n_ranks, double *out)
{
    const char *who = "seqik_head_align_stats_pick";
    if (!s || !ranks_stat || !ranks_all || !out) return bad_arg(who, "null pointer");
    if (n_ranks <= 0 || n_ranks > 16) return bad_arg(who, "n_ranks must be 1..16");
    if (s->n == 0) return bad_arg(who, "no recording was selected (call seqik_head_align_stats_select first)");
    if (s->n_stat[0] == 0 || s->n_stat[1] == 0) return bad_arg(who, "the threshold selected no frame on one side");
    int64_t h_ranks[3 * 16];  // rows: the stationary set of R, of L, all frames
    for (int r = 0; r < n_ranks; ++r) {
        h_ranks[r] = ranks_stat[r];
        h_ranks[n_ranks + r] = ranks_stat[n_ranks + r];
        h_ranks[2 * n_ranks + r] = ranks_all[r];
    }
    // a side's first four series hold its n_stat selected values in front of +inf; the fifth (len) counts every frame
    auto pick_of = [s](int i) {
        const int side = i / kHeadSeries;
        const bool all = i % kHeadSeries == kHeadSeries - 1;
        return seqik::RankPick{all ? s->n : s->n_stat[side], all ? 2 : side};
    };
    return seqik::order_statistics(s->device, s->d_series, s->n, 2 * kHeadSeries, s->n, h_ranks, 3, n_ranks, pick_of, out);
}

int seqik_head_align_stats_close(SeqikHeadAlignStats *s) { return seqik::close_series(s); }

int seqik_head_angles_raw_device(const double *d_r_head, const double *d_l_head, int64_t n_frames, int32_t n_points,
                                 const double *d_neck, int64_t neck_stride, double rest_head_pitch,
                                 double rest_antenna_pitch, int32_t compute_ant, const double *d_head_roll,
                                 const SeqikHeadAffine *affine, double *d_angles, double *d_r_aligned,
                                 double *d_l_aligned, void *hip_stream)
{
    if (!affine) return bad_arg(kWhoRaw, "null pointer");
    if (int rc = seqik::check_head_args(kWhoRaw, d_r_head, d_l_head, d_neck, d_angles, n_frames, neck_stride, n_points, compute_ant))
        return rc;
    // asynchronous: a fault an earlier launch left in this stream's word is reported now (this kernel raises none)
    if (int rc = seqik_check_faults_stream(hip_stream)) return rc;
    if (n_frames == 0) return SEQIK_OK;
    HeadRawArgs k;
    k.h = seqik::head_args(d_r_head, d_l_head, n_frames, n_points, d_neck, neck_stride, rest_head_pitch, rest_antenna_pitch,
                           compute_ant, d_head_roll, d_angles);
    k.affine[0] = affine[0]; k.affine[1] = affine[1];
    k.r_aligned = d_r_aligned; k.l_aligned = d_l_aligned;
    k.n_points = n_points; k.out_rec = n_points >= 2 ? 6 : 3;
    return seqik::launch_head(kRawKernels[d_r_aligned || d_l_aligned], seqik::plan_head(k.h, d_r_aligned, d_l_aligned), k,
                              hip_stream);
}

int seqik_head_angles_raw(const double *r_head, const double *l_head, int64_t n_frames, int32_t n_points,
                          const double *neck, int64_t neck_stride, double rest_head_pitch, double rest_antenna_pitch,
                          int32_t compute_ant, const double *head_roll, const SeqikHeadAffine *affine, double *angles,
                          double *r_aligned, double *l_aligned, const SeqikOptions *opt)
{
    if (!affine) return bad_arg(kWhoRaw, "null pointer");
    if (int rc = seqik::check_head_args(kWhoRaw, r_head, l_head, neck, angles, n_frames, neck_stride, n_points, compute_ant))
        return rc;
    if (n_frames == 0) return SEQIK_OK;
    const size_t out_doubles = (n_points >= 2 ? 6 : 3) * (size_t)n_frames;
    seqik::HostCall call;
    seqik::HeadBuffers d;
    double *d_ra, *d_la;
    d.declare(call, seqik::head_args(r_head, l_head, n_frames, n_points, neck, neck_stride, rest_head_pitch,
                                     rest_antenna_pitch, compute_ant, head_roll, angles));
    call.download(d_ra, out_doubles, r_aligned);
    call.download(d_la, out_doubles, l_aligned);
    if (int rc = call.begin(opt ? opt->device : -1)) return rc;
    return call.finish(seqik_head_angles_raw_device(d.r_head, d.l_head, n_frames, n_points, d.neck, neck_stride,
                                                    rest_head_pitch, rest_antenna_pitch, compute_ant, d.head_roll, affine,
                                                    d.angles, d_ra, d_la, call.stream()));
}

}  // extern "C"
