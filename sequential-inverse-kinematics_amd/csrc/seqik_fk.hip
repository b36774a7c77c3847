// seqik_fk.hip -- forward kinematics from joint angles: kernel and C ABI entry points (include/seqik_fk.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "seqik_leg_map.hpp"
#include "../../include/seqik_fk.h"

namespace {

using seqik::bad_arg;
using seqik::kFkRow;  // doubles of FK per leg-frame
using seqik::wave_lds_fence;

struct FkArgs {
    const double *angles;  // [n_total][7]
    const double *pose;    // nullable, [n_total][5][3]
    const double *origin;  // nullable, [n_total][3]
    double *fk;            // [n_total][9][3]
    double *dist;          // nullable, [n_total][4]
    seqik::LegFrameIndex ix;
};

constexpr int kFkWaveLds = 64 * kFkRow;  // doubles of LDS per wavefront (STAGED)

__device__ __forceinline__ const double *fk_origin(const FkArgs &a, int64_t i)
{
    return a.pose ? a.pose + i * 15 : (a.origin ? a.origin + i * 3 : nullptr);
}

__device__ __forceinline__ void fk_store_dist(const FkArgs &a, int64_t i, const double *row)
{
    if (a.dist) {
        double d[4];
        seqik::fk_fit_distances(row, a.pose + i * 15, d);
#pragma unroll
        for (int k = 0; k < 4; ++k) a.dist[i * 4 + k] = d[k];
    }
}

// One leg-frame per lane, grid-stride over the flat index (64-bit throughout).  Per leg-frame 56 B of angles in and
// 216 B of FK out (+ 24 B origin / 120 B pose in, 32 B distances out): a map bound by memory, not by its few hundred FP64
// operations.
//   per lane (STAGED false): each lane loads its 7 angles and stores its 27 values itself; one store instruction of a
//     wavefront then touches 64 records 216 B apart.
//   STAGED: a wavefront's 64 consecutive leg-frames are one contiguous block per array; the angles come in as 7 fully
//     coalesced loads into LDS, the lanes pick their 7 from there, write their 27 values back into the same LDS and the
//     wavefront stores the block as 27 fully coalesced lines (non-temporal: written once).  Whole wavefronts only; the
//     tail of the range takes the per-lane path.
template <int KIND, bool STAGED>
__global__ void __launch_bounds__(1024) seqik_fk_kernel(FkArgs a)
{
    extern __shared__ double s_fk[];  // STAGED: kFkWaveLds doubles per wavefront
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, n = a.ix.n_total;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t t0 = (int64_t)blockIdx.x * blockDim.x; t0 < n; t0 += stride) {
        const int64_t i = t0 + threadIdx.x;
        const int64_t w0 = t0 + wave * 64;  // first leg-frame of this wavefront
        if (STAGED && w0 + 64 <= n) {
            double *st = s_fk + wave * kFkWaveLds;
            const double *ga = a.angles + w0 * 7;
#pragma unroll
            for (int k = 0; k < 7; ++k) st[k * 64 + lane] = __builtin_nontemporal_load(ga + k * 64 + lane);
            wave_lds_fence();
            double x[7];
#pragma unroll
            for (int d = 0; d < 7; ++d) x[d] = st[lane * 7 + d];
            wave_lds_fence();  // every lane has its angles before any lane overwrites them with FK rows
            const int leg = a.ix.leg_of(i);
            double *row = st + lane * kFkRow;
            seqik::fk_leg_frame<KIND>(a.ix.legs[leg], x, fk_origin(a, i), row);
            fk_store_dist(a, i, row);
            wave_lds_fence();
            double *gf = a.fk + w0 * kFkRow;
#pragma unroll
            for (int k = 0; k < kFkRow; ++k) __builtin_nontemporal_store(st[k * 64 + lane], gf + k * 64 + lane);
            wave_lds_fence();  // the next iteration's LDS writes stay behind these reads
        } else if (i < n) {
            const int leg = a.ix.leg_of(i);
            double row[kFkRow];
            seqik::fk_leg_frame<KIND>(a.ix.legs[leg], a.angles + i * 7, fk_origin(a, i), row);
            fk_store_dist(a, i, row);
            double *gf = a.fk + i * kFkRow;
#pragma unroll
            for (int k = 0; k < kFkRow; ++k) gf[k] = row[k];
        }
    }
}

constexpr const char *kWho = "seqik_forward_kinematics";  // both entry points report under this name

// The checks both entry points make before anything touches HIP; *n_total receives n_seq * n_legs * n_frames.
int fk_validate(const double *angles, int64_t n_seq, int32_t n_legs, int64_t n_frames, const SeqikLegParams *legs,
                int32_t kind, const double *pose, const double *origin, const double *fk, const double *dist,
                int64_t *n_total)
{
    if (int rc = seqik::check_leg_map(kWho, n_seq, n_legs, n_frames, legs, kind, kFkRow, n_total)) return rc;
    if (!angles || !fk) return bad_arg(kWho, "angles and fk must not be null");
    if (pose && origin) return bad_arg(kWho, "pass pose or origin, not both");
    if (dist && !pose) return bad_arg(kWho, "dist needs pose (the key points to measure against)");
    return SEQIK_OK;
}

}  // namespace

extern "C" {

int seqik_forward_kinematics_device(const double *d_angles, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                                    const SeqikLegParams *legs, int32_t kind, const double *d_pose,
                                    const double *d_origin, double *d_fk, double *d_dist, void *hip_stream)
{
    int64_t n = 0;
    int rc = fk_validate(d_angles, n_seq, n_legs, n_frames, legs, kind, d_pose, d_origin, d_fk, d_dist, &n);
    if (rc != SEQIK_OK) return rc;
    if (n == 0) return SEQIK_OK;
    FkArgs a;
    a.angles = d_angles; a.pose = d_pose; a.origin = d_origin; a.fk = d_fk; a.dist = d_dist;
    a.ix.fill(n, n_legs, n_frames, legs);
    // LDS-staged by default: 6 M leg-frames in 0.296 ms = 1.00 x a copy of the same traffic, the per-lane kernel 0.508 ms =
    // 0.58 x (profiles/fk_bench_r07.json, EXPERIMENTS.md 7.1).  Per lane up to 1024 threads per workgroup; staged at most
    // 256: 13.5 KiB of LDS per wavefront, 54 KiB per workgroup.
    const seqik::LegMapPlan p = seqik::plan_leg_map("SEQIK_FK", n, true, 1024, 256, kFkWaveLds);
    auto *kernel = kind == SEQIK_FK_KIND_SEQ ? (p.staged ? seqik_fk_kernel<0, true> : seqik_fk_kernel<0, false>)
                                             : (p.staged ? seqik_fk_kernel<1, true> : seqik_fk_kernel<1, false>);
    return seqik::launch_leg_map(kernel, p, a, hip_stream);
}

int seqik_forward_kinematics(const double *angles, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                             const SeqikLegParams *legs, int32_t kind, const double *pose, const double *origin,
                             double *fk, double *dist, int32_t device)
{
    int64_t n = 0;
    int rc = fk_validate(angles, n_seq, n_legs, n_frames, legs, kind, pose, origin, fk, dist, &n);
    if (rc != SEQIK_OK) return rc;
    if (n == 0) return SEQIK_OK;
    seqik::HostCall call;
    double *d_ang, *d_pose, *d_org, *d_fk, *d_dist;
    call.upload(d_ang, 7 * (size_t)n, angles);
    call.upload(d_pose, 15 * (size_t)n, pose);
    call.upload(d_org, 3 * (size_t)n, origin);
    call.download(d_fk, kFkRow * (size_t)n, fk);
    call.download(d_dist, 4 * (size_t)n, dist);
    if ((rc = call.begin(device)) != SEQIK_OK) return rc;
    return call.finish(seqik_forward_kinematics_device(d_ang, n_seq, n_legs, n_frames, legs, kind, d_pose, d_org, d_fk, d_dist,
                                                       call.stream()));
}

}  // extern "C"
