// seqik_jacobian.hip -- leg Jacobians, stage conditioning and key-point velocities from joint angles: kernel and C ABI
// entry points (include/seqik_jacobian.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "seqik_jacobian.hpp"
#include "seqik_runtime.hpp"
#include "../../include/seqik_jacobian.h"

namespace {

using seqik::bad_arg;
using seqik::kJacQuad;   // 21 doubles: the quarter of a record one lane of the staged path holds
using seqik::kJacRow;    // 84
using seqik::kJacSigma;  // 8
using seqik::kJacVel;    // 12
using seqik::wave_lds_fence;

struct JacArgs {
    const double *angles;  // [n_total][7]
    const double *qdot;    // nullable, [n_total][7]
    double *jac;           // nullable, [n_total][4][3][7]
    double *sigma;         // nullable, [n_total][8]
    double *vel;           // nullable, [n_total][4][3]
    int64_t n_frames;      // leg-frame i belongs to leg (i / n_frames) % n_legs
    int64_t n_total;       // n_seq * n_legs * n_frames
    int32_t n_legs;
    int32_t pad_;
    seqik::FkLeg legs[seqik::kFkMaxLegs];
};

constexpr int kSubTile = 16;                  // leg-frames per pass of the staged path
constexpr int kJacWaveLds = 64 * kJacQuad;    // doubles of LDS per wavefront (STAGED): 16 records = 10 752 B

struct GlobalSink {
    double *out;
    template <int IDX> __device__ __forceinline__ void put(double v) { out[IDX] = v; }
};

// One leg-frame per lane, grid-stride over the flat index (64-bit throughout).  Per leg-frame 56 B of angles (+ 56 B of
// rates) in and up to 672 + 64 + 96 B out.  JAC: the record is wanted; RED: sigma and / or vel are (which of the two: the
// pointers).  Without JAC no record is formed anywhere: the reduction takes its 21 entries and 12 sums from the walk.
//   per lane (STAGED false): one walk feeds the record's stores and the reduction; a store instruction of a wavefront
//     touches 64 records 672 B apart.
//   STAGED (JAC only): sigma and vel of the lane's own leg-frame first (one walk, per-lane stores of 64 and 96 B), then the
//     wavefront's 64 records -- one contiguous run of 43 008 B -- in four passes of 16 (10 752 B = 84 whole 128-B lines):
//     four lanes share a record, each walks the chain and keeps its quarter, 21 values chosen by compile-time selects,
//     writes it to LDS at lane * 21 (8-byte stores 42 dwords apart: 16 consecutive lanes fall on 16 distinct bank pairs),
//     and the wavefront stores the pass as 21 coalesced, non-temporal rows of 512 B.  Whole wavefronts only; the tail
//     of the range takes the per-lane path.
template <int KIND, bool JAC, bool RED, bool STAGED>
__global__ void __launch_bounds__(256) seqik_jacobian_kernel(JacArgs a)
{
    extern __shared__ double s_jac[];  // STAGED: kJacWaveLds doubles per wavefront
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, n = a.n_total;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t t0 = (int64_t)blockIdx.x * blockDim.x; t0 < n; t0 += stride) {
        const int64_t i = t0 + threadIdx.x;
        const int64_t w0 = t0 + wave * 64;  // first leg-frame of this wavefront
        if (JAC && STAGED && w0 + 64 <= n) {
            if constexpr (RED) {  // i < w0 + 64 <= n
                const int leg = (int)((i / a.n_frames) % a.n_legs);
                seqik::JacBothSink<KIND, false, true, GlobalSink> sink;
                sink.red.begin(a.vel ? a.qdot + i * 7 : nullptr);
                const bool finite = seqik::leg_jacobian_walk<KIND>(a.legs[leg], a.angles + i * 7, sink);
                sink.red.finish(finite, a.sigma ? a.sigma + i * kJacSigma : nullptr, a.vel ? a.vel + i * kJacVel : nullptr);
            }
            double *st = s_jac + wave * kJacWaveLds;
#pragma unroll 1
            for (int p = 0; p < 64 / kSubTile; ++p) {
                const int64_t r0 = w0 + p * kSubTile, rec = r0 + (lane >> 2);  // rec < w0 + 64 <= n
                const int leg = (int)((rec / a.n_frames) % a.n_legs);
                seqik::JacQuadSink sink;
                sink.q = lane & 3;
                seqik::leg_jacobian_walk<KIND>(a.legs[leg], a.angles + rec * 7, sink);
#pragma unroll
                for (int j = 0; j < kJacQuad; ++j) st[lane * kJacQuad + j] = sink.buf[j];  // <= 63 * 21 + 20 < kJacWaveLds
                wave_lds_fence();
                double *gj = a.jac + r0 * kJacRow;  // 16 records = 21 rows of 64 doubles
#pragma unroll
                for (int k = 0; k < kJacQuad; ++k) __builtin_nontemporal_store(st[k * 64 + lane], gj + k * 64 + lane);
                wave_lds_fence();  // the next pass's LDS writes stay behind these reads
            }
        } else if (i < n) {
            const int leg = (int)((i / a.n_frames) % a.n_legs);
            seqik::JacBothSink<KIND, JAC, RED, GlobalSink> sink;
            sink.rec.out = JAC ? a.jac + i * kJacRow : nullptr;
            sink.red.begin(RED && a.vel ? a.qdot + i * 7 : nullptr);
            const bool finite = seqik::leg_jacobian_walk<KIND>(a.legs[leg], a.angles + i * 7, sink);
            if constexpr (RED)
                sink.red.finish(finite, a.sigma ? a.sigma + i * kJacSigma : nullptr, a.vel ? a.vel + i * kJacVel : nullptr);
        }
    }
}

constexpr const char *kWho = "seqik_leg_jacobians";  // both entry points report under this name

// The checks both entry points make before anything touches HIP; *n_total receives n_seq * n_legs * n_frames.
int jac_validate(const double *angles, int64_t n_seq, int32_t n_legs, int64_t n_frames, const SeqikLegParams *legs,
                 int32_t kind, const double *qdot, const double *jac, const double *sigma, const double *vel,
                 int64_t *n_total)
{
    if (n_legs < 1 || n_legs > seqik::kFkMaxLegs) return bad_arg(kWho, "n_legs must lie in 1..8");
    if (n_seq < 0 || n_frames < 0) return bad_arg(kWho, "negative n_seq or n_frames");
    if (!angles) return bad_arg(kWho, "angles must not be null");
    if (!legs) return bad_arg(kWho, "legs must not be null");
    if (!jac && !sigma && !vel) return bad_arg(kWho, "no output requested: give jac, sigma or vel");
    if (vel && !qdot) return bad_arg(kWho, "vel needs qdot");
    if (kind != SEQIK_FK_KIND_SEQ && kind != SEQIK_FK_KIND_GENERIC)
        return bad_arg(kWho, "kind must be 0 (sequential chain) or 1 (generic chain)");
    if (int rc = seqik::check_segments(kWho, legs, n_legs)) return rc;
    if (int rc = seqik::leg_frames_fit(kWho, n_seq, n_legs, n_frames, n_total)) return rc;
    // leg_frames_fit leaves room for 27 doubles per leg-frame; a record here has 84
    if (*n_total > INT64_MAX / (8 * kJacRow)) return bad_arg(kWho, "too many leg-frames");
    return SEQIK_OK;
}

int env_int(const char *name, int absent)
{
    const char *v = getenv(name);
    return v ? atoi(v) : absent;
}

}  // namespace

extern "C" {

int seqik_leg_jacobians_device(const double *d_angles, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                               const SeqikLegParams *legs, int32_t kind, const double *d_qdot, double *d_jac,
                               double *d_sigma, double *d_vel, void *hip_stream)
{
    int64_t n = 0;
    int rc = jac_validate(d_angles, n_seq, n_legs, n_frames, legs, kind, d_qdot, d_jac, d_sigma, d_vel, &n);
    if (rc != SEQIK_OK) return rc;
    if (n == 0) return SEQIK_OK;
    JacArgs a;
    a.angles = d_angles; a.qdot = d_qdot; a.jac = d_jac; a.sigma = d_sigma; a.vel = d_vel;
    a.n_frames = n_frames; a.n_total = n; a.n_legs = n_legs; a.pad_ = 0;
    for (int l = 0; l < seqik::kFkMaxLegs; ++l) seqik::make_fk_leg(legs[l < n_legs ? l : 0], a.legs[l]);
    // SEQIK_JAC_STAGED = 0 / 1, SEQIK_JAC_BLOCK (threads per workgroup, 64..256) and SEQIK_JAC_GRID (a cap on the number
    // of workgroups, so that the grid-stride loop can be exercised at small sizes) select variants for measurements and
    // tests; read per call so that one process can run them all.  Default: EXPERIMENTS.md, "Leg Jacobians".
    const bool jac = d_jac != nullptr, red = d_sigma || d_vel;
    const bool staged = jac && env_int("SEQIK_JAC_STAGED", 1) != 0;
    int block = env_int("SEQIK_JAC_BLOCK", 256);
    if (block < 64 || block > 256 || block % 64) block = 256;
    int64_t blocks = (n + block - 1) / block;
    if (blocks > 256 * 64) blocks = 256 * 64;  // grid-stride beyond 64 workgroups per CU (as seqik_frames.hip)
    const int cap = env_int("SEQIK_JAC_GRID", 0);
    if (cap >= 1 && blocks > cap) blocks = cap;
    const size_t lds = staged ? sizeof(double) * kJacWaveLds * (block / 64) : 0;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
#define JAC_LAUNCH(K, J, R, ST) \
    hipLaunchKernelGGL((seqik_jacobian_kernel<K, J, R, ST>), dim3((unsigned)blocks), dim3(block), lds, s, a)
#define JAC_LAUNCH_KIND(K)                                                       \
    do {                                                                         \
        if (!jac) JAC_LAUNCH(K, false, true, false);                             \
        else if (staged) { if (red) JAC_LAUNCH(K, true, true, true); else JAC_LAUNCH(K, true, false, true); }   \
        else { if (red) JAC_LAUNCH(K, true, true, false); else JAC_LAUNCH(K, true, false, false); }             \
    } while (0)
    if (kind == SEQIK_FK_KIND_SEQ) JAC_LAUNCH_KIND(0);
    else JAC_LAUNCH_KIND(1);
#undef JAC_LAUNCH_KIND
#undef JAC_LAUNCH
    return seqik::launched();
}

int seqik_leg_jacobians(const double *angles, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                        const SeqikLegParams *legs, int32_t kind, const double *qdot, double *jac, double *sigma,
                        double *vel, int32_t device)
{
    int64_t n = 0;
    int rc = jac_validate(angles, n_seq, n_legs, n_frames, legs, kind, qdot, jac, sigma, vel, &n);
    if (rc != SEQIK_OK) return rc;
    if (n == 0) return SEQIK_OK;
    seqik::HostCall call;
    double *d_ang, *d_qdot, *d_jac, *d_sigma, *d_vel;
    call.upload(d_ang, 7 * (size_t)n, angles);
    call.upload(d_qdot, 7 * (size_t)n, vel ? qdot : nullptr);  // the rates are read for the velocities only
    call.download(d_jac, kJacRow * (size_t)n, jac);
    call.download(d_sigma, kJacSigma * (size_t)n, sigma);
    call.download(d_vel, kJacVel * (size_t)n, vel);
    if ((rc = call.begin(device)) != SEQIK_OK) return rc;
    return call.finish(seqik_leg_jacobians_device(d_ang, n_seq, n_legs, n_frames, legs, kind, d_qdot, d_jac, d_sigma, d_vel,
                                                  call.stream()));
}

}  // extern "C"
