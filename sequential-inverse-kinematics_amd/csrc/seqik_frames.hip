// seqik_frames.hip -- link frames from joint angles: kernel and C ABI entry points (include/seqik_frames.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "seqik_frames.hpp"
#include "seqik_runtime.hpp"
#include "../../include/seqik_frames.h"

namespace {

using seqik::bad_arg;
using seqik::kFramesRow;  // doubles of frames per leg-frame
using seqik::wave_lds_fence;

struct FramesArgs {
    const double *angles;  // [n_total][7]
    const double *origin;  // nullable, [n_total][3]
    double *frames;        // [n_total][9][3][4]
    int64_t n_frames;      // leg-frame i belongs to leg (i / n_frames) % n_legs
    int64_t n_total;       // n_seq * n_legs * n_frames
    int32_t n_legs;
    int32_t pad_;
    seqik::FkLeg legs[seqik::kFkMaxLegs];
};

using seqik::kFramesQuad;                          // 27 doubles: the quarter of a record one lane of the staged path holds
constexpr int kSubTile = 16;                       // leg-frames per pass of the staged path
constexpr int kFramesWaveLds = 64 * kFramesQuad;   // doubles of LDS per wavefront (STAGED): 16 records = 13.5 KiB

// Straight to global memory, value by value (per-lane path).
struct GlobalSink {
    double *out;
    template <int IDX> __device__ __forceinline__ void put(double v) { out[IDX] = v; }
};

// One leg-frame per lane, grid-stride over the flat index (64-bit throughout).  Per leg-frame 56 B of angles (+ 24 B of
// origin) in and 864 B out: a map bound by its stores.
//   per lane (STAGED false): each lane stores its 108 values itself; one store instruction of a wavefront then touches
//     64 records 864 B apart.
//   STAGED: a wavefront's 64 leg-frames are one contiguous run of 55 296 B in the output.  Held in LDS at once that is
//     54 KiB per wavefront -- two or three wavefronts per CU.  Instead the run goes out in four passes of 16 records
//     (13 824 B = 108 whole 128-B lines, the LDS footprint of the FK kernel): in a pass four lanes share a record, each
//     walks the chain (a few hundred FP64 operations, free next to the stores) and keeps its quarter of the record --
//     27 values chosen by selects as the walk produces them, never 108 registers -- and writes it to LDS at lane * 27
//     (8-byte stores 54 dwords apart: 16 consecutive lanes fall on 16 distinct bank pairs); then the wavefront stores
//     the 13 824 B as 27 fully coalesced lines (non-temporal: written once).  Whole wavefronts only; the tail of the
//     range takes the per-lane path.
template <int KIND, bool STAGED>
__global__ void __launch_bounds__(256) seqik_frames_kernel(FramesArgs a)
{
    extern __shared__ double s_frames[];  // STAGED: kFramesWaveLds doubles per wavefront
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, n = a.n_total;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t t0 = (int64_t)blockIdx.x * blockDim.x; t0 < n; t0 += stride) {
        const int64_t i = t0 + threadIdx.x;
        const int64_t w0 = t0 + wave * 64;  // first leg-frame of this wavefront
        if (STAGED && w0 + 64 <= n) {
            double *st = s_frames + wave * kFramesWaveLds;
#pragma unroll 1
            for (int p = 0; p < 64 / kSubTile; ++p) {
                const int64_t r0 = w0 + p * kSubTile, rec = r0 + (lane >> 2);  // rec < w0 + 64 <= n
                const int leg = (int)((rec / a.n_frames) % a.n_legs);
                seqik::FramesQuadSink sink;
                sink.q = lane & 3;
                seqik::link_frames_walk<KIND>(a.legs[leg], a.angles + rec * 7, a.origin ? a.origin + rec * 3 : nullptr,
                                              sink);
#pragma unroll
                for (int j = 0; j < kFramesQuad; ++j) st[lane * kFramesQuad + j] = sink.buf[j];  // <= 63 * 27 + 26 < kFramesWaveLds
                wave_lds_fence();
                double *gf = a.frames + r0 * kFramesRow;
#pragma unroll
                for (int k = 0; k < kFramesQuad; ++k) __builtin_nontemporal_store(st[k * 64 + lane], gf + k * 64 + lane);
                wave_lds_fence();  // the next pass's LDS writes stay behind these reads
            }
        } else if (i < n) {
            const int leg = (int)((i / a.n_frames) % a.n_legs);
            GlobalSink sink{a.frames + i * kFramesRow};
            seqik::link_frames_walk<KIND>(a.legs[leg], a.angles + i * 7, a.origin ? a.origin + i * 3 : nullptr, sink);
        }
    }
}

constexpr const char *kWho = "seqik_link_frames";  // both entry points report under this name

// The checks both entry points make before anything touches HIP; *n_total receives n_seq * n_legs * n_frames.
int frames_validate(const double *angles, int64_t n_seq, int32_t n_legs, int64_t n_frames, const SeqikLegParams *legs,
                    int32_t kind, const double *frames, int64_t *n_total)
{
    if (n_legs < 1 || n_legs > seqik::kFkMaxLegs) return bad_arg(kWho, "n_legs must lie in 1..8");
    if (n_seq < 0 || n_frames < 0) return bad_arg(kWho, "negative n_seq or n_frames");
    if (!angles || !frames) return bad_arg(kWho, "angles and frames must not be null");
    if (!legs) return bad_arg(kWho, "legs must not be null");
    if (kind != SEQIK_FK_KIND_SEQ && kind != SEQIK_FK_KIND_GENERIC)
        return bad_arg(kWho, "kind must be 0 (sequential chain) or 1 (generic chain)");
    if (int rc = seqik::check_segments(kWho, legs, n_legs)) return rc;
    if (int rc = seqik::leg_frames_fit(kWho, n_seq, n_legs, n_frames, n_total)) return rc;
    // leg_frames_fit leaves room for 27 doubles per leg-frame; a record here has 108
    if (*n_total > INT64_MAX / (8 * kFramesRow)) return bad_arg(kWho, "too many leg-frames");
    return SEQIK_OK;
}

}  // namespace

extern "C" {

int seqik_link_frames_device(const double *d_angles, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                             const SeqikLegParams *legs, int32_t kind, const double *d_origin, double *d_frames,
                             void *hip_stream)
{
    int64_t n = 0;
    int rc = frames_validate(d_angles, n_seq, n_legs, n_frames, legs, kind, d_frames, &n);
    if (rc != SEQIK_OK) return rc;
    if (n == 0) return SEQIK_OK;
    FramesArgs a;
    a.angles = d_angles; a.origin = d_origin; a.frames = d_frames;
    a.n_frames = n_frames; a.n_total = n; a.n_legs = n_legs; a.pad_ = 0;
    for (int l = 0; l < seqik::kFkMaxLegs; ++l) seqik::make_fk_leg(legs[l < n_legs ? l : 0], a.legs[l]);
    // LDS-staged by default (EXPERIMENTS.md).  SEQIK_FRAMES_STAGED = 0 / 1 and SEQIK_FRAMES_BLOCK (threads per
    // workgroup, 64..256) select variants for measurements and tests; read per call so that one process can run both.
    const char *env_staged = getenv("SEQIK_FRAMES_STAGED"), *env_block = getenv("SEQIK_FRAMES_BLOCK");
    const bool staged = env_staged ? atoi(env_staged) != 0 : true;
    int block = env_block ? atoi(env_block) : 256;
    if (block < 64 || block > 256 || block % 64) block = 256;
    int64_t blocks = (n + block - 1) / block;
    if (blocks > 256 * 64) blocks = 256 * 64;  // grid-stride beyond 64 workgroups per CU (as seqik_fk.hip)
    const size_t lds = staged ? sizeof(double) * kFramesWaveLds * (block / 64) : 0;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
#define FRAMES_LAUNCH(K, ST) \
    hipLaunchKernelGGL((seqik_frames_kernel<K, ST>), dim3((unsigned)blocks), dim3(block), lds, s, a)
    if (kind == SEQIK_FK_KIND_SEQ) { if (staged) FRAMES_LAUNCH(0, true); else FRAMES_LAUNCH(0, false); }
    else { if (staged) FRAMES_LAUNCH(1, true); else FRAMES_LAUNCH(1, false); }
#undef FRAMES_LAUNCH
    return seqik::launched();
}

int seqik_link_frames(const double *angles, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                      const SeqikLegParams *legs, int32_t kind, const double *origin, double *frames, int32_t device)
{
    int64_t n = 0;
    int rc = frames_validate(angles, n_seq, n_legs, n_frames, legs, kind, frames, &n);
    if (rc != SEQIK_OK) return rc;
    if (n == 0) return SEQIK_OK;
    seqik::HostCall call;
    double *d_ang, *d_org, *d_frames;
    call.upload(d_ang, 7 * (size_t)n, angles);
    call.upload(d_org, 3 * (size_t)n, origin);
    call.download(d_frames, kFramesRow * (size_t)n, frames);
    if ((rc = call.begin(device)) != SEQIK_OK) return rc;
    return call.finish(seqik_link_frames_device(d_ang, n_seq, n_legs, n_frames, legs, kind, d_org, d_frames, call.stream()));
}

}  // extern "C"
