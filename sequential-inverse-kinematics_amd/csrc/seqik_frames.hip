// seqik_frames.hip -- link frames from joint angles: kernel and C ABI entry points (include/seqik_frames.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "seqik_frames.hpp"
#include "seqik_leg_map.hpp"
#include "../../include/seqik_frames.h"

namespace {

using seqik::bad_arg;
using seqik::kFramesRow;  // doubles of frames per leg-frame

struct FramesArgs {
    const double *angles;  // [n_total][7]
    const double *origin;  // nullable, [n_total][3]
    double *frames;        // [n_total][9][3][4]
    seqik::LegFrameIndex ix;
};

using seqik::kFramesQuad;                          // 27 doubles: the quarter of a record one lane of the staged path holds
constexpr int kFramesWaveLds = 64 * kFramesQuad;   // doubles of LDS per wavefront (STAGED): 16 records = 13.5 KiB

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
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, n = a.ix.n_total;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t t0 = (int64_t)blockIdx.x * blockDim.x; t0 < n; t0 += stride) {
        const int64_t i = t0 + threadIdx.x;
        const int64_t w0 = t0 + wave * 64;  // first leg-frame of this wavefront
        if (STAGED && w0 + 64 <= n) {
            seqik::staged_quad_passes<kFramesQuad>(
                s_frames + wave * kFramesWaveLds, lane, w0, a.frames, [&](int64_t rec, seqik::QuadSink<kFramesQuad> &sink) {
                    const int leg = a.ix.leg_of(rec);
                    seqik::link_frames_walk<KIND>(a.ix.legs[leg], a.angles + rec * 7,
                                                  a.origin ? a.origin + rec * 3 : nullptr, sink);
                });
        } else if (i < n) {
            const int leg = a.ix.leg_of(i);
            seqik::ArraySink sink{a.frames + i * kFramesRow};
            seqik::link_frames_walk<KIND>(a.ix.legs[leg], a.angles + i * 7, a.origin ? a.origin + i * 3 : nullptr, sink);
        }
    }
}

constexpr const char *kWho = "seqik_link_frames";  // both entry points report under this name

// The checks both entry points make before anything touches HIP; *n_total receives n_seq * n_legs * n_frames.
int frames_validate(const double *angles, int64_t n_seq, int32_t n_legs, int64_t n_frames, const SeqikLegParams *legs,
                    int32_t kind, const double *frames, int64_t *n_total)
{
    if (int rc = seqik::check_leg_map(kWho, n_seq, n_legs, n_frames, legs, kind, kFramesRow, n_total)) return rc;
    if (!angles || !frames) return bad_arg(kWho, "angles and frames must not be null");
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
    a.ix.fill(n, n_legs, n_frames, legs);
    // LDS-staged by default (EXPERIMENTS.md); 64..256 threads per workgroup either way.
    const seqik::LegMapPlan p = seqik::plan_leg_map("SEQIK_FRAMES", n, true, 256, 256, kFramesWaveLds);
    auto *kernel = kind == SEQIK_FK_KIND_SEQ ? (p.staged ? seqik_frames_kernel<0, true> : seqik_frames_kernel<0, false>)
                                             : (p.staged ? seqik_frames_kernel<1, true> : seqik_frames_kernel<1, false>);
    return seqik::launch_leg_map(kernel, p, a, hip_stream);
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
