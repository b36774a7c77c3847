// seqik_jacobian.hip -- leg Jacobians, stage conditioning and key-point velocities from joint angles: kernel and C ABI
// entry points (include/seqik_jacobian.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "seqik_jacobian.hpp"
#include "seqik_leg_map.hpp"
#include "../../include/seqik_jacobian.h"

namespace {

using seqik::bad_arg;
using seqik::kJacQuad;   // 21 doubles: the quarter of a record one lane of the staged path holds
using seqik::kJacRow;    // 84
using seqik::kJacSigma;  // 8
using seqik::kJacVel;    // 12

struct JacArgs {
    const double *angles;  // [n_total][7]
    const double *qdot;    // nullable, [n_total][7]
    double *jac;           // nullable, [n_total][4][3][7]
    double *sigma;         // nullable, [n_total][8]
    double *vel;           // nullable, [n_total][4][3]
    seqik::LegFrameIndex ix;
};

using seqik::ArraySink;
constexpr int kJacWaveLds = 64 * kJacQuad;    // doubles of LDS per wavefront (STAGED): 16 records = 10 752 B

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
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, n = a.ix.n_total;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t t0 = (int64_t)blockIdx.x * blockDim.x; t0 < n; t0 += stride) {
        const int64_t i = t0 + threadIdx.x;
        const int64_t w0 = t0 + wave * 64;  // first leg-frame of this wavefront
        if (JAC && STAGED && w0 + 64 <= n) {
            if constexpr (RED) {  // i < w0 + 64 <= n
                const int leg = a.ix.leg_of(i);
                seqik::JacBothSink<KIND, false, true, ArraySink> sink;
                sink.red.begin(a.vel ? a.qdot + i * 7 : nullptr);
                const bool finite = seqik::leg_jacobian_walk<KIND>(a.ix.legs[leg], a.angles + i * 7, sink);
                sink.red.finish(finite, a.sigma ? a.sigma + i * kJacSigma : nullptr, a.vel ? a.vel + i * kJacVel : nullptr);
            }
            seqik::staged_quad_passes<kJacQuad>(  // a pass: 16 records = 21 rows
                s_jac + wave * kJacWaveLds, lane, w0, a.jac, [&](int64_t rec, seqik::QuadSink<kJacQuad> &sink) {
                    const int leg = a.ix.leg_of(rec);
                    seqik::leg_jacobian_walk<KIND>(a.ix.legs[leg], a.angles + rec * 7, sink);
                });
        } else if (i < n) {
            const int leg = a.ix.leg_of(i);
            seqik::JacBothSink<KIND, JAC, RED, ArraySink> sink;
            sink.rec.out = JAC ? a.jac + i * kJacRow : nullptr;
            sink.red.begin(RED && a.vel ? a.qdot + i * 7 : nullptr);
            const bool finite = seqik::leg_jacobian_walk<KIND>(a.ix.legs[leg], a.angles + i * 7, sink);
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
    if (int rc = seqik::check_leg_map(kWho, n_seq, n_legs, n_frames, legs, kind, kJacRow, n_total)) return rc;
    if (!angles) return bad_arg(kWho, "angles must not be null");
    if (!jac && !sigma && !vel) return bad_arg(kWho, "no output requested: give jac, sigma or vel");
    if (vel && !qdot) return bad_arg(kWho, "vel needs qdot");
    return SEQIK_OK;
}

// The kernel of a request: without a record (JAC false) there is only the reduction, and nothing to stage.
template <int KIND>
auto jac_kernel(bool jac, bool red, bool staged) -> void (*)(JacArgs)
{
    if (!jac) return seqik_jacobian_kernel<KIND, false, true, false>;
    if (staged) return red ? seqik_jacobian_kernel<KIND, true, true, true> : seqik_jacobian_kernel<KIND, true, false, true>;
    return red ? seqik_jacobian_kernel<KIND, true, true, false> : seqik_jacobian_kernel<KIND, true, false, false>;
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
    a.ix.fill(n, n_legs, n_frames, legs);
    // Staged only when a record is requested (staging concerns the record).  Default: EXPERIMENTS.md, "Leg Jacobians".
    const bool jac = d_jac != nullptr, red = d_sigma || d_vel;
    const seqik::LegMapPlan p = seqik::plan_leg_map("SEQIK_JAC", n, jac, 256, 256, kJacWaveLds);
    auto *kernel = kind == SEQIK_FK_KIND_SEQ ? jac_kernel<0>(jac, red, p.staged) : jac_kernel<1>(jac, red, p.staged);
    return seqik::launch_leg_map(kernel, p, a, hip_stream);
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
