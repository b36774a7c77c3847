// seqik_sensitivity.hip -- key-point sensitivity of the sequential leg fit, angle standard deviations and the held-joint
// flags: kernel and C ABI entry points (include/seqik_sensitivity.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "seqik_sensitivity.hpp"
#include "seqik_leg_map.hpp"
#include "../../include/seqik_sensitivity.h"

namespace {

using seqik::bad_arg;
using seqik::kSensQuad;  // 21 doubles: the quarter of a record one lane of the staged path holds
using seqik::kSensRow;   // 84
using seqik::kSensStd;   // 7

struct SensArgs {
    const double *angles;    // [n_total][7]
    const double *pose;      // [n_total][5][3]
    const double *kp_sigma;  // nullable, [n_total][4]; given exactly when std is
    double *sens;            // nullable, [n_total][7][4][3]
    double *std_out;         // nullable, [n_total][7]
    int32_t *flags;          // nullable, [n_total]
    double tol;
    seqik::LegFrameIndex ix;
    seqik::LegBoundsTable bounds;
};

constexpr int kSensWaveLds = 64 * kSensQuad;  // doubles of LDS per wavefront (STAGED): 16 records = 10 752 B

// The rule of leg-frame i into `res`.
__device__ __forceinline__ void sens_of(const SensArgs &a, int64_t i, seqik::SensResult &res)
{
    const int leg = a.ix.leg_of(i);
    seqik::sens_leg_frame_rule(a.ix.legs[leg], a.bounds.b[leg], a.angles + i * 7, a.pose + i * 15,
                               a.std_out ? a.kp_sigma + i * 4 : nullptr, a.tol, res);
}

// std and flags of leg-frame i, whichever are wanted
__device__ __forceinline__ void sens_reduce(const SensArgs &a, int64_t i, const seqik::SensResult &res)
{
    if (a.std_out) seqik::sens_std(res, a.kp_sigma + i * 4, a.std_out + i * kSensStd);
    if (a.flags) a.flags[i] = res.flags;
}

// One leg-frame per lane, grid-stride over the flat index (64-bit throughout), FP64.  Per leg-frame 56 + 120 (+ 32) B in
// and up to 672 + 56 + 4 B out.  SENS: the record is wanted; RED: std and / or flags are (which of the two: the
// pointers).  Without SENS no record is formed: std and the flags come from the 48 computed entries the stages hand on.
//   per lane (STAGED false): one pass over the rule feeds the record's stores and the reduction; a store instruction of a
//     wavefront touches 64 records 672 B apart.
//   STAGED (SENS only): std and flags of the lane's own leg-frame first, then the wavefront's 64 records -- one contiguous
//     run of 43 008 B -- in four passes of 16 (the scheme of seqik_jacobian.hip: four lanes share a record, each runs the
//     rule and keeps its quarter, 21 values chosen by compile-time selects, writes it to LDS at lane * 21, and the
//     wavefront stores the pass as 21 coalesced, non-temporal rows of 512 B).  Whole wavefronts only; the tail of the
//     range takes the per-lane path.  No LDS beyond that, no atomics.
template <bool SENS, bool RED, bool STAGED>
__global__ void __launch_bounds__(256) seqik_sensitivity_kernel(SensArgs a)
{
    extern __shared__ double s_sens[];  // STAGED: kSensWaveLds doubles per wavefront
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, n = a.ix.n_total;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t t0 = (int64_t)blockIdx.x * blockDim.x; t0 < n; t0 += stride) {
        const int64_t i = t0 + threadIdx.x;
        const int64_t w0 = t0 + wave * 64;  // first leg-frame of this wavefront
        if (SENS && STAGED && w0 + 64 <= n) {
            if constexpr (RED) {  // i < w0 + 64 <= n
                seqik::SensResult res;
                sens_of(a, i, res);
                sens_reduce(a, i, res);
            }
            seqik::staged_quad_passes<kSensQuad>(  // a pass: 16 records = 21 rows
                s_sens + wave * kSensWaveLds, lane, w0, a.sens, [&](int64_t rec, seqik::QuadSink<kSensQuad> &sink) {
                    seqik::SensResult res;
                    sens_of(a, rec, res);
                    seqik::sens_emit(sink, res);
                });
        } else if (i < n) {
            seqik::SensResult res;
            sens_of(a, i, res);
            if constexpr (SENS) {
                seqik::ArraySink sink{a.sens + i * kSensRow};
                seqik::sens_emit(sink, res);
            }
            if constexpr (RED) sens_reduce(a, i, res);
        }
    }
}

constexpr const char *kWho = "seqik_fit_sensitivity";  // both entry points report under this name

// The checks both entry points make before anything touches HIP; *n_total receives n_seq * n_legs * n_frames.
int sens_validate(const double *angles, const double *pose, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                  const SeqikLegParams *legs, int32_t kind, const double *kp_sigma, const double *sens, const double *std_out,
                  const int32_t *flags, int64_t *n_total)
{
    if (int rc = seqik::check_leg_map(kWho, n_seq, n_legs, n_frames, legs, kind, kSensRow, n_total)) return rc;
    if (kind != SEQIK_FK_KIND_SEQ)
        return bad_arg(kWho, "kind 1 (generic chain) has no sensitivity: seven angles fitted to three coordinates are not a "
                             "function of the key points");
    if (!angles) return bad_arg(kWho, "angles must not be null");
    if (!pose) return bad_arg(kWho, "pose must not be null");
    if (!sens && !std_out && !flags) return bad_arg(kWho, "no output requested: give sens, std or flags");
    if (std_out && !kp_sigma) return bad_arg(kWho, "std needs kp_sigma");
    return SEQIK_OK;
}

// The kernel of a request: without a record (SENS false) there is only the reduction, and nothing to stage.
auto sens_kernel(bool sens, bool red, bool staged) -> void (*)(SensArgs)
{
    if (!sens) return seqik_sensitivity_kernel<false, true, false>;
    if (staged) return red ? seqik_sensitivity_kernel<true, true, true> : seqik_sensitivity_kernel<true, false, true>;
    return red ? seqik_sensitivity_kernel<true, true, false> : seqik_sensitivity_kernel<true, false, false>;
}

}  // namespace

extern "C" {

int seqik_fit_sensitivity_device(const double *d_angles, const double *d_pose, int64_t n_seq, int32_t n_legs,
                                 int64_t n_frames, const SeqikLegParams *legs, int32_t kind, const double *d_kp_sigma,
                                 double bound_tol, double *d_sens, double *d_std, int32_t *d_flags, void *hip_stream)
{
    int64_t n = 0;
    int rc = sens_validate(d_angles, d_pose, n_seq, n_legs, n_frames, legs, kind, d_kp_sigma, d_sens, d_std, d_flags, &n);
    if (rc != SEQIK_OK) return rc;
    if (n == 0) return SEQIK_OK;
    SensArgs a;
    a.angles = d_angles; a.pose = d_pose; a.kp_sigma = d_kp_sigma; a.sens = d_sens; a.std_out = d_std; a.flags = d_flags;
    a.tol = bound_tol;
    a.ix.fill(n, n_legs, n_frames, legs);
    a.bounds.fill(n_legs, legs);
    // Staged only when a record is requested (staging concerns the record).
    const bool sens = d_sens != nullptr, red = d_std || d_flags;
    const seqik::LegMapPlan p = seqik::plan_leg_map("SEQIK_SENS", n, sens, 256, 256, kSensWaveLds);
    return seqik::launch_leg_map(sens_kernel(sens, red, p.staged), p, a, hip_stream);
}

int seqik_fit_sensitivity(const double *angles, const double *pose, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                          const SeqikLegParams *legs, int32_t kind, const double *kp_sigma, double bound_tol, double *sens,
                          double *std, int32_t *flags, int32_t device)
{
    int64_t n = 0;
    int rc = sens_validate(angles, pose, n_seq, n_legs, n_frames, legs, kind, kp_sigma, sens, std, flags, &n);
    if (rc != SEQIK_OK) return rc;
    if (n == 0) return SEQIK_OK;
    seqik::HostCall call;
    double *d_ang, *d_pose, *d_sigma, *d_sens, *d_std;
    int32_t *d_flags;
    call.upload(d_ang, 7 * (size_t)n, angles);
    call.upload(d_pose, 15 * (size_t)n, pose);
    call.upload(d_sigma, 4 * (size_t)n, std ? kp_sigma : nullptr);  // the sigmas are read for std only
    call.download(d_sens, kSensRow * (size_t)n, sens);
    call.download(d_std, kSensStd * (size_t)n, std);
    call.download(d_flags, (size_t)n, flags);
    if ((rc = call.begin(device)) != SEQIK_OK) return rc;
    return call.finish(seqik_fit_sensitivity_device(d_ang, d_pose, n_seq, n_legs, n_frames, legs, kind, d_sigma, bound_tol,
                                                    d_sens, d_std, d_flags, call.stream()));
}

}  // extern "C"
