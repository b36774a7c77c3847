// seqik_refine_sens.hip -- error bars of the whole-leg refinement: key-point sensitivity of the refined angles, their
// standard deviations, the gradient measure and the held / not-a-minimum flags: kernel and C ABI entry points
// (include/seqik_refine_sensitivity.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "seqik_refine_sens.hpp"
#include "seqik_leg_map.hpp"
#include "../../include/seqik_refine_sensitivity.h"

namespace {

using seqik::bad_arg;
using seqik::kSensQuad;  // 21 doubles: the quarter of a record one lane of the staged path holds
using seqik::kSensRow;   // 84
using seqik::kSensStd;   // 7

struct RefSensArgs {
    const double *angles;     // [n_total][7]
    const double *pose;       // [n_total][5][3]
    const double *kp_weight;  // nullable, [n_total][4]
    const double *kp_sigma;   // nullable, [n_total][4]; given exactly when std is
    double *sens;             // nullable, [n_total][7][4][3]
    double *std_out;          // nullable, [n_total][7]
    double *grad;             // nullable, [n_total]
    int32_t *flags;           // nullable, [n_total]
    double tol;
    seqik::LegFrameIndex ix;
    seqik::LegBoundsTable bounds;
};

constexpr int kRefSensWaveLds = 64 * kSensQuad;  // doubles of LDS per wavefront (STAGED): 16 records = 10 752 B

// The rule of leg-frame i: the record into `sink` when RECORD, std / grad / flags of the request when RED.
template <bool RECORD, bool RED, class Sink>
__device__ __forceinline__ void refsens_of(const RefSensArgs &a, int64_t i, Sink &sink)
{
    const int leg = a.ix.leg_of(i);
    seqik::refsens_rule<RECORD>(a.ix.legs[leg], a.bounds.b[leg], a.angles + i * 7, a.pose + i * 15,
                                a.kp_weight ? a.kp_weight + i * 4 : nullptr, a.kp_sigma ? a.kp_sigma + i * 4 : nullptr,
                                a.tol, sink, RED && a.std_out ? a.std_out + i * kSensStd : nullptr,
                                RED && a.grad ? a.grad + i : nullptr, RED && a.flags ? a.flags + i : nullptr);
}

// One leg-frame per lane, grid-stride over the flat index (64-bit throughout), FP64.  Per leg-frame 56 + 120 (+ 32 + 32) B
// in and up to 672 + 56 + 8 + 4 B out.  SENS: the record is wanted; RED: std, grad and / or flags are (which: the pointers).
// Without SENS no record is formed, and without SENS and std the twelve solves are not made.
//   per lane (STAGED false): one pass over the rule feeds the record's stores and the reduction; a store instruction of a
//     wavefront touches 64 records 672 B apart.
//     This is the default: the rule's arithmetic, not the store, is what the unit takes its time for.
//   STAGED (SENS only; SEQIK_REFSENS_STAGED=1): std, grad and flags of the lane's own leg-frame first, then the
//     wavefront's 64 records -- one contiguous run of 43 008 B -- in four passes of 16 (staged_quad_passes of
//     seqik_leg_map.hpp, the scheme of seqik_sensitivity.hip: four lanes share a record, each runs the rule and keeps its
//     quarter, 21 values chosen by compile-time selects).  Whole wavefronts only; the tail of the range takes the per-lane
//     path.  No LDS beyond that, no atomics.
template <bool SENS, bool RED, bool STAGED>
__global__ void __launch_bounds__(256) seqik_refine_sens_kernel(RefSensArgs a)
{
    extern __shared__ double s_refsens[];  // STAGED: kRefSensWaveLds doubles per wavefront
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, n = a.ix.n_total;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t t0 = (int64_t)blockIdx.x * blockDim.x; t0 < n; t0 += stride) {
        const int64_t i = t0 + threadIdx.x;
        const int64_t w0 = t0 + wave * 64;  // first leg-frame of this wavefront
        if (SENS && STAGED && w0 + 64 <= n) {
            if constexpr (RED) {  // i < w0 + 64 <= n
                seqik::NoSink none;
                refsens_of<false, true>(a, i, none);
            }
            seqik::staged_quad_passes<kSensQuad>(  // a pass: 16 records = 21 rows
                s_refsens + wave * kRefSensWaveLds, lane, w0, a.sens, [&](int64_t rec, seqik::QuadSink<kSensQuad> &quad) {
                    seqik::QuadAnySink<kSensQuad> sink{quad};
                    sink.clear();
                    refsens_of<true, false>(a, rec, sink);
                });
        } else if (i < n) {
            if constexpr (SENS) {
                seqik::ArraySink sink{a.sens + i * kSensRow};
                refsens_of<true, RED>(a, i, sink);
            } else {
                seqik::NoSink none;
                refsens_of<false, RED>(a, i, none);
            }
        }
    }
}

constexpr const char *kWho = "seqik_refine_sensitivity";  // both entry points report under this name

// The checks both entry points make before anything touches HIP; *n_total receives n_seq * n_legs * n_frames.
int refsens_validate(const double *angles, const double *pose, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                     const SeqikLegParams *legs, int32_t kind, const double *kp_sigma, double bound_tol, const double *sens,
                     const double *std_out, const double *grad, const int32_t *flags, int64_t *n_total)
{
    if (int rc = seqik::check_leg_map(kWho, n_seq, n_legs, n_frames, legs, kind, kSensRow, n_total)) return rc;
    if (kind != SEQIK_FK_KIND_SEQ)
        return bad_arg(kWho, "kind 1 (generic chain) has no sensitivity: seven angles fitted to three coordinates are not a "
                             "function of the key points");
    if (!angles) return bad_arg(kWho, "angles must not be null");
    if (!pose) return bad_arg(kWho, "pose must not be null");
    if (!sens && !std_out && !grad && !flags) return bad_arg(kWho, "no output requested: give sens, std, grad or flags");
    if (std_out && !kp_sigma) return bad_arg(kWho, "std needs kp_sigma");
    if (!(bound_tol >= 0.0) || !isfinite(bound_tol)) return bad_arg(kWho, "bound_tol must be finite and not negative");
    return SEQIK_OK;
}

// The kernel of a request: without a record (SENS false) there is only the reduction, and nothing to stage.
auto refsens_kernel(bool sens, bool red, bool staged) -> void (*)(RefSensArgs)
{
    if (!sens) return seqik_refine_sens_kernel<false, true, false>;
    if (staged) return red ? seqik_refine_sens_kernel<true, true, true> : seqik_refine_sens_kernel<true, false, true>;
    return red ? seqik_refine_sens_kernel<true, true, false> : seqik_refine_sens_kernel<true, false, false>;
}

}  // namespace

extern "C" {

int seqik_refine_sensitivity_device(const double *d_angles, const double *d_pose, int64_t n_seq, int32_t n_legs,
                                    int64_t n_frames, const SeqikLegParams *legs, int32_t kind, const double *d_kp_weight,
                                    const double *d_kp_sigma, double bound_tol, double *d_sens, double *d_std,
                                    double *d_grad, int32_t *d_flags, void *hip_stream)
{
    int64_t n = 0;
    int rc = refsens_validate(d_angles, d_pose, n_seq, n_legs, n_frames, legs, kind, d_kp_sigma, bound_tol, d_sens, d_std,
                              d_grad, d_flags, &n);
    if (rc != SEQIK_OK) return rc;
    if (n == 0) return SEQIK_OK;
    RefSensArgs a;
    a.angles = d_angles; a.pose = d_pose; a.kp_weight = d_kp_weight;
    a.kp_sigma = d_std ? d_kp_sigma : nullptr;  // the sigmas are read for std only
    a.sens = d_sens; a.std_out = d_std; a.grad = d_grad; a.flags = d_flags;
    a.tol = bound_tol;
    a.ix.fill(n, n_legs, n_frames, legs);
    a.bounds.fill(n_legs, legs);
    // Staged only when a record is requested (staging concerns the record) and SEQIK_REFSENS_STAGED=1 asks for it: unlike
    // the other leg maps this unit is bound by its FP64 arithmetic, not by its store (at 1 M leg-frames the
    // record per lane takes 0.66 ms, the staged path, which runs the rule four times per record, 1.14 ms, a copy of the
    // same bytes 0.16 ms), so the per-lane kernel is the default.
    const bool sens = d_sens != nullptr, red = d_std || d_grad || d_flags;
    const bool staged_asked = seqik::leg_map_switch("SEQIK_REFSENS", "_STAGED", 0) != 0;
    const seqik::LegMapPlan p = seqik::plan_leg_map("SEQIK_REFSENS", n, sens && staged_asked, 256, 256, kRefSensWaveLds);
    return seqik::launch_leg_map(refsens_kernel(sens, red, p.staged), p, a, hip_stream);
}

int seqik_refine_sensitivity(const double *angles, const double *pose, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                             const SeqikLegParams *legs, int32_t kind, const double *kp_weight, const double *kp_sigma,
                             double bound_tol, double *sens, double *std, double *grad, int32_t *flags, int32_t device)
{
    int64_t n = 0;
    int rc = refsens_validate(angles, pose, n_seq, n_legs, n_frames, legs, kind, kp_sigma, bound_tol, sens, std, grad, flags,
                              &n);
    if (rc != SEQIK_OK) return rc;
    if (n == 0) return SEQIK_OK;
    seqik::HostCall call;
    double *d_ang, *d_pose, *d_weight, *d_sigma, *d_sens, *d_std, *d_grad;
    int32_t *d_flags;
    call.upload(d_ang, 7 * (size_t)n, angles);
    call.upload(d_pose, 15 * (size_t)n, pose);
    call.upload(d_weight, 4 * (size_t)n, kp_weight);
    call.upload(d_sigma, 4 * (size_t)n, std ? kp_sigma : nullptr);  // the sigmas are read for std only
    call.download(d_sens, kSensRow * (size_t)n, sens);
    call.download(d_std, kSensStd * (size_t)n, std);
    call.download(d_grad, (size_t)n, grad);
    call.download(d_flags, (size_t)n, flags);
    if ((rc = call.begin(device)) != SEQIK_OK) return rc;
    return call.finish(seqik_refine_sensitivity_device(d_ang, d_pose, n_seq, n_legs, n_frames, legs, kind, d_weight, d_sigma,
                                                       bound_tol, d_sens, d_std, d_grad, d_flags, call.stream()));
}

}  // extern "C"
