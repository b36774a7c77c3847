// seqik_smooth_sens.hip -- error bars of the smoothed trajectory: the sensitivity of every frame's angles to the key points
// of its own and its neighbouring frames, their standard deviations, the gradient measure and the held / not-a-minimum /
// bad-sigma flags: kernels and C ABI entry points (include/seqik_smooth_sensitivity.h).  The rule and its phases:
// seqik_smooth_sens.hpp.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "seqik_smooth_sens.hpp"
#include "seqik_leg_map.hpp"
#include "../../include/seqik_smooth_sensitivity.h"

namespace {

using seqik::bad_arg;
using seqik::SmoothSensProblem;

enum Phase : int { ASSEMBLE, SCHUR, COMBINE, COV, FINISH };

// One phase of the rule over all its items, grid-stride (64-bit throughout), FP64.  Items of one launch read only what
// earlier launches stored (COMBINE also its own frame's verdict word, which no other item touches) and no two write the
// same word: no atomics, no waiting, the launch boundary is the barrier.  ASSEMBLE, COMBINE and FINISH have one item per
// frame; SCHUR and COV one per (trajectory, direction), serial over the frames of the trajectory -- item i is trajectory
// i >> 1 in direction i & 1, and the direction is a run-time value, so the two sweeps of a trajectory sit in neighbouring
// lanes and execute the same instructions.  A wavefront may hold up to 512 registers per lane (one wave per SIMD): the
// sweeps keep three 7 x 7 blocks in registers and are latency-bound chains, not occupancy-bound maps.
template <int PHASE>
__global__ void __launch_bounds__(256) seqik_smooth_sens_kernel(SmoothSensProblem p, int64_t n)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if constexpr (PHASE == ASSEMBLE) seqik::ssens_assemble(p, i);
        else if constexpr (PHASE == SCHUR) seqik::ssens_schur_sweep(p, i >> 1, (int)(i & 1));
        else if constexpr (PHASE == COMBINE) seqik::ssens_combine(p, i);
        else if constexpr (PHASE == COV) seqik::ssens_cov_sweep(p, i >> 1, (int)(i & 1));
        else seqik::ssens_finish(p, i);
    }
}

constexpr const char *kWho = "seqik_smooth_sensitivity";  // every entry point reports under this name

// doubles of the widest per-leg-frame array of a call: the record, or the workspace
int ssens_row(int32_t half_width)
{
    const int rec = seqik::kSensRow * (2 * half_width + 1), ws = (seqik::kSsensFrameBytes + 7) / 8;
    return rec > ws ? rec : ws;
}

bool ssens_width_ok(int32_t half_width) { return half_width >= 0 && half_width <= SEQIK_SMOOTHSENS_MAX_HALF_WIDTH; }

// The checks both entry points make before anything touches HIP.  Fills the sizes, smooth and the leg tables of *p.
int ssens_validate(const double *angles, const double *pose, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                   const SeqikLegParams *legs, int32_t kind, const double *kp_sigma, const double *smooth, double bound_tol,
                   int32_t half_width, const double *sens, const double *std_out, const double *grad, const int32_t *flags,
                   int64_t *n_total, SmoothSensProblem *p)
{
    if (!ssens_width_ok(half_width)) return bad_arg(kWho, "half_width must lie in 0..32");
    if (int rc = seqik::check_leg_map(kWho, n_seq, n_legs, n_frames, legs, kind, ssens_row(half_width), n_total)) return rc;
    if (kind != SEQIK_FK_KIND_SEQ)
        return bad_arg(kWho, "kind 1 (generic chain) has no sensitivity: the trajectory refinement exists for the sequential "
                             "chain only");
    if (!angles) return bad_arg(kWho, "angles must not be null");
    if (!pose) return bad_arg(kWho, "pose must not be null");
    if (!sens && !std_out && !grad && !flags) return bad_arg(kWho, "no output requested: give sens, std, grad or flags");
    if (std_out && !kp_sigma) return bad_arg(kWho, "std needs kp_sigma");
    if (!(bound_tol >= 0.0) || !isfinite(bound_tol)) return bad_arg(kWho, "bound_tol must be finite and not negative");
    *p = SmoothSensProblem{};
    for (int j = 0; j < 7; ++j) {
        p->sp.opt.smooth[j] = smooth ? smooth[j] : SEQIK_SMOOTH_DEFAULT;
        if (!(p->sp.opt.smooth[j] >= 0.0) || !isfinite(p->sp.opt.smooth[j])) return bad_arg(kWho, "smooth must be finite and not negative");
    }
    p->sp.n_frames = n_frames;
    p->sp.n_traj = n_seq * n_legs;
    p->sp.n_legs = n_legs;
    for (int l = 0; l < seqik::kFkMaxLegs; ++l) {
        seqik::make_fk_leg(legs[l < n_legs ? l : 0], p->sp.legs[l]);
        seqik::make_leg_bounds(legs[l < n_legs ? l : 0], p->sp.bounds[l]);
    }
    p->tol = bound_tol;
    p->half_width = half_width;
    return SEQIK_OK;
}

template <int PHASE>
int launch_phase(const SmoothSensProblem &p, int64_t n, hipStream_t stream)
{
    const seqik::LegMapPlan plan = seqik::plan_leg_map("SEQIK_SMOOTHSENS", n, false, 256, 256, 0);
    hipLaunchKernelGGL(seqik_smooth_sens_kernel<PHASE>, dim3((unsigned)plan.blocks), dim3(plan.block), 0, stream, p, n);
    return seqik::launched();
}

#define SSENS_TRY(expr)                  \
    do {                                 \
        const int rc_ = (expr);          \
        if (rc_ != SEQIK_OK) return rc_; \
    } while (0)

}  // namespace

extern "C" {

int64_t seqik_smooth_sensitivity_workspace_bytes(int64_t n_seq, int32_t n_legs, int64_t n_frames, int32_t half_width)
{
    if (!ssens_width_ok(half_width)) return bad_arg(kWho, "half_width must lie in 0..32"), -1;
    if (n_legs < 1 || n_legs > seqik::kFkMaxLegs) return bad_arg(kWho, "n_legs must lie in 1..8"), -1;
    if (n_seq < 0 || n_frames < 0) return bad_arg(kWho, "negative n_seq or n_frames"), -1;
    int64_t n = 0;
    if (seqik::leg_frames_fit(kWho, n_seq, n_legs, n_frames, &n, ssens_row(half_width)) != SEQIK_OK) return -1;
    if (n == 0) return 0;
    SmoothSensProblem p;
    p.sp.n_frames = n_frames;
    p.sp.n_traj = n_seq * n_legs;
    return (int64_t)seqik::ssens_carve(p, nullptr);
}

int seqik_smooth_sensitivity_device(const double *d_angles, const double *d_pose, int64_t n_seq, int32_t n_legs,
                                    int64_t n_frames, const SeqikLegParams *legs, int32_t kind, const double *d_kp_weight,
                                    const double *d_kp_sigma, const double *smooth, double bound_tol, int32_t half_width,
                                    double *d_sens, double *d_std, double *d_grad, int32_t *d_flags, void *d_workspace,
                                    int64_t workspace_bytes, void *hip_stream)
{
    int64_t n = 0;
    SmoothSensProblem p;
    SSENS_TRY(ssens_validate(d_angles, d_pose, n_seq, n_legs, n_frames, legs, kind, d_kp_sigma, smooth, bound_tol, half_width,
                             d_sens, d_std, d_grad, d_flags, &n, &p));
    if (n > 0 && (!d_workspace || workspace_bytes < seqik_smooth_sensitivity_workspace_bytes(n_seq, n_legs, n_frames, half_width)))
        return bad_arg(kWho, "workspace is null or smaller than seqik_smooth_sensitivity_workspace_bytes() asks for");
    if (n > 0 && ((uintptr_t)d_workspace & 7)) return bad_arg(kWho, "workspace must be 8-byte aligned");
    if (n == 0) return SEQIK_OK;
    p.angles = d_angles; p.pose = d_pose; p.kp_weight = d_kp_weight;
    p.kp_sigma = d_std ? d_kp_sigma : nullptr;  // the sigmas are read for std only
    p.sens = d_sens; p.std_out = d_std; p.grad = d_grad; p.flags = d_flags;
    seqik::ssens_carve(p, static_cast<char *>(d_workspace));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    // the phases of ssens_run_host, one launch each: five at most, fewer for a request that needs fewer
    SSENS_TRY(launch_phase<ASSEMBLE>(p, n, stream));
    if (!seqik::ssens_wants_verdict(p)) return SEQIK_OK;
    SSENS_TRY(launch_phase<SCHUR>(p, 2 * p.sp.n_traj, stream));
    SSENS_TRY(launch_phase<COMBINE>(p, n, stream));
    if (seqik::ssens_wants_cov(p)) SSENS_TRY(launch_phase<COV>(p, 2 * p.sp.n_traj, stream));
    if (seqik::ssens_wants_finish(p)) SSENS_TRY(launch_phase<FINISH>(p, n, stream));
    return SEQIK_OK;
}

int seqik_smooth_sensitivity(const double *angles, const double *pose, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                             const SeqikLegParams *legs, int32_t kind, const double *kp_weight, const double *kp_sigma,
                             const double *smooth, double bound_tol, int32_t half_width, double *sens, double *std,
                             double *grad, int32_t *flags, int32_t device)
{
    int64_t n = 0;
    SmoothSensProblem p;
    SSENS_TRY(ssens_validate(angles, pose, n_seq, n_legs, n_frames, legs, kind, kp_sigma, smooth, bound_tol, half_width, sens,
                             std, grad, flags, &n, &p));
    if (n == 0) return SEQIK_OK;
    const int64_t ws_bytes = seqik_smooth_sensitivity_workspace_bytes(n_seq, n_legs, n_frames, half_width);
    seqik::HostCall call;
    double *d_ang, *d_pose, *d_weight, *d_sigma, *d_sens, *d_std, *d_grad;
    int32_t *d_flags;
    char *d_ws;
    call.upload(d_ang, 7 * (size_t)n, angles);
    call.upload(d_pose, 15 * (size_t)n, pose);
    call.upload(d_weight, 4 * (size_t)n, kp_weight);
    call.upload(d_sigma, 4 * (size_t)n, std ? kp_sigma : nullptr);  // the sigmas are read for std only
    call.download(d_sens, (size_t)seqik::kSensRow * (2 * (size_t)half_width + 1) * (size_t)n, sens);
    call.download(d_std, seqik::kSensStd * (size_t)n, std);
    call.download(d_grad, (size_t)n, grad);
    call.download(d_flags, (size_t)n, flags);
    call.scratch(d_ws, (size_t)ws_bytes);
    int rc = call.begin(device);
    if (rc != SEQIK_OK) return rc;
    return call.finish(seqik_smooth_sensitivity_device(d_ang, d_pose, n_seq, n_legs, n_frames, legs, kind, d_weight, d_sigma,
                                                       smooth, bound_tol, half_width, d_sens, d_std, d_grad, d_flags, d_ws,
                                                       ws_bytes, call.stream()));
}

}  // extern "C"
