// seqik_smooth.hip -- trajectory refinement, a whole-leg fit with smoothness across frames: kernels and C ABI entry
// points (include/seqik_smooth.h).  The rule and its phases: seqik_smooth.hpp.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "seqik_smooth.hpp"
#include "seqik_leg_map.hpp"
#include "../../include/seqik_smooth.h"

namespace {

using seqik::bad_arg;
using seqik::SmoothProblem;

enum Phase : int { INIT, START_COST, ASSEMBLE, STOP, SETUP, NORMALISE, REDUCE, FINAL, TRIAL, FINISH };

// One phase of the rule over all its items, grid-stride (64-bit throughout), FP64.  Items of one launch read only what
// earlier launches stored, and no two write the same word except the flag words (atomic OR) and the counter of running
// trajectories (atomic add): the order of the items is free.  SETUP, NORMALISE and REDUCE have eight items per row, the
// row's eight lanes next to each other, so a wavefront holds eight whole rows and the rows a lane's neighbours read are a
// broadcast; the others have one item per frame, STOP one per trajectory.  Items of a stopped trajectory return at once.
template <int PHASE>
__global__ void __launch_bounds__(256) seqik_smooth_kernel(SmoothProblem p, int64_t n, int64_t h, int cur)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if constexpr (PHASE == INIT) seqik::smooth_init(p, i);
        else if constexpr (PHASE == START_COST) seqik::smooth_start_cost(p, i);
        else if constexpr (PHASE == ASSEMBLE) seqik::smooth_assemble(p, i);
        else if constexpr (PHASE == STOP) seqik::smooth_stop(p, i);
        else if constexpr (PHASE == SETUP) seqik::smooth_setup(p, i >> 3, (int)(i & 7));
        else if constexpr (PHASE == NORMALISE) seqik::smooth_normalise(p, i >> 3, (int)(i & 7), cur);
        else if constexpr (PHASE == REDUCE) seqik::smooth_reduce(p, i >> 3, (int)(i & 7), h, cur);
        else if constexpr (PHASE == FINAL) seqik::smooth_final(p, i, cur);
        else if constexpr (PHASE == TRIAL) seqik::smooth_trial(p, i);
        else seqik::smooth_finish(p, i);
    }
}

// The cost of a trajectory and what follows from it, one workgroup per trajectory (grid-stride): the tree over e, level
// by level with a workgroup barrier between levels, then lane 0 decides (START: it keeps the starting cost) and, where the
// trial was accepted, the workgroup copies qn to q.  Everything a lane reads here that another lane of this launch wrote
// was written by its own workgroup in front of a barrier.
template <bool START>
__global__ void __launch_bounds__(256) seqik_smooth_decide_kernel(SmoothProblem p)
{
    __shared__ int accepted;
    for (int64_t traj = blockIdx.x; traj < p.n_traj; traj += gridDim.x) {
        const bool run = START || p.traj[traj].status == seqik::SMOOTH_TRIAL;
        __syncthreads();  // every lane has read the status before lane 0 changes it
        if (run) {
            for (int64_t m = 1; m < p.n_pad; m *= 2) {
                for (int64_t i = threadIdx.x; i < p.n_pad / (2 * m); i += blockDim.x) seqik::smooth_tree_add(p, traj, m, i);
                __syncthreads();
            }
        }
        if (threadIdx.x == 0) {
            if constexpr (START) {
                seqik::smooth_start(p, traj);
                accepted = 0;
            } else {
                accepted = run && seqik::smooth_decide(p, traj);
            }
        }
        __syncthreads();
        if (accepted) {
            const int64_t i0 = traj * p.n_frames * 7, i1 = i0 + p.n_frames * 7;
            for (int64_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) p.q[i] = p.qn[i];
        }
        __syncthreads();  // `accepted` is read before the next trajectory's lane 0 writes it
    }
}

constexpr const char *kWho = "seqik_smooth_legs";  // both entry points report under this name
constexpr int kBytesPerFrame = 8 * seqik::kSmoothFrameDoubles + 16 + 4;  // + e (n_pad < 2 N doubles per N frames) + held

// The checks every entry point makes before anything touches HIP.  Fills the sizes, the options and the leg tables of *p.
int smooth_validate(int64_t n_seq, int32_t n_legs, int64_t n_frames, const SeqikLegParams *legs, int32_t kind,
                    const SeqikSmoothOptions *opt, int64_t *n_total, SmoothProblem *p)
{
    if (int rc = seqik::check_leg_map(kWho, n_seq, n_legs, n_frames, legs, kind, (kBytesPerFrame + 7) / 8 + 64, n_total)) return rc;
    if (kind != SEQIK_FK_KIND_SEQ)
        return bad_arg(kWho, "kind 1 (generic chain) is not built: the trajectory refinement exists for the sequential chain only");
    for (int j = 0; j < 7; ++j) {
        p->opt.smooth[j] = opt ? opt->smooth[j] : SEQIK_SMOOTH_DEFAULT;
        if (!(p->opt.smooth[j] >= 0.0) || !isfinite(p->opt.smooth[j])) return bad_arg(kWho, "smooth must be finite and not negative");
    }
    p->opt.max_iter = opt ? opt->max_iter : SEQIK_SMOOTH_MAX_ITER;
    p->opt.gtol = opt ? opt->gtol : SEQIK_REFINE_GTOL;
    p->opt.ftol = opt ? opt->ftol : SEQIK_REFINE_FTOL;
    p->opt.pad_ = 0;
    if (p->opt.max_iter < 1 || p->opt.max_iter > 1000) return bad_arg(kWho, "max_iter must lie in 1..1000");
    if (!(p->opt.gtol >= 0.0) || !isfinite(p->opt.gtol)) return bad_arg(kWho, "gtol must be finite and not negative");
    if (!(p->opt.ftol >= 0.0) || !isfinite(p->opt.ftol)) return bad_arg(kWho, "ftol must be finite and not negative");
    p->n_frames = n_frames;
    p->n_traj = n_seq * n_legs;
    p->n_pad = n_frames > 0 ? seqik::smooth_pad(n_frames) : 0;
    p->n_legs = n_legs;
    p->pad_ = 0;
    for (int l = 0; l < seqik::kFkMaxLegs; ++l) {
        seqik::make_fk_leg(legs[l < n_legs ? l : 0], p->legs[l]);
        seqik::make_leg_bounds(legs[l < n_legs ? l : 0], p->bounds[l]);
    }
    return SEQIK_OK;
}

int smooth_check_buffers(const double *angles, const double *pose, const double *angles_out)
{
    if (!angles) return bad_arg(kWho, "angles must not be null");
    if (!pose) return bad_arg(kWho, "pose must not be null");
    if (!angles_out) return bad_arg(kWho, "angles_out must not be null");
    return SEQIK_OK;
}

template <int PHASE>
int launch_phase(const SmoothProblem &p, int64_t n, int64_t h, int cur, hipStream_t stream)
{
    const seqik::LegMapPlan plan = seqik::plan_leg_map("SEQIK_SMOOTH", n, false, 256, 256, 0);
    hipLaunchKernelGGL(seqik_smooth_kernel<PHASE>, dim3((unsigned)plan.blocks), dim3(plan.block), 0, stream, p, n, h, cur);
    return seqik::launched();
}

template <bool START>
int launch_decide(const SmoothProblem &p, hipStream_t stream)
{
    // one workgroup per trajectory: the plan of n_traj workgroups' worth of lanes
    const seqik::LegMapPlan plan = seqik::plan_leg_map("SEQIK_SMOOTH", p.n_traj * 256, false, 256, 256, 0);
    const int64_t blocks = plan.blocks < p.n_traj ? plan.blocks : p.n_traj;
    hipLaunchKernelGGL(seqik_smooth_decide_kernel<START>, dim3((unsigned)blocks), dim3(plan.block), 0, stream, p);
    return seqik::launched();
}

#define SMOOTH_TRY(expr)                 \
    do {                                 \
        const int rc_ = (expr);          \
        if (rc_ != SEQIK_OK) return rc_; \
    } while (0)

}  // namespace

extern "C" {

int64_t seqik_smooth_workspace_bytes(int64_t n_seq, int32_t n_legs, int64_t n_frames)
{
    if (n_legs < 1 || n_legs > seqik::kFkMaxLegs) return bad_arg(kWho, "n_legs must lie in 1..8"), -1;
    if (n_seq < 0 || n_frames < 0) return bad_arg(kWho, "negative n_seq or n_frames"), -1;
    int64_t n = 0;
    if (seqik::leg_frames_fit(kWho, n_seq, n_legs, n_frames, &n, (kBytesPerFrame + 7) / 8 + 64) != SEQIK_OK) return -1;
    if (n == 0) return 0;
    SmoothProblem p;
    p.n_frames = n_frames;
    p.n_traj = n_seq * n_legs;
    p.n_pad = seqik::smooth_pad(n_frames);
    return (int64_t)seqik::smooth_carve(p, nullptr);
}

int seqik_smooth_legs_device(const double *d_angles, const double *d_pose, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                             const SeqikLegParams *legs, int32_t kind, const double *d_kp_weight,
                             const SeqikSmoothOptions *opt, double *d_angles_out, int32_t *d_frame_info, double *d_cost,
                             int32_t *d_info, void *d_workspace, int64_t workspace_bytes, void *hip_stream)
{
    int64_t n = 0;
    SmoothProblem p;
    SMOOTH_TRY(smooth_validate(n_seq, n_legs, n_frames, legs, kind, opt, &n, &p));
    SMOOTH_TRY(smooth_check_buffers(d_angles, d_pose, d_angles_out));
    if (n > 0 && (!d_workspace || workspace_bytes < seqik_smooth_workspace_bytes(n_seq, n_legs, n_frames)))
        return bad_arg(kWho, "workspace is null or smaller than seqik_smooth_workspace_bytes() asks for");
    if (n > 0 && ((uintptr_t)d_workspace & 7)) return bad_arg(kWho, "workspace must be 8-byte aligned");
    if (n == 0) return SEQIK_OK;
    p.angles = d_angles; p.pose = d_pose; p.kp_weight = d_kp_weight;
    p.angles_out = d_angles_out; p.frame_info = d_frame_info; p.cost = d_cost; p.info = d_info;
    seqik::smooth_carve(p, static_cast<char *>(d_workspace));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const int64_t lanes = n * seqik::kSmoothLanes;

    SMOOTH_TRY(launch_phase<INIT>(p, n, 0, 0, stream));
    SMOOTH_TRY(launch_phase<START_COST>(p, n, 0, 0, stream));
    SMOOTH_TRY(launch_decide<true>(p, stream));
    // every trajectory stops: at most max_iter accepted steps, at most 41 rejections in front of each and behind the last
    const int64_t round_cap = 42 * ((int64_t)p.opt.max_iter + 1);
    for (int64_t round = 0;; ++round) {
        SMOOTH_TRY(launch_phase<ASSEMBLE>(p, n, 0, 0, stream));
        HIP_TRY(hipMemsetAsync(p.active, 0, sizeof(int32_t), stream));
        SMOOTH_TRY(launch_phase<STOP>(p, p.n_traj, 0, 0, stream));
        int32_t active = 0;
        HIP_TRY(hipMemcpyAsync(&active, p.active, sizeof active, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (active == 0) break;
        if (round >= round_cap) return seqik::fail(SEQIK_ERR_HIP, "%s", "seqik_smooth_legs: the trajectories did not stop");
        SMOOTH_TRY(launch_phase<SETUP>(p, lanes, 0, 0, stream));
        int cur = 0;
        for (int64_t h = 1; h < n_frames; h *= 2) {
            SMOOTH_TRY(launch_phase<NORMALISE>(p, lanes, h, cur, stream));
            SMOOTH_TRY(launch_phase<REDUCE>(p, lanes, h, cur, stream));
            cur ^= 1;
        }
        SMOOTH_TRY(launch_phase<FINAL>(p, n, 0, cur, stream));
        SMOOTH_TRY(launch_phase<TRIAL>(p, n, 0, 0, stream));
        SMOOTH_TRY(launch_decide<false>(p, stream));
    }
    return launch_phase<FINISH>(p, n, 0, 0, stream);
}

int seqik_smooth_legs(const double *angles, const double *pose, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                      const SeqikLegParams *legs, int32_t kind, const double *kp_weight, const SeqikSmoothOptions *opt,
                      double *angles_out, int32_t *frame_info, double *cost, int32_t *info, int32_t device)
{
    int64_t n = 0;
    SmoothProblem p;
    SMOOTH_TRY(smooth_validate(n_seq, n_legs, n_frames, legs, kind, opt, &n, &p));
    SMOOTH_TRY(smooth_check_buffers(angles, pose, angles_out));
    if (n == 0) return SEQIK_OK;
    const int64_t ws_bytes = seqik_smooth_workspace_bytes(n_seq, n_legs, n_frames);
    const size_t traj = (size_t)p.n_traj;
    seqik::HostCall call;
    double *d_ang, *d_pose, *d_weight, *d_out, *d_cost;
    int32_t *d_finfo, *d_info;
    char *d_ws;
    call.upload(d_ang, 7 * (size_t)n, angles);
    call.upload(d_pose, 15 * (size_t)n, pose);
    call.upload(d_weight, 4 * (size_t)n, kp_weight);
    call.download(d_out, 7 * (size_t)n, angles_out);
    call.download(d_finfo, (size_t)n, frame_info);
    call.download(d_cost, 2 * traj, cost);
    call.download(d_info, 3 * traj, info);
    call.scratch(d_ws, (size_t)ws_bytes);
    int rc = call.begin(device);
    if (rc != SEQIK_OK) return rc;
    return call.finish(seqik_smooth_legs_device(d_ang, d_pose, n_seq, n_legs, n_frames, legs, kind, d_weight, opt, d_out,
                                                d_finfo, d_cost, d_info, d_ws, ws_bytes, call.stream()));
}

}  // extern "C"
