// seqik_refine.hip -- whole-leg refinement of the sequential fit's angles: kernel and C ABI entry points
// (include/seqik_refine.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "seqik_refine.hpp"
#include "seqik_leg_map.hpp"
#include "../../include/seqik_refine.h"

namespace {

using seqik::bad_arg;

struct RefineArgs {
    const double *angles;     // [n_total][7]
    const double *pose;       // [n_total][5][3]
    const double *kp_weight;  // nullable, [n_total][4]
    double *angles_out;       // [n_total][7]; may be `angles`
    double *cost;             // nullable, [n_total][2]
    int32_t *info;            // nullable, [n_total]
    seqik::RefineOptions opt;
    seqik::LegFrameIndex ix;
    seqik::LegBoundsTable bounds;
};

// One leg-frame per lane, grid-stride over the flat index (64-bit throughout), FP64.  Per leg-frame 56 + 120 (+ 32) B in
// and 56 (+ 16 + 4) B out: the arithmetic of the iterations is everything, so there is no LDS, no staging and no atomics.
// A lane reads its seven angles before it writes them, and no lane reads another's: angles_out may be angles.
// Lanes of a wavefront finish after different numbers of iterations (the shipped recording: median 10, a tail to ~80;
// every rejected step is one more pass of the retry loop), and a wavefront takes as long as its slowest lane.  Nothing
// here redistributes that work.
__global__ void __launch_bounds__(256) seqik_refine_kernel(RefineArgs a)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, n = a.ix.n_total;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int leg = a.ix.leg_of(i);
        seqik::refine_leg_frame(a.ix.legs[leg], a.bounds.b[leg], a.angles + i * 7, a.pose + i * 15,
                                a.kp_weight ? a.kp_weight + i * 4 : nullptr, a.opt, a.angles_out + i * 7,
                                a.cost ? a.cost + i * seqik::kRefineCost : nullptr, a.info ? a.info + i : nullptr);
    }
}

constexpr const char *kWho = "seqik_refine_legs";  // both entry points report under this name

// The checks both entry points make before anything touches HIP; *n_total receives n_seq * n_legs * n_frames, *ro the
// options in force.
int refine_validate(const double *angles, const double *pose, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                    const SeqikLegParams *legs, int32_t kind, const SeqikRefineOptions *opt, const double *angles_out,
                    int64_t *n_total, seqik::RefineOptions *ro)
{
    if (int rc = seqik::check_leg_map(kWho, n_seq, n_legs, n_frames, legs, kind, 15, n_total)) return rc;
    if (kind != SEQIK_FK_KIND_SEQ)
        return bad_arg(kWho, "kind 1 (generic chain) is not built: the refinement exists for the sequential chain only");
    if (!angles) return bad_arg(kWho, "angles must not be null");
    if (!pose) return bad_arg(kWho, "pose must not be null");
    if (!angles_out) return bad_arg(kWho, "angles_out must not be null");
    ro->max_iter = opt ? opt->max_iter : SEQIK_REFINE_MAX_ITER;
    ro->gtol = opt ? opt->gtol : SEQIK_REFINE_GTOL;
    ro->ftol = opt ? opt->ftol : SEQIK_REFINE_FTOL;
    ro->pad_ = 0;
    if (ro->max_iter < 1 || ro->max_iter > 255) return bad_arg(kWho, "max_iter must lie in 1..255");
    if (!(ro->gtol >= 0.0) || !isfinite(ro->gtol)) return bad_arg(kWho, "gtol must be finite and not negative");
    if (!(ro->ftol >= 0.0) || !isfinite(ro->ftol)) return bad_arg(kWho, "ftol must be finite and not negative");
    return SEQIK_OK;
}

}  // namespace

extern "C" {

int seqik_refine_legs_device(const double *d_angles, const double *d_pose, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                             const SeqikLegParams *legs, int32_t kind, const double *d_kp_weight,
                             const SeqikRefineOptions *opt, double *d_angles_out, double *d_cost, int32_t *d_info,
                             void *hip_stream)
{
    int64_t n = 0;
    RefineArgs a;
    int rc = refine_validate(d_angles, d_pose, n_seq, n_legs, n_frames, legs, kind, opt, d_angles_out, &n, &a.opt);
    if (rc != SEQIK_OK) return rc;
    if (n == 0) return SEQIK_OK;
    a.angles = d_angles; a.pose = d_pose; a.kp_weight = d_kp_weight;
    a.angles_out = d_angles_out; a.cost = d_cost; a.info = d_info;
    a.ix.fill(n, n_legs, n_frames, legs);
    a.bounds.fill(n_legs, legs);
    const seqik::LegMapPlan p = seqik::plan_leg_map("SEQIK_REFINE", n, false, 256, 256, 0);
    return seqik::launch_leg_map(seqik_refine_kernel, p, a, hip_stream);
}

int seqik_refine_legs(const double *angles, const double *pose, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                      const SeqikLegParams *legs, int32_t kind, const double *kp_weight, const SeqikRefineOptions *opt,
                      double *angles_out, double *cost, int32_t *info, int32_t device)
{
    int64_t n = 0;
    seqik::RefineOptions ro;
    int rc = refine_validate(angles, pose, n_seq, n_legs, n_frames, legs, kind, opt, angles_out, &n, &ro);
    if (rc != SEQIK_OK) return rc;
    if (n == 0) return SEQIK_OK;
    seqik::HostCall call;
    double *d_ang, *d_pose, *d_weight, *d_out, *d_cost;
    int32_t *d_info;
    call.upload(d_ang, 7 * (size_t)n, angles);
    call.upload(d_pose, 15 * (size_t)n, pose);
    call.upload(d_weight, 4 * (size_t)n, kp_weight);
    call.download(d_out, 7 * (size_t)n, angles_out);
    call.download(d_cost, seqik::kRefineCost * (size_t)n, cost);
    call.download(d_info, (size_t)n, info);
    if ((rc = call.begin(device)) != SEQIK_OK) return rc;
    return call.finish(seqik_refine_legs_device(d_ang, d_pose, n_seq, n_legs, n_frames, legs, kind, d_weight, opt, d_out,
                                                d_cost, d_info, call.stream()));
}

}  // extern "C"
