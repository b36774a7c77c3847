// TEST INFRASTRUCTURE ONLY -- not part of the product, never loaded by seqikpy_amd.
//
// Runs the refinement's device rule (csrc/seqik_refine.hpp, `__host__ __device__`) on the HOST, one leg-frame after the
// other, so that the CPU-only test tier can hold it to its properties, to scipy and to the 200-bit yardstick; the GPU tier
// compares the kernel with it bit for bit.  Built by tests/refine_support.py through harness_build.build_harness.
#include "../../sequential-inverse-kinematics_amd/csrc/seqik_refine.hpp"

// angles [n][7] (DOFS order), pose [n][5][3], kp_weight nullable [n][4]; angles_out [n][7] (may be angles), cost [n][2]
// and info [n] nullable.  The segment lengths are taken as they are: a non-finite one is bad input here (the C ABI
// refuses it before it reaches the rule).
extern "C" int harness_refine_legs(const double *angles, const double *pose, int64_t n, const SeqikLegParams *leg,
                                   const double *kp_weight, int32_t max_iter, double gtol, double ftol, double *angles_out,
                                   double *cost, int32_t *info)
{
    if (!angles || !pose || !angles_out || max_iter < 1 || max_iter > 255) return SEQIK_ERR_BAD_ARG;
    seqik::FkLeg fl;
    seqik::LegBounds sb;
    seqik::make_fk_leg(*leg, fl);
    seqik::make_leg_bounds(*leg, sb);
    seqik::RefineOptions opt;
    opt.max_iter = max_iter; opt.gtol = gtol; opt.ftol = ftol; opt.pad_ = 0;
    for (int64_t i = 0; i < n; ++i)
        seqik::refine_leg_frame(fl, sb, angles + i * 7, pose + i * 15, kp_weight ? kp_weight + i * 4 : nullptr, opt,
                                angles_out + i * 7, cost ? cost + i * 2 : nullptr, info ? info + i : nullptr);
    return SEQIK_OK;
}
