// TEST INFRASTRUCTURE ONLY -- not part of the product, never loaded by seqikpy_amd.
//
// Runs the device rule of the refinement's sensitivity (csrc/seqik_refine_sens.hpp, `__host__ __device__`) on the HOST, one
// leg-frame after the other, so that the CPU-only test tier can hold it to its yardstick, its identities and the solver;
// the GPU tier compares the kernel with it bit for bit.  Built by tests/refine_sens_support.py through
// harness_build.build_harness.
#include "../../sequential-inverse-kinematics_amd/csrc/seqik_refine_sens.hpp"
#include "staged_pass.hpp"

// angles [n][7] (DOFS order), pose [n][5][3], kp_weight and kp_sigma nullable [n][4]; sens [n][7][4][3], std [n][7], grad
// [n], flags [n]: each nullable (std needs kp_sigma)
extern "C" int harness_refine_sensitivity(const double *angles, const double *pose, int64_t n, const SeqikLegParams *leg,
                                          const double *kp_weight, const double *kp_sigma, double bound_tol, double *sens,
                                          double *std_out, double *grad, int32_t *flags)
{
    if (!angles || !pose || (std_out && !kp_sigma) || !(bound_tol >= 0.0)) return SEQIK_ERR_BAD_ARG;
    seqik::FkLeg fl;
    seqik::LegBounds sb;
    seqik::make_fk_leg(*leg, fl);
    seqik::make_leg_bounds(*leg, sb);
    for (int64_t i = 0; i < n; ++i)
        seqik::refsens_leg_frame(fl, sb, angles + i * 7, pose + i * 15, kp_weight ? kp_weight + i * 4 : nullptr,
                                 kp_sigma ? kp_sigma + i * 4 : nullptr, bound_tol, sens ? sens + i * seqik::kSensRow : nullptr,
                                 std_out ? std_out + i * seqik::kSensStd : nullptr, grad ? grad + i : nullptr,
                                 flags ? flags + i : nullptr);
    return SEQIK_OK;
}

// The kernel's staged pass on the host (staged_pass.hpp), n a multiple of 16: must equal harness_refine_sensitivity bit
// for bit.
extern "C" int harness_refine_sensitivity_staged(const double *angles, const double *pose, int64_t n,
                                                 const SeqikLegParams *leg, const double *kp_weight, double bound_tol,
                                                 double *sens)
{
    if (n % 16) return SEQIK_ERR_BAD_ARG;
    seqik::FkLeg fl;
    seqik::LegBounds sb;
    seqik::make_fk_leg(*leg, fl);
    seqik::make_leg_bounds(*leg, sb);
    staged_pass_host<seqik::kSensQuad>(n, sens, [&](int64_t rec, seqik::QuadSink<seqik::kSensQuad> &quad) {
        seqik::QuadAnySink<seqik::kSensQuad> sink{quad};
        sink.clear();
        seqik::refsens_rule<true>(fl, sb, angles + rec * 7, pose + rec * 15, kp_weight ? kp_weight + rec * 4 : nullptr,
                                  nullptr, bound_tol, sink, nullptr, nullptr, nullptr);
    });
    return SEQIK_OK;
}

// The masked factorisation alone on a hand-made matrix: H [7][7] (the lower triangle is read) -> the factor in place and
// whether every pivot was positive.
extern "C" int harness_refsens_factor(double *H, int32_t held)
{
    double M[7][7];
    for (int i = 0; i < 7; ++i)
        for (int j = 0; j < 7; ++j) M[i][j] = H[7 * i + j];
    const bool pd = seqik::refsens_factor(M, held);
    for (int i = 0; i < 7; ++i)
        for (int j = 0; j < 7; ++j) H[7 * i + j] = M[i][j];
    return pd ? 1 : 0;
}
