// TEST INFRASTRUCTURE ONLY -- not part of the product, never loaded by seqikpy_amd.
//
// Runs the device rule of the smoothed trajectory's error bars (csrc/seqik_smooth_sens.hpp, `__host__ __device__`) on the
// HOST, phase after phase in plain loops, so that the CPU-only test tier can hold it to dense numpy, to its identities and
// to seqik_refine_sensitivity; the GPU tier compares the kernels with it bit for bit.  Built by tests/smooth_sens_support.py
// through harness_build.build_harness.
#include <string.h>
#include <vector>

#include "../../sequential-inverse-kinematics_amd/csrc/seqik_smooth_sens.hpp"

namespace {

void size_problem(seqik::SmoothSensProblem &p, int64_t n_traj, int32_t n_legs, int64_t n_frames, std::vector<char> &ws)
{
    memset(&p, 0, sizeof p);
    p.sp.n_traj = n_traj; p.sp.n_legs = n_legs; p.sp.n_frames = n_frames;
    ws.assign(seqik::ssens_carve(p, nullptr) + 8, 0);
    seqik::ssens_carve(p, ws.data() + (8 - (uintptr_t)ws.data() % 8) % 8);
}

// The right-hand sides of the linear part: the caller's B [7][12]; a held row is 0
struct LinearRhs {
    const double *B;
    int held;
    template <int K0> void fill(double (&b)[7][3]) const
    {
        for (int d = 0; d < 7; ++d)
            for (int c = 0; c < 3; ++c) b[d][c] = ((held >> d) & 1) ? 0.0 : B[12 * d + 3 * K0 + c];
    }
};

}  // namespace

// The layouts of include/seqik_smooth_sensitivity.h; smooth [7] is required.  The segment lengths are taken as they are
// (the C ABI refuses a non-finite one before it reaches the rule).
extern "C" int harness_smooth_sensitivity(const double *angles, const double *pose, int64_t n_seq, int32_t n_legs,
                                          int64_t n_frames, const SeqikLegParams *legs, const double *kp_weight,
                                          const double *kp_sigma, const double *smooth, double bound_tol, int32_t half_width,
                                          double *sens, double *std_out, double *grad, int32_t *flags)
{
    if (!angles || !pose || !legs || !smooth || n_legs < 1 || n_legs > 8 || (std_out && !kp_sigma) || !(bound_tol >= 0.0) ||
        half_width < 0 || half_width > seqik::kSsensMaxHalfWidth || (!sens && !std_out && !grad && !flags))
        return SEQIK_ERR_BAD_ARG;
    if (n_seq * n_legs * n_frames == 0) return SEQIK_OK;
    seqik::SmoothSensProblem p;
    std::vector<char> ws;
    size_problem(p, n_seq * n_legs, n_legs, n_frames, ws);
    p.angles = angles; p.pose = pose; p.kp_weight = kp_weight; p.kp_sigma = std_out ? kp_sigma : nullptr;
    p.sens = sens; p.std_out = std_out; p.grad = grad; p.flags = flags;
    p.tol = bound_tol; p.half_width = half_width;
    for (int j = 0; j < 7; ++j) p.sp.opt.smooth[j] = smooth[j];
    for (int l = 0; l < seqik::kFkMaxLegs; ++l) {
        seqik::make_fk_leg(legs[l < n_legs ? l : 0], p.sp.legs[l]);
        seqik::make_leg_bounds(legs[l < n_legs ? l : 0], p.sp.bounds[l]);
    }
    seqik::ssens_run_host(p);
    return SEQIK_OK;
}

// The linear part alone, one trajectory of n frames on the caller's blocks: H [n][7][7] (the lower triangle is read; the
// rows and columns of held DOFs are replaced by the identity's here, as assemble does), word [n] (bits 0..6 held, bit 24 an
// identity row that cuts the coupling), s [7] (K_t = diag(s) under the masks of rule 4), B [n][7][12], sigma [n][4] ->
// sens [n][2 W + 1][7][12] (G_{t,t+d-W} B_{t+d-W}), std [n][7], flags [n].  The sweeps, the combine and the finish are the
// rule's own functions; only the right-hand sides come from B instead of the chain.
extern "C" int harness_smooth_sens_linear(const double *H, const int32_t *word, int64_t n, const double *s, const double *B,
                                          const double *sigma, int32_t half_width, double *sens, double *std_out,
                                          int32_t *flags)
{
    if (!H || !word || !s || !B || !sigma || !sens || !std_out || !flags || n < 1 || half_width < 0 ||
        half_width > seqik::kSsensMaxHalfWidth)
        return SEQIK_ERR_BAD_ARG;
    seqik::SmoothSensProblem p;
    std::vector<char> ws;
    size_problem(p, 1, 1, n, ws);
    p.kp_sigma = sigma; p.sens = sens; p.std_out = std_out; p.flags = flags;
    p.half_width = half_width;
    for (int j = 0; j < 7; ++j) p.sp.opt.smooth[j] = s[j];
    p.sp.legs[0].nseg[0] = -1.0;  // len^2 = 1: smooth_stiffness gives s itself
    for (int64_t r = 0; r < n; ++r) {
        double M[7][7];
        for (int i = 0; i < 7; ++i)
            for (int j = 0; j < 7; ++j) M[i][j] = H[49 * r + 7 * i + j];
        p.sp.held[r] = word[r] & (0x7f | seqik::REFINE_BAD_INPUT);
        seqik::ssens_store_H(p, r, M, word[r] & 0x7f);
    }
    for (int dir = 0; dir < 2; ++dir) seqik::ssens_schur_sweep(p, 0, dir);
    const double ones[4] = {1.0, 1.0, 1.0, 1.0};
    for (int64_t r = 0; r < n; ++r) {
        if (seqik::smooth_bad(p.sp, r)) {
            seqik::ssens_combine_bad(p, r);
            continue;
        }
        double L[7][7];
        const bool ok = seqik::ssens_verdict(p, r, seqik::smooth_at(p.sp, r), L);
        const LinearRhs rhs{B + 84 * r, p.sp.held[r] & 0x7f};
        seqik::ssens_centre(p, r, L, ok, rhs, ones);
    }
    for (int dir = 0; dir < 2; ++dir) seqik::ssens_cov_sweep(p, 0, dir);
    for (int64_t r = 0; r < n; ++r) seqik::ssens_finish(p, r);
    return SEQIK_OK;
}
