// TEST INFRASTRUCTURE ONLY -- not part of the product, never loaded by seqikpy_amd.
//
// The round-10 cut of csrc/seqik_core.hpp (bit 1024 of SEQIK_PASS_CUTS: the xtol test of a pass decided from the two sums
// of squares, without the root under ||x||) next to its plain form, run on the HOST so that tests/test_xtol_squares.py can
// compare them without a GPU.  On the host a "wavefront" is one lane, so every row takes its own branch and the harness
// reports which.  Built by that test through tests/harness_build.py: once as it is, and once with -DSEQIK_PASS_CUTS=1023
// so that whole host runs of run_stage with and without the bit can be compared (xs_pass_cuts says which build this is).
#include "../../sequential-inverse-kinematics_amd/csrc/seqik_core.hpp"
#include "../../sequential-inverse-kinematics_amd/csrc/seqik_consts.hpp"
#include <vector>

extern "C" int32_t xs_pass_cuts(void) { return SEQIK_PASS_CUTS; }

extern "C" void xs_constants(double *out)
{
    out[0] = seqik::XTOL_SQ_LO;
    out[1] = seqik::XTOL_SQ_HI;
}

// X [n], step [n][2], na = 2 (stages 1-3) or 1 (stage 4: step[.][1] is not read) ->
// plain[n] = xtol_test<na, false>, cut[n] = xtol_test<na, true>, branch[n] = 1 sure true / 0 sure false / 2 plain form,
// S[n] = the sum of squares under ||step|| as both forms compute it
extern "C" void xs_xtol_test(const double *X, const double *step, int64_t n, int32_t na, int32_t *plain, int32_t *cut,
                             int32_t *branch, double *S)
{
    const double xtol = 1e-8;
    for (int64_t k = 0; k < n; ++k) {
        int br = -1;
        S[k] = step[2 * k] * step[2 * k];
        if (na == 2) S[k] = seqik::fma_(step[2 * k + 1], step[2 * k + 1], S[k]);
        if (na == 2) {
            plain[k] = seqik::xtol_test<2, false>(X[k], step + 2 * k, xtol) ? 1 : 0;
            cut[k] = seqik::xtol_test<2, true>(X[k], step + 2 * k, xtol, &br) ? 1 : 0;
        } else {
            plain[k] = seqik::xtol_test<1, false>(X[k], step + 2 * k, xtol) ? 1 : 0;
            cut[k] = seqik::xtol_test<1, true>(X[k], step + 2 * k, xtol, &br) ? 1 : 0;
        }
        branch[k] = br;
    }
}

// One chain through run_stage<1..4> with forward kinematics and scipy's status / nfev, as the staged launch with
// diagnostics runs it: angles [n][7], fk [n][27], status [n][4], nfev [n][4]
extern "C" int xs_run_chain(const double *pose, int64_t n_frames, const SeqikLegParams *leg, double *angles, double *fk,
                            int32_t *status, int32_t *nfev)
{
    const int rc = seqik::validate_leg(*leg, 1, 4);
    if (rc != SEQIK_OK) return rc;
    seqik::LegConst lc;
    seqik::make_leg_consts(*leg, nullptr, lc);
    std::vector<double> ws((size_t)n_frames * 12 + 1);
    seqik::ChainIO io;
    io.pose = pose; io.pose_row = 3; io.pose_frame = 15;
    io.angles = angles; io.ang_dof = 1; io.ang_frame = 7;
    io.fk = fk; io.status = status; io.nfev = nfev; io.init = nullptr;
    io.frames = ws.data(); io.n_frames = n_frames;
    seqik::run_stage<1, false, true, false, true>(lc, io);
    seqik::run_stage<2, true, true, false, true>(lc, io);
    seqik::run_stage<3, true, true, false, true>(lc, io);
    seqik::run_stage<4, true, true, false, false>(lc, io);
    return SEQIK_OK;
}
