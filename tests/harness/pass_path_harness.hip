// TEST INFRASTRUCTURE ONLY -- not part of the product, never loaded by seqikpy_amd.
//
// The per-pass helpers of csrc/seqik_core.hpp that have a short form next to their general form (sincos_cw's quadrant
// signs, fd_step / fd_step_wide, residual_sc_general<1> / residual_sc_stage1), run on the HOST so that
// tests/test_pass_path_cuts.py can compare the forms bit for bit without a GPU.  Built by that test with
// `hipcc --offload-host-only`, like host_harness.hip.
#include "../../sequential-inverse-kinematics_amd/csrc/seqik_core.hpp"
#include "../../sequential-inverse-kinematics_amd/csrc/seqik_consts.hpp"
#include <string.h>

static uint64_t bits_of(double v)
{
    uint64_t u;
    memcpy(&u, &v, sizeof u);
    return u;
}

// sincos_cw against a reference routine (the oracle's, passed as a function pointer) on n angles: number of angles
// whose sine or cosine differs in any bit; *first = index of the first such angle (-1: none)
extern "C" int64_t pp_sincos_mismatches(void (*ref)(double, double *, double *), const double *x, int64_t n, int64_t *first)
{
    int64_t bad = 0;
    *first = -1;
    for (int64_t i = 0; i < n; ++i) {
        double s, c, rs, rc;
        seqik::sincos_cw(x[i], s, c);
        ref(x[i], &rs, &rc);
        if (bits_of(s) != bits_of(rs) || bits_of(c) != bits_of(rc)) {
            if (bad == 0) *first = i;
            ++bad;
        }
    }
    return bad;
}

// per-stage constants of a leg that the tests look at: out[stage][joint] = {lb_out, sin, cos, ub_out, sin, cos},
// flags[stage] = StageConst::fd_wide
extern "C" void pp_leg_consts(const SeqikLegParams *leg, double *out /* [4][2][6] */, int32_t *flags /* [4] */)
{
    seqik::LegConst lc;
    seqik::make_leg_consts(*leg, nullptr, lc);
    for (int st = 0; st < 4; ++st) {
        flags[st] = lc.st[st].fd_wide;
        for (int j = 0; j < 2; ++j) {
            double *o = out + (st * 2 + j) * 6;
            o[0] = lc.st[st].lb_out[j]; o[1] = lc.st[st].sc_lb[j][0]; o[2] = lc.st[st].sc_lb[j][1];
            o[3] = lc.st[st].ub_out[j]; o[4] = lc.st[st].sc_ub[j][0]; o[5] = lc.st[st].sc_ub[j][1];
        }
    }
}

extern "C" int32_t pp_fd_limits_wide(double lb, double ub) { return seqik::fd_limits_wide(lb, ub) ? 1 : 0; }

// fd_step (general) and fd_step_wide on n points of one limit pair
extern "C" void pp_fd_steps(const double *x, int64_t n, double lb, double ub, double *general, double *wide)
{
    for (int64_t i = 0; i < n; ++i) {
        general[i] = seqik::fd_step(x[i], lb, ub);
        wide[i] = seqik::fd_step_wide(x[i], lb, ub);
    }
}

// the finite-difference steps as run_stage takes them: fd_jacobian<2> of a made-up problem with the stage's flag
// (fd_general = some joint is not wide), J returned; `general` = 1 forces the general routine (what the flag must give
// whenever it is clear)
extern "C" void pp_fd_jacobian(const double *x, const double *lb, const double *ub, int32_t general, double *J6)
{
    seqik::StageProblem<2> P;
    seqik::frame_identity(P.pre);
    P.pre.r[0] = 0.6; P.pre.r[1] = -0.8; P.pre.r[3] = 0.8; P.pre.r[4] = 0.6; P.pre.t[0] = 0.1; P.pre.t[2] = -0.3;
    P.tz_a = 0.0; P.tz_b = -0.4; P.tz_last = -0.7;
    P.target[0] = 0.2; P.target[1] = -0.1; P.target[2] = -0.9;
    double f[3], sa, ca, sb, cb, J[3][2];
    seqik::eval_residual<2>(P, x[0], x[1], f, sa, ca, sb, cb);
    const bool fd_general = general || !(seqik::fd_limits_wide(lb[0], ub[0]) && seqik::fd_limits_wide(lb[1], ub[1]));
    seqik::fd_jacobian<2>(P, x, f, lb, ub, sa, ca, sb, cb, fd_general, J);
    for (int k = 0; k < 3; ++k) { J6[2 * k] = J[k][0]; J6[2 * k + 1] = J[k][1]; }
}

// stage 1's end-effector evaluation in both forms: out = {f[3], pe[3]} each
extern "C" void pp_stage1_eval(double sa, double ca, double sb, double cb, double tz_last, const double *target,
                               double *out_general, double *out_closed)
{
    seqik::StageProblem<1> P;
    seqik::frame_identity(P.pre);
    P.tz_a = 0.0; P.tz_b = 0.0; P.tz_last = tz_last;
    for (int i = 0; i < 3; ++i) P.target[i] = target[i];
    seqik::residual_sc_general<1>(P, sa, ca, sb, cb, out_general, out_general + 3);
    seqik::residual_sc_stage1(tz_last, target, sa, ca, sb, cb, out_closed, out_closed + 3);
}
