// TEST INFRASTRUCTURE ONLY -- not part of the product, never loaded by seqikpy_amd.
//
// The operands of the first pass of every solve of a chain, from a HOST run of run_stage: what the bit-for-bit tests of the
// per-pass cuts (tests/test_frame_constants.py, tests/test_trans_cuts.py) feed their short and plain forms with.  The one
// place that re-enacts run_stage's start-of-frame sequence.  Built and read by tests/pass_cut_support.py (first_pass_rows).
#include "../../sequential-inverse-kinematics_amd/csrc/seqik_core.hpp"
#include "../../sequential-inverse-kinematics_amd/csrc/seqik_consts.hpp"
#include <vector>

enum { ROW = 28 };   // Jh 6, diag_h 2, f 3, Delta, alpha | x 2, d 2, g_h 2, lb 2, ub 2, theta, T | p_h 2 | stage

// The chain is solved by run_stage<1..4> as the staged launch does it; then for every frame and stage the operands of the
// FIRST pass of that solve are formed from the run's angles with run_stage's own helpers in its order (the header has no
// hook to record operands in flight): prefix, warm start = the previous frame's solution made strictly feasible, residual,
// finite-difference Jacobian, Coleman-Li scaling, Delta_0, the trust-region step p_h, and T = xtol (xtol + ||x||) of the
// post-trial block.  One row of ROW doubles per frame and stage.
template <int STAGE>
static void first_pass(const seqik::LegConst &lc, const double *pose, const double *ang, const double *warm, double *o)
{
    using namespace seqik;
    using Tr = StageTraits<STAGE>;
    constexpr int NA = Tr::NA;
    const StageConst &sc = lc.st[STAGE - 1];
    StageProblem<STAGE> P;
    P.tz_a = sc.tz_a; P.tz_b = sc.tz_b; P.tz_last = sc.tz_last;
    build_prefix<STAGE>(P.pre, lc, ang, 1, nullptr);
    for (int i = 0; i < 3; ++i) P.target[i] = pose[3 * STAGE + i] - pose[i];
    double x[2] = {0.0, 0.0}, f[3], sa, ca, sb, cb, J[3][2], g[2], v[2] = {1.0, 1.0}, dv[2] = {0.0, 0.0}, d[2] = {1.0, 1.0};
    for (int j = 0; j < NA; ++j) x[j] = strictly_feasible(warm[j], sc.lb[j], sc.ub[j], 1e-10);
    eval_residual<STAGE>(P, x[0], x[1], f, sa, ca, sb, cb);
    fd_jacobian<STAGE>(P, x, f, sc.lb, sc.ub, sa, ca, sb, cb, true, J);
    for (int j = 0; j < 2; ++j) g[j] = fma_(J[2][j], f[2], fma_(J[1][j], f[1], J[0][j] * f[0]));
    for (int j = 0; j < NA; ++j) {
        cl_scaling(x[j], g[j], sc.lb[j], sc.ub[j], v[j], dv[j]);
        d[j] = sqrt_pos_(v[j]);
    }
    double acc = sc.x_pre_sq;
    for (int j = 0; j < NA; ++j) { const double t = div_(x[j], d[j]); acc = fma_(t, t, acc); }
    acc = fma_(sc.x_suf, sc.x_suf, acc);
    double Delta = sqrt_(acc);
    if (Delta == 0) Delta = 1.0;
    double Jh[3][2], diag_h[2], g_h[2], p_h[2] = {0.0, 0.0}, alpha = 0.0;
    for (int k = 0; k < 3; ++k) { Jh[k][0] = J[k][0] * d[0]; Jh[k][1] = J[k][1] * d[1]; }
    for (int j = 0; j < 2; ++j) { diag_h[j] = g[j] * dv[j] * 1.0; g_h[j] = d[j] * g[j]; }
    double g_norm = fabs(g[0] * v[0]);
    if (NA == 2) g_norm = fmax(g_norm, fabs(g[1] * v[1]));
    if constexpr (NA == 2) {
        solve_tr_2x2<Tr::DEFICIENT>(Jh, diag_h, f, Delta, alpha, p_h);
    } else {
        double q[2] = {sqrt_(diag_h[0]), 0.0}, s[2], V[2][2], uf[2];
        svd_active<1>(Jh, q, f, s, V, uf);
        solve_lsq_trust_region<1, false>(uf, s, V, Delta, alpha, p_h);
    }
    double xn = sc.x_pre_sq;
    xn = fma_(x[0], x[0], xn);
    if (NA == 2) xn = fma_(x[1], x[1], xn);
    xn = sqrt_(fma_(sc.x_suf, sc.x_suf, xn));
    for (int k = 0; k < 3; ++k) { o[2 * k] = Jh[k][0]; o[2 * k + 1] = Jh[k][1]; o[8 + k] = f[k]; }
    o[6] = diag_h[0]; o[7] = diag_h[1]; o[11] = Delta; o[12] = 0.0;
    for (int j = 0; j < 2; ++j) {
        o[13 + j] = x[j]; o[15 + j] = d[j]; o[17 + j] = g_h[j]; o[19 + j] = sc.lb[j]; o[21 + j] = sc.ub[j]; o[25 + j] = p_h[j];
    }
    o[23] = fmax(0.995, 1 - g_norm);
    o[24] = 1e-8 * (1e-8 + xn);
    o[27] = (double)STAGE;
}

extern "C" int64_t fp_record(const double *pose, int64_t n_frames, const SeqikLegParams *leg, double *rows, int64_t cap)
{
    if (seqik::validate_leg(*leg, 1, 4) != SEQIK_OK) return -1;
    seqik::LegConst lc;
    seqik::make_leg_consts(*leg, nullptr, lc);
    std::vector<double> ang((size_t)n_frames * 7, 0.0), ws((size_t)n_frames * 12 + 1);
    seqik::ChainIO io;
    io.pose = pose; io.pose_row = 3; io.pose_frame = 15;
    io.angles = ang.data(); io.ang_dof = 1; io.ang_frame = 7;
    io.fk = nullptr; io.status = nullptr; io.nfev = nullptr; io.init = nullptr;
    io.frames = ws.data(); io.n_frames = n_frames;
    seqik::run_stage<1, false, false, false, true>(lc, io);
    seqik::run_stage<2, false, false, false, true>(lc, io);
    seqik::run_stage<3, false, false, false, true>(lc, io);
    seqik::run_stage<4, false, false, false, false>(lc, io);
    int64_t n = 0;
    for (int64_t t = 0; t < n_frames && n + 4 <= cap; ++t) {
        const double *a = ang.data() + 7 * t;
        const double *prev = t ? ang.data() + 7 * (t - 1) : nullptr;
        first_pass<1>(lc, pose + 15 * t, a, prev ? prev : lc.st[0].seed, rows + ROW * n++);
        first_pass<2>(lc, pose + 15 * t, a, prev ? prev + 2 : lc.st[1].seed, rows + ROW * n++);
        first_pass<3>(lc, pose + 15 * t, a, prev ? prev + 4 : lc.st[2].seed, rows + ROW * n++);
        first_pass<4>(lc, pose + 15 * t, a, prev ? prev + 6 : lc.st[3].seed, rows + ROW * n++);
    }
    return n;
}
