// TEST INFRASTRUCTURE ONLY -- not part of the product, never loaded by seqikpy_amd.
//
// The four round-9 cuts of csrc/seqik_core.hpp (bits 32, 64, 128, 512 of SEQIK_PASS_CUTS: divisions and square roots whose
// value nothing reads as a value) next to their plain forms, run on the HOST so that tests/test_trans_cuts.py can compare them
// bit for bit without a GPU.  On the host a "wavefront" is one lane, so every row takes its own branch and the harness
// reports which.  Built by that test with `hipcc --offload-host-only`, like pass_path_harness.hip.
#include "../../sequential-inverse-kinematics_amd/csrc/seqik_core.hpp"
#include "../../sequential-inverse-kinematics_amd/csrc/seqik_consts.hpp"
#include <string.h>
#include <vector>

static uint64_t bits_of(double v)
{
    uint64_t u;
    memcpy(&u, &v, sizeof u);
    return u;
}

static bool same(double a, double b) { return bits_of(a) == bits_of(b) || (a != a && b != b); }   // (NaN stays NaN)

// ---- A (bit 32) --------------------------------------------------------------------------------------------------------------
// abc [n][3] -> sure[n] = tr2_rank_sure, plain[n] = tr2_rank_plain
extern "C" void tc_rank(const double *abc, int64_t n, int32_t *sure, int32_t *plain)
{
    for (int64_t k = 0; k < n; ++k) {
        sure[k] = seqik::tr2_rank_sure(abc[3 * k], abc[3 * k + 1], abc[3 * k + 2]) ? 1 : 0;
        plain[k] = seqik::tr2_rank_plain(abc[3 * k], abc[3 * k + 1], abc[3 * k + 2]) ? 1 : 0;
    }
}

// ops [n][13] = {Jh[3][2], diag_h[2], f[3], Delta, alpha}: a, b, c as solve_tr_2x2 forms them
extern "C" void tc_abc(const double *ops, int64_t n, double *abc)
{
    using namespace seqik;
    for (int64_t k = 0; k < n; ++k) {
        const double *o = ops + 13 * k;
        double a = o[6], b = 0.0, c = o[7];
        for (int i = 0; i < 3; ++i) {
            a = fma_(o[2 * i], o[2 * i], a);
            b = fma_(o[2 * i], o[2 * i + 1], b);
            c = fma_(o[2 * i + 1], o[2 * i + 1], c);
        }
        abc[3 * k] = a; abc[3 * k + 1] = b; abc[3 * k + 2] = c;
    }
}

// solve_tr_2x2<false> with and without the guard on n operand sets; returns the rows whose p or alpha differ
extern "C" int64_t tc_tr2_compare(const double *ops, int64_t n, int64_t *first)
{
    int64_t bad = 0;
    *first = -1;
    for (int64_t k = 0; k < n; ++k) {
        const double *o = ops + 13 * k;
        double Jh[3][2];
        for (int i = 0; i < 3; ++i) { Jh[i][0] = o[2 * i]; Jh[i][1] = o[2 * i + 1]; }
        double p0[2] = {0.0, 0.0}, p1[2] = {0.0, 0.0}, a0 = o[12], a1 = o[12];
        seqik::solve_tr_2x2<false, true, false>(Jh, o + 6, o + 8, o[11], a0, p0);
        seqik::solve_tr_2x2<false, true, true>(Jh, o + 6, o + 8, o[11], a1, p1);
        if (!same(p0[0], p1[0]) || !same(p0[1], p1[1]) || !same(a0, a1)) {
            if (bad == 0) *first = k;
            ++bad;
        }
    }
    return bad;
}

// ---- B (bit 64) --------------------------------------------------------------------------------------------------------------
// plain[n] = sqrt(S) < T, cut[n] = step_below<true>, branch[n] = 1 decided true / 0 decided false / 2 plain form
extern "C" void tc_step_below(const double *S, const double *T, int64_t n, int32_t *plain, int32_t *cut, int32_t *branch)
{
    for (int64_t k = 0; k < n; ++k) {
        plain[k] = seqik::step_below<false>(S[k], T[k]) ? 1 : 0;
        int br = -1;
        cut[k] = seqik::step_below<true>(S[k], T[k], &br) ? 1 : 0;
        branch[k] = br;
    }
}

// ---- C (bit 128) -------------------------------------------------------------------------------------------------------------
extern "C" void tc_norm1(const double *a0, int64_t n, double *plain, double *cut, int32_t *short_form)
{
    for (int64_t k = 0; k < n; ++k) {
        const double a[2] = {a0[k], 0.0};
        bool sf = false;
        plain[k] = seqik::norm2v<1, false>(a);
        cut[k] = seqik::norm2v<1, true>(a, &sf);
        short_form[k] = sf ? 1 : 0;
    }
}

// ---- E (bit 512) -------------------------------------------------------------------------------------------------------------
extern "C" void tc_first_alpha(const double *au, int64_t n, double *plain, double *cut)
{
    for (int64_t k = 0; k < n; ++k) {
        plain[k] = seqik::tr_first_alpha<false>(au[k]);
        cut[k] = seqik::tr_first_alpha<true>(au[k]);
    }
}

enum { ROW = 28 };   // Jh 6, diag_h 2, f 3, Delta, alpha | x 2, d 2, g_h 2, lb 2, ub 2, theta, T | p_h 2 | stage

// ---- operands from host runs of run_stage ------------------------------------------------------------------------------------
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

extern "C" int64_t tc_record(const double *pose, int64_t n_frames, const SeqikLegParams *leg, double *rows, int64_t cap)
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
