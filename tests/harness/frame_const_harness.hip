// TEST INFRASTRUCTURE ONLY -- not part of the product, never loaded by seqikpy_amd.
//
// The two round-8 cuts of csrc/seqik_core.hpp next to their plain forms, run on the HOST so that
// tests/test_frame_constants.py can compare them bit for bit without a GPU:
//   bit 8   residual_sc<STAGE, true> (translation of the frame after the active links kept in StageProblem::t_act) against
//           residual_sc_general<STAGE>, and frame_after_active with t replaced by t_act against the plain call;
//   bit 16  solve_tr_2x2<false, true> (Gauss-Newton step and norm kept) against solve_tr_2x2<false, false>.
// Built by that test through tests/harness_build.py.  The operands of solve_tr_2x2 recorded from host runs of run_stage come
// from first_pass_harness.hip (stages 2 and 3, columns 0..12).
#include "../../sequential-inverse-kinematics_amd/csrc/seqik_core.hpp"
#include "../../sequential-inverse-kinematics_amd/csrc/seqik_consts.hpp"
#include <string.h>

static uint64_t bits_of(double v)
{
    uint64_t u;
    memcpy(&u, &v, sizeof u);
    return u;
}

// prefix frames of STAGE as run_stage<.., FROM_ANGLES> builds them: angles [n][7] -> pre [n][12] (r 9, t 3);
// tz[3] = {tz_a, tz_b, tz_last} of the stage
extern "C" int fc_prefixes(int32_t stage, const SeqikLegParams *leg, const double *angles, int64_t n, double *pre12, double *tz)
{
    seqik::LegConst lc;
    seqik::make_leg_consts(*leg, nullptr, lc);
    if (stage < 2 || stage > 4) return -1;
    tz[0] = lc.st[stage - 1].tz_a; tz[1] = lc.st[stage - 1].tz_b; tz[2] = lc.st[stage - 1].tz_last;
    for (int64_t k = 0; k < n; ++k) {
        seqik::Frame pre;
        if (stage == 2) seqik::build_prefix<2>(pre, lc, angles + 7 * k, 1, nullptr);
        else if (stage == 3) seqik::build_prefix<3>(pre, lc, angles + 7 * k, 1, nullptr);
        else seqik::build_prefix<4>(pre, lc, angles + 7 * k, 1, nullptr);
        for (int i = 0; i < 9; ++i) pre12[12 * k + i] = pre.r[i];
        for (int i = 0; i < 3; ++i) pre12[12 * k + 9 + i] = pre.t[i];
    }
    return 0;
}

template <int STAGE>
static void fc_eval_one(const double *pre12, const double *tz, const double *target, const double *sc, int64_t *bad)
{
    seqik::StageProblem<STAGE> P;
    for (int i = 0; i < 9; ++i) P.pre.r[i] = pre12[i];
    for (int i = 0; i < 3; ++i) { P.pre.t[i] = pre12[9 + i]; P.target[i] = target[i]; }
    P.tz_a = tz[0]; P.tz_b = tz[1]; P.tz_last = tz[2];
    seqik::stage_translation<STAGE>(P);
    const double sa = sc[0], ca = sc[1];
    const double sb = (STAGE == 4) ? 0.0 : sc[2], cb = (STAGE == 4) ? 1.0 : sc[3];   // (as eval_residual sets them)
    double g[6], h[6];
    seqik::residual_sc_general<STAGE>(P, sa, ca, sb, cb, g, g + 3);
    seqik::residual_sc<STAGE, true>(P, sa, ca, sb, cb, h, h + 3);
    for (int i = 0; i < 6; ++i) bad[0] += bits_of(g[i]) != bits_of(h[i]);
    // without pe (the form the three evaluations of a pass use)
    double h2[3];
    seqik::residual_sc<STAGE, true>(P, sa, ca, sb, cb, h2);
    for (int i = 0; i < 3; ++i) bad[0] += bits_of(g[i]) != bits_of(h2[i]);
    // the frame at the frame's end: plain, and with the translation taken from t_act (what run_stage stores)
    seqik::Frame plain, kept;
    seqik::frame_after_active<STAGE>(P, sa, ca, sb, cb, plain);
    seqik::frame_after_active<STAGE>(P, sa, ca, sb, cb, kept);
    for (int i = 0; i < 3; ++i) kept.t[i] = P.t_act[i];
    for (int i = 0; i < 9; ++i) bad[1] += bits_of(plain.r[i]) != bits_of(kept.r[i]);
    for (int i = 0; i < 3; ++i) bad[1] += bits_of(plain.t[i]) != bits_of(kept.t[i]);
}

// n operand sets, one per row: pre [n][12], tz [n][3], target [n][3], sc [n][4] = {sa, ca, sb, cb}.
// bad[0] = differing words of f / pe, bad[1] = differing entries of the frame after the active links; *first = first bad row
extern "C" int fc_compare(int32_t stage, const double *pre12, const double *tz, const double *target, const double *sc, int64_t n,
                          int64_t *bad, int64_t *first)
{
    bad[0] = bad[1] = 0;
    *first = -1;
    for (int64_t k = 0; k < n; ++k) {
        const int64_t before = bad[0] + bad[1];
        if (stage == 2) fc_eval_one<2>(pre12 + 12 * k, tz + 3 * k, target + 3 * k, sc + 4 * k, bad);
        else if (stage == 3) fc_eval_one<3>(pre12 + 12 * k, tz + 3 * k, target + 3 * k, sc + 4 * k, bad);
        else if (stage == 4) fc_eval_one<4>(pre12 + 12 * k, tz + 3 * k, target + 3 * k, sc + 4 * k, bad);
        else return -1;
        if (*first < 0 && bad[0] + bad[1] != before) *first = k;
    }
    return 0;
}

extern "C" void fc_sincos(const double *x, int64_t n, double *sc2)
{
    for (int64_t i = 0; i < n; ++i) seqik::sincos_cw(x[i], sc2[2 * i], sc2[2 * i + 1]);
}

// ---- bit 16 ---------------------------------------------------------------------------------------------------------------
// Which way solve_tr_2x2<false> goes for these operands, worked out here with the function's own expressions:
//   0  rank deficient (lmin under the threshold): no Gauss-Newton step
//   1  full rank, Gauss-Newton step inside the trust region (returned as it is)
//   2  full rank, outside: the branch bit 16 changes
// gn_norm: norm of the Gauss-Newton step (NaN in branch 0)
static int tr2_branch(const double Jh[3][2], const double *diag_h, const double *f, double Delta, double *gn_norm)
{
    using namespace seqik;
    double a = diag_h[0], b = 0.0, c = diag_h[1], r[2], pp[2];
    for (int k = 0; k < 3; ++k) {
        a = fma_(Jh[k][0], Jh[k][0], a);
        b = fma_(Jh[k][0], Jh[k][1], b);
        c = fma_(Jh[k][1], Jh[k][1], c);
    }
    r[0] = fma_(Jh[2][0], f[2], fma_(Jh[1][0], f[1], Jh[0][0] * f[0]));
    r[1] = fma_(Jh[2][1], f[2], fma_(Jh[1][1], f[1], Jh[0][1] * f[0]));
    double h = 0.5 * (a - c);
    double lmax = fma_(0.5, a + c, sqrt_(fma_(h, h, b * b)));
    double lmin = div_(fma_(a, c, -(b * b)), lmax);
    *gn_norm = __builtin_nan("");
    if (!(lmin > 4.437342591868191e-31 * lmax)) return 0;
    tr2_apply(a + 0.0, b, c + 0.0, r, pp);
    *gn_norm = sqrt_(fma_(pp[1], pp[1], pp[0] * pp[0]));
    return (*gn_norm <= Delta) ? 1 : 2;
}

// n operand sets, one per row: ops [n][13] = {Jh[3][2], diag_h[2], f[3], Delta, alpha}.  Runs both forms; bad = rows whose
// p or alpha differ in any bit; counts[3] = rows per branch; branch[n], gn_norm[n] (nullable) per row; out [n][3] (nullable) =
// {p[0], p[1], alpha} of the kept form
extern "C" int64_t fc_tr2_compare(const double *ops, int64_t n, int64_t *counts, int32_t *branch, double *gn_norm, double *out,
                                  int64_t *first)
{
    int64_t bad = 0;
    counts[0] = counts[1] = counts[2] = 0;
    *first = -1;
    for (int64_t k = 0; k < n; ++k) {
        const double *o = ops + 13 * k;
        double Jh[3][2];
        for (int i = 0; i < 3; ++i) { Jh[i][0] = o[2 * i]; Jh[i][1] = o[2 * i + 1]; }
        double gn;
        const int br = tr2_branch(Jh, o + 6, o + 8, o[11], &gn);
        counts[br] += 1;
        if (branch) branch[k] = br;
        if (gn_norm) gn_norm[k] = gn;
        double p0[2] = {0.0, 0.0}, p1[2] = {0.0, 0.0}, a0 = o[12], a1 = o[12];
        seqik::solve_tr_2x2<false, false>(Jh, o + 6, o + 8, o[11], a0, p0);
        seqik::solve_tr_2x2<false, true>(Jh, o + 6, o + 8, o[11], a1, p1);
        if (out) { out[3 * k] = p1[0]; out[3 * k + 1] = p1[1]; out[3 * k + 2] = a1; }
        if (bits_of(p0[0]) != bits_of(p1[0]) || bits_of(p0[1]) != bits_of(p1[1]) || bits_of(a0) != bits_of(a1)) {
            if (bad == 0) *first = k;
            ++bad;
        }
    }
    return bad;
}
