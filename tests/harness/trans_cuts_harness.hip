// TEST INFRASTRUCTURE ONLY -- not part of the product, never loaded by seqikpy_amd.
//
// The four round-9 cuts of csrc/seqik_core.hpp (bits 32, 64, 128, 512 of SEQIK_PASS_CUTS: divisions and square roots whose
// value nothing reads as a value) next to their plain forms, run on the HOST so that tests/test_trans_cuts.py can compare them
// bit for bit without a GPU.  On the host a "wavefront" is one lane, so every row takes its own branch and the harness
// reports which.  Built by that test through tests/harness_build.py.  The operands recorded from host runs of run_stage
// that the test feeds these with come from first_pass_harness.hip.
#include "../../sequential-inverse-kinematics_amd/csrc/seqik_core.hpp"
#include "../../sequential-inverse-kinematics_amd/csrc/seqik_consts.hpp"
#include <string.h>

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
