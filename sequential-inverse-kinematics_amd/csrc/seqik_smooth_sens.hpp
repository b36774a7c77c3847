// seqik_smooth_sens.hpp -- error bars of the smoothed trajectory (include/seqik_smooth_sensitivity.h): the device rule,
// host-runnable.
//
// The header states the rule; this file fixes its arithmetic so that the rule run on the host and the kernels agree bit
// for bit (-ffp-contract=off, correctly rounded sqrt and /).  The rule is cut into five PHASES, each a function of one work
// item that reads only what earlier phases stored in the workspace: the kernels of seqik_smooth_sens.hip run one phase per
// launch, ssens_run_host below runs the same functions in loops.  No two items of a phase write the same word.
//
//   assemble   (frame)  whether the frame and its two neighbours are usable (smooth_targets, angle_in_domain); chain walk,
//              refine_residual, refsens_hessian -> H (lower triangle), g; the penalty's share of g and of the diagonal of H
//              in smooth_assemble's order; held by sens_held on the full g; grad; the bad-sigma bit; H with the rows and
//              columns of held DOFs replaced by the identity's -> workspace (28 doubles).  The frame's word (bits 0..6
//              held, 17 bad sigma, REFINE_BAD_INPUT bad) goes where smooth_bad / smooth_pair of seqik_smooth.hpp read it.
//   schur      (trajectory, direction)  serial over the frames: S = H - k_i P_prev[i][j] where the incoming pair is coupled,
//              refsens_factor, P = S^-1 K_out column by column with smooth_substitute; pivot poisoning.
//   combine    (frame)  T = (Sf + Sb) - H with Sf, Sb formed again from the stored P of the neighbours (the same
//              expression, hence the same bits), refsens_factor, the verdict (bit 8) into mark[0] and flags; then
//              the centre block: per key point b = refsens_rhs, three smooth_substitute, the selects and acc of
//              seqik_refine_sens.hpp; Wt (28 doubles) -> workspace; own_j is parked in std.
//   cov        (trajectory, direction)  serial: X = P ((X + Wt_prev) P^T), its diagonal and whether a frame earlier in the
//              run is sick (poisoned, or bit 17) -> workspace.
//   finish     (frame)  std from own, Lam, Ups and the sick marks; the off-centre blocks Q_m sens0_s, Q built from the
//              stored P of at most half_width frames.
// Every product of matrices is smooth_dot7's p_0, then + p_1, ... + p_6.
//
// Deliberately done more than once: assemble tests the usability of a frame AND of its two neighbours (so every frame's
// test runs three times), and combine walks the chain a second time for the right-hand sides.  The alternatives are a sixth
// launch in front of assemble and 84 more doubles of workspace per frame; the per-frame launches are 2 % of the unit, the
// serial sweeps the rest.
#pragma once
#include <stdint.h>
#include <utility>

#include "seqik_refine_sens.hpp"
#include "seqik_smooth.hpp"

namespace seqik {

constexpr int32_t SSENS_FLAG_NOT_PD = 1 << 8;
constexpr int32_t SSENS_FLAG_BAD_INPUT = 1 << 16;
constexpr int32_t SSENS_FLAG_BAD_SIGMA = 1 << 17;
constexpr int kSsensMaxHalfWidth = 32;
constexpr int kSsensTri = 28;  // doubles of the lower triangle of a 7 x 7 block
constexpr int kSsensFrameBytes = 8 * (2 * kSsensTri + 2 * 49 + 2 * 7) + 4 * 5;  // 1364

constexpr int ssens_tri(int i, int j) { return i * (i + 1) / 2 + j; }  // j <= i

struct SmoothSensProblem {
    // Sizes, leg tables and smooth of the fit; sp.held is the frame word of this unit (the other pointers of sp are unused).
    SmoothProblem sp;
    const double *angles;     // [R][7]
    const double *pose;       // [R][5][3]
    const double *kp_weight;  // nullable, [R][4]
    const double *kp_sigma;   // nullable, [R][4]; given exactly when std is
    double *sens;             // nullable, [R][2 W + 1][7][4][3]
    double *std_out;          // nullable, [R][7]
    double *grad;             // nullable, [R]
    int32_t *flags;           // nullable, [R]
    // the workspace
    double *H;         // [R][28]: the masked H_tt, lower triangle
    double *P[2];      // [R][49]: Pf, Pb
    double *Wt;        // [R][28]
    double *D[2];      // [R][7]: the diagonals of Lam, Ups
    int32_t *mark[4];  // [R]: poisoned by Sf (after combine: the frame's verdict), by Sb; a sick frame earlier, later in the run
    double tol;
    int32_t half_width, pad_;
};

// Bytes of workspace for p.sp.n_traj trajectories of p.sp.n_frames, and the pointers of `p` into `base` (every piece starts
// a multiple of 256 bytes from it; null: only the size is wanted).
inline size_t ssens_carve(SmoothSensProblem &p, char *base)
{
    const size_t R = (size_t)p.sp.n_traj * (size_t)p.sp.n_frames;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *at = base ? base + off : nullptr;
        off += (bytes + 255) / 256 * 256;
        return at;
    };
    p.H = (double *)take(8 * (size_t)kSsensTri * R);
    p.P[0] = (double *)take(8 * 49 * R);
    p.P[1] = (double *)take(8 * 49 * R);
    p.Wt = (double *)take(8 * (size_t)kSsensTri * R);
    p.D[0] = (double *)take(8 * 7 * R);
    p.D[1] = (double *)take(8 * 7 * R);
    p.sp.held = (int32_t *)take(4 * R);
    for (int i = 0; i < 4; ++i) p.mark[i] = (int32_t *)take(4 * R);
    return off;
}

// Weights, targets and angles of leg-frame r -> whether it is usable under rule 1 of seqik_refine.h
SEQIK_HD bool ssens_frame_ok(const SmoothSensProblem &p, int64_t r, int leg, double (&w)[4], double (&t)[4][3], double *q)
{
    bool ok = smooth_targets(p.sp.legs[leg], p.pose + r * 15, p.kp_weight ? p.kp_weight + r * 4 : nullptr, w, t);
#pragma unroll
    for (int d = 0; d < 7; ++d) {
        q[d] = p.angles[r * 7 + d];
        ok = ok && angle_in_domain(q[d]);
    }
    return ok;
}

// H (lower triangle) with the rows and columns of held DOFs replaced by the identity's -> the workspace
SEQIK_HD void ssens_store_H(const SmoothSensProblem &p, int64_t r, const double (&H)[7][7], int held)
{
    double *out = p.H + r * kSsensTri;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const bool fi = !((held >> i) & 1);
#pragma unroll
        for (int j = 0; j < i; ++j) out[ssens_tri(i, j)] = (fi && !((held >> j) & 1)) ? H[i][j] : 0.0;
        out[ssens_tri(i, i)] = fi ? H[i][i] : 1.0;
    }
}

// ---- assemble: one item per frame ----
SEQIK_HD void ssens_assemble(const SmoothSensProblem &p, int64_t r)
{
    const double nan = __builtin_nan("");
    const SmoothAt at = smooth_at(p.sp, r);
    const FkLeg &fl = p.sp.legs[at.leg];
    const LegBounds &sb = p.sp.bounds[at.leg];
    double w[4], t[4][3], q[7];
    if (!ssens_frame_ok(p, r, at.leg, w, t, q)) {
        p.sp.held[r] = REFINE_BAD_INPUT;
        if (p.grad) p.grad[r] = nan;
        return;
    }
    JacChain ch;
    double res[4][3], H[7][7], g[7], s[7];
    seq_chain_walk(fl, q, ch);
    refine_residual(ch, t, w, res);
    refsens_hessian(ch, w, res, H, g);
    smooth_stiffness(p.sp, at.leg, s);
#pragma unroll 1
    for (int side = 0; side < 2; ++side) {  // the previous neighbour, then the next
        const int64_t u = side ? r + 1 : r - 1;
        if (side ? at.t + 1 >= p.sp.n_frames : at.t == 0) continue;
        double wu[4], tu[4][3], qu[7];
        if (!ssens_frame_ok(p, u, at.leg, wu, tu, qu)) continue;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            g[j] = g[j] + s[j] * (q[j] - qu[j]);
            H[j][j] = H[j][j] + s[j];
        }
    }
    int32_t held = 0;
    double gmax = 0.0;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const bool h = sens_held(q[j], sb.lb[j], sb.ub[j], g[j], p.tol);
        held |= h ? 1 << j : 0;
        const double a = fabs(g[j]);
        gmax = (!h && a > gmax) ? a : gmax;
    }
    bool sigma_ok = true;
    if (p.kp_sigma) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (w[k] == 0.0) continue;  // not read
            const double sg = p.kp_sigma[r * 4 + k];
            sigma_ok = sigma_ok && is_finite(sg) && sg >= 0.0;
        }
    }
    p.sp.held[r] = held | (sigma_ok ? 0 : SSENS_FLAG_BAD_SIGMA);
    if (p.grad) {
        const double len = ((fl.nseg[0] + fl.nseg[1]) + fl.nseg[2]) + fl.nseg[3];
        const double gr = gmax / (len * len);
        p.grad[r] = gr == gr ? gr : nan;
    }
    ssens_store_H(p, r, H, held);
}

// k of K_t, the pair (r - 1, r) with t the frame of r: s_j where the pair exists and DOF j is held in neither frame, else
// +0.0 -> whether the pair is coupled.  t outside 1..N-1: no pair (nothing is read).
SEQIK_HD bool ssens_coupling(const SmoothSensProblem &p, int64_t r, int64_t t, const double *s, double *k)
{
    const bool pair = t > 0 && t < p.sp.n_frames && smooth_pair(p.sp, r, t);
    const int32_t m = pair ? (p.sp.held[r - 1] | p.sp.held[r]) : 0x7f;
    bool any = false;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        k[j] = ((m >> j) & 1) ? 0.0 : s[j];
        any = any || k[j] != 0.0;
    }
    return any;
}

// S = H_tt of frame r, minus k_i P[i][j] where `in` (lower triangle)
SEQIK_HD void ssens_schur_block(const SmoothSensProblem &p, int64_t r, bool in, const double *k, const double (&P)[7][7],
                                double (&S)[7][7])
{
    const double *H = p.H + r * kSsensTri;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            const double h = H[ssens_tri(i, j)];
            S[i][j] = in ? h - k[i] * P[i][j] : h;
        }
    }
}

// ---- Schur sweep: one item per (trajectory, direction); dir 0 forward (Sf, Pf), 1 backward (Sb, Pb) ----
SEQIK_HD void ssens_schur_sweep(const SmoothSensProblem &p, int64_t traj, int dir)
{
    const int64_t N = p.sp.n_frames;
    double s[7], P[7][7], kin[7], kout[7];
    smooth_stiffness(p.sp, (int)(traj % p.sp.n_legs), s);
#pragma unroll
    for (int i = 0; i < 7; ++i) {
#pragma unroll
        for (int j = 0; j < 7; ++j) P[i][j] = 0.0;
    }
    bool poison = false;
    double *Pout = dir ? p.P[1] : p.P[0];
    int32_t *mark = dir ? p.mark[1] : p.mark[0];
#pragma unroll 1
    for (int64_t n = 0; n < N; ++n) {
        const int64_t t = dir ? N - 1 - n : n, r = traj * N + t;
        if (smooth_bad(p.sp, r)) {
            mark[r] = 0;
            continue;
        }
        // the pair towards the frames already swept, and the pair towards those to come
        const bool in = ssens_coupling(p, r + dir, t + dir, s, kin);
        double M[7][7];
        ssens_schur_block(p, r, in, kin, P, M);
        const bool pd = refsens_factor(M, p.sp.held[r] & 0x7f);
        poison = (in && poison) || !pd;
        mark[r] = poison ? 1 : 0;
        if (ssens_coupling(p, r + 1 - dir, t + 1 - dir, s, kout)) {
#pragma unroll
            for (int c = 0; c < 7; ++c) {
                double y[7];
#pragma unroll
                for (int i = 0; i < 7; ++i) y[i] = i == c ? kout[c] : 0.0;
                smooth_substitute(M, y);
#pragma unroll
                for (int i = 0; i < 7; ++i) {
                    P[i][c] = y[i];
                    Pout[r * 49 + i * 7 + c] = y[i];
                }
            }
        }
    }
}

SEQIK_HD void ssens_load_P(const double *src, bool wanted, double (&P)[7][7])
{
#pragma unroll
    for (int i = 0; i < 7; ++i) {
#pragma unroll
        for (int j = 0; j < 7; ++j) P[i][j] = wanted ? src[i * 7 + j] : 0.0;
    }
}

// ---- combine, first half: the factor of T = (Sf + Sb) - H of a good frame into L, the verdict into mark[0] and flags ->
// whether the frame is NOT poisoned ----
SEQIK_HD bool ssens_verdict(const SmoothSensProblem &p, int64_t r, const SmoothAt &at, double (&L)[7][7])
{
    double s[7], k[7], P[7][7], Sb[7][7];
    smooth_stiffness(p.sp, at.leg, s);
    const bool inf = ssens_coupling(p, r, at.t, s, k);
    ssens_load_P(p.P[0] + (inf ? r - 1 : r) * 49, inf, P);
    ssens_schur_block(p, r, inf, k, P, L);
    const bool inb = ssens_coupling(p, r + 1, at.t + 1, s, k);
    ssens_load_P(p.P[1] + (inb ? r + 1 : r) * 49, inb, P);
    ssens_schur_block(p, r, inb, k, P, Sb);
    const double *H = p.H + r * kSsensTri;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) L[i][j] = (L[i][j] + Sb[i][j]) - H[ssens_tri(i, j)];
    }
    const int32_t word = p.sp.held[r];
    const bool pd = refsens_factor(L, word & 0x7f);
    const bool ok = pd && !p.mark[0][r] && !p.mark[1][r];
    p.mark[0][r] = ok ? 0 : 1;  // from here on: the frame's verdict (this item alone reads and writes the word)
    if (p.flags) p.flags[r] = word | (ok ? 0 : SSENS_FLAG_NOT_PD);
    return ok;
}

// The right-hand sides of the rule: b of key point K0 + 1 from the chain (refsens_rhs of seqik_refine_sens.hpp)
struct SsensChainRhs {
    const JacChain &ch;
    const double *w;
    int held;
    template <int K0, int... D> SEQIK_HD void fill_dofs(double (&b)[7][3], std::integer_sequence<int, D...>) const
    {
        (refsens_rhs<K0, D>(ch, w[K0], held, b), ...);
    }
    template <int K0> SEQIK_HD void fill(double (&b)[7][3]) const { fill_dofs<K0>(b, std::make_integer_sequence<int, 7>{}); }
};

// The three columns of key point K0 + 1 of the centre block: solve, select, their share of acc
template <int K0, class Rhs>
SEQIK_HD void ssens_key_point(const Rhs &rhs, double w, const double (&L)[7][7], int held, bool ok, double sig2,
                              double (&rec)[7][4][3], double (&acc)[7])
{
    const double nan = __builtin_nan("");
    double b[7][3];
    rhs.template fill<K0>(b);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double y[7];
#pragma unroll
        for (int i = 0; i < 7; ++i) y[i] = b[i][c];
        smooth_substitute(L, y);
#pragma unroll
        for (int i = 0; i < 7; ++i) b[i][c] = y[i];
    }
#pragma unroll
    for (int d = 0; d < 7; ++d) {
        const bool h = (held >> d) & 1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double x = b[d][c];
            b[d][c] = h ? 0.0 : !ok ? nan : w == 0.0 ? 0.0 : x == x ? x : nan;
            rec[d][K0][c] = b[d][c];
        }
        const double t = sig2 * ((b[d][0] * b[d][0] + b[d][1] * b[d][1]) + b[d][2] * b[d][2]);
        acc[d] = K0 == 0 ? t : acc[d] + t;
    }
}

// ---- combine, second half: the centre block of a good frame, own (parked in std) and Wt ----
template <class Rhs>
SEQIK_HD void ssens_centre(const SmoothSensProblem &p, int64_t r, const double (&L)[7][7], bool ok, const Rhs &rhs,
                           const double *w)
{
    const int held = p.sp.held[r] & 0x7f;
    double sg2[4], rec[7][4][3], acc[7];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double sg = 0.0;
        if (p.kp_sigma && w[k] != 0.0) sg = p.kp_sigma[r * 4 + k];  // the sigma of a key point without weight is not read
        sg2[k] = sg * sg;
    }
    ssens_key_point<0>(rhs, w[0], L, held, ok, sg2[0], rec, acc);
    ssens_key_point<1>(rhs, w[1], L, held, ok, sg2[1], rec, acc);
    ssens_key_point<2>(rhs, w[2], L, held, ok, sg2[2], rec, acc);
    ssens_key_point<3>(rhs, w[3], L, held, ok, sg2[3], rec, acc);
    if (p.sens) {
        double *out = p.sens + (r * (2 * (int64_t)p.half_width + 1) + p.half_width) * kSensRow;
#pragma unroll
        for (int d = 0; d < 7; ++d) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
#pragma unroll
                for (int c = 0; c < 3; ++c) out[12 * d + 3 * k + c] = rec[d][k][c];
            }
        }
    }
    if (p.std_out) {
#pragma unroll
        for (int d = 0; d < 7; ++d) p.std_out[r * 7 + d] = acc[d];
        double *Wt = p.Wt + r * kSsensTri;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                double v = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double t = sg2[k] * ((rec[i][k][0] * rec[j][k][0] + rec[i][k][1] * rec[j][k][1]) + rec[i][k][2] * rec[j][k][2]);
                    v = k == 0 ? t : v + t;
                }
                Wt[ssens_tri(i, j)] = v;
            }
        }
    }
}

// what combine leaves for a bad frame: the centre block NaN, flags bit 16 alone (std: finish)
SEQIK_HD void ssens_combine_bad(const SmoothSensProblem &p, int64_t r)
{
    const double nan = __builtin_nan("");
    if (p.flags) p.flags[r] = SSENS_FLAG_BAD_INPUT;
    if (p.sens) {
        double *out = p.sens + (r * (2 * (int64_t)p.half_width + 1) + p.half_width) * kSensRow;
        for (int i = 0; i < kSensRow; ++i) out[i] = nan;
    }
}

// ---- combine: one item per frame ----
SEQIK_HD void ssens_combine(const SmoothSensProblem &p, int64_t r)
{
    if (smooth_bad(p.sp, r)) {
        ssens_combine_bad(p, r);
        return;
    }
    const SmoothAt at = smooth_at(p.sp, r);
    double L[7][7];
    const bool ok = ssens_verdict(p, r, at, L);
    if (!p.sens && !p.std_out) return;  // only the verdict was wanted
    double w[4], t[4][3], q[7];
    ssens_frame_ok(p, r, at.leg, w, t, q);
    JacChain ch;
    seq_chain_walk(p.sp.legs[at.leg], q, ch);
    const SsensChainRhs rhs{ch, w, p.sp.held[r] & 0x7f};
    ssens_centre(p, r, L, ok, rhs, w);
}

// ---- covariance sweep: one item per (trajectory, direction); dir 0 forward (Lam, with Pb), 1 backward (Ups, with Pf) ----
SEQIK_HD void ssens_cov_sweep(const SmoothSensProblem &p, int64_t traj, int dir)
{
    const int64_t N = p.sp.n_frames;
    double s[7], k[7], X[7][7];
    smooth_stiffness(p.sp, (int)(traj % p.sp.n_legs), s);
#pragma unroll
    for (int i = 0; i < 7; ++i) {
#pragma unroll
        for (int j = 0; j < 7; ++j) X[i][j] = 0.0;
    }
    bool sick = false;
    const double *Pin = dir ? p.P[0] : p.P[1];
    double *D = dir ? p.D[1] : p.D[0];
    int32_t *mark = dir ? p.mark[3] : p.mark[2];
#pragma unroll 1
    for (int64_t n = 0; n < N; ++n) {
        const int64_t t = dir ? N - 1 - n : n, r = traj * N + t;
        if (smooth_bad(p.sp, r)) {
            mark[r] = 0;
            continue;
        }
        if (ssens_coupling(p, r + dir, t + dir, s, k)) {
            const int64_t u = dir ? r + 1 : r - 1;  // the frame swept before this one
            sick = sick || p.mark[0][u] || (p.sp.held[u] & SSENS_FLAG_BAD_SIGMA) != 0;
            const double *Wt = p.Wt + u * kSsensTri;
#pragma unroll
            for (int i = 0; i < 7; ++i) {
#pragma unroll
                for (int j = 0; j <= i; ++j) {
                    X[i][j] = X[i][j] + Wt[ssens_tri(i, j)];
                    X[j][i] = X[i][j];
                }
            }
            double P[7][7], T[7][7];
            ssens_load_P(Pin + r * 49, true, P);
#pragma unroll
            for (int i = 0; i < 7; ++i) {
#pragma unroll
                for (int c = 0; c < 7; ++c) T[i][c] = smooth_dot7(P[i], X[c]);  // X is symmetric: row c is column c
            }
#pragma unroll
            for (int i = 0; i < 7; ++i) {
#pragma unroll
                for (int j = 0; j <= i; ++j) {
                    X[i][j] = smooth_dot7(T[i], P[j]);
                    X[j][i] = X[i][j];
                }
            }
        } else {
            sick = false;
#pragma unroll
            for (int i = 0; i < 7; ++i) {
#pragma unroll
                for (int j = 0; j < 7; ++j) X[i][j] = 0.0;
            }
        }
        mark[r] = sick ? 1 : 0;
#pragma unroll
        for (int j = 0; j < 7; ++j) D[r * 7 + j] = X[j][j];
    }
}

// The off-centre blocks of frame r on one side: side 0 the sources t - m (Pb), side 1 the sources t + m (Pf), m = 1..W
SEQIK_HD void ssens_side_blocks(const SmoothSensProblem &p, int64_t r, const SmoothAt &at, int side)
{
    const double nan = __builtin_nan("");
    const int64_t N = p.sp.n_frames, W = p.half_width, step = side ? 1 : -1;
    const int32_t word = p.sp.held[r];
    const bool bad = smooth_bad(p.sp, r), poisoned = p.mark[0][r] != 0;
    const double *Pin = side ? p.P[0] : p.P[1];
    double s[7], k[7], Q[7][7];
    smooth_stiffness(p.sp, at.leg, s);
#pragma unroll
    for (int i = 0; i < 7; ++i) {
#pragma unroll
        for (int j = 0; j < 7; ++j) Q[i][j] = 0.0;
    }
    bool cut = false;
#pragma unroll 1
    for (int64_t m = 1; m <= W; ++m) {
        const int64_t ts = at.t + step * m, rs = r + step * m;
        double *out = p.sens + (r * (2 * W + 1) + W + step * m) * kSensRow;
        const bool inside = ts >= 0 && ts < N;
        if (inside && !bad && !cut) {
            // the pair between the source and the frame before it on the way from t, and the P of that frame
            const int64_t rp = rs - step;  // m == 1: r
            if (!ssens_coupling(p, side ? rs : rp, side ? ts : ts + 1, s, k)) {
                cut = true;
            } else {
                const double *P = Pin + rp * 49;
                if (m == 1) {
                    ssens_load_P(P, true, Q);
                } else {
                    double Qn[7][7];
#pragma unroll
                    for (int c = 0; c < 7; ++c) {
                        double col[7];
#pragma unroll
                        for (int j = 0; j < 7; ++j) col[j] = P[j * 7 + c];
#pragma unroll
                        for (int i = 0; i < 7; ++i) Qn[i][c] = smooth_dot7(Q[i], col);
                    }
#pragma unroll
                    for (int i = 0; i < 7; ++i) {
#pragma unroll
                        for (int c = 0; c < 7; ++c) Q[i][c] = Qn[i][c];
                    }
                }
            }
        }
        if (!inside || (!bad && cut)) {
            for (int i = 0; i < kSensRow; ++i) out[i] = 0.0;
        } else if (bad) {
            for (int i = 0; i < kSensRow; ++i) out[i] = nan;
        } else {
            const double *src = p.sens + (rs * (2 * W + 1) + W) * kSensRow;  // sens0 of the source frame
#pragma unroll 1
            for (int kc = 0; kc < 12; ++kc) {
                const double ws = p.kp_weight ? p.kp_weight[rs * 4 + kc / 3] : 1.0;
                double col[7];
#pragma unroll
                for (int j = 0; j < 7; ++j) col[j] = src[j * 12 + kc];
#pragma unroll
                for (int i = 0; i < 7; ++i) {
                    const double v = smooth_dot7(Q[i], col);
                    out[i * 12 + kc] = ((word >> i) & 1) ? 0.0 : poisoned ? nan : ws == 0.0 ? 0.0 : v == v ? v : nan;
                }
            }
        }
    }
}

// ---- finish: one item per frame ----
SEQIK_HD void ssens_finish(const SmoothSensProblem &p, int64_t r)
{
    const double nan = __builtin_nan("");
    const SmoothAt at = smooth_at(p.sp, r);
    if (p.std_out) {
        const int32_t word = p.sp.held[r];
        const bool bad = smooth_bad(p.sp, r);
        const bool sick = bad || p.mark[0][r] || p.mark[2][r] || p.mark[3][r] || (word & SSENS_FLAG_BAD_SIGMA) != 0;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            double v = nan;
            if (!sick) {
                const double sd = sqrt(p.std_out[r * 7 + j] + (p.D[0][r * 7 + j] + p.D[1][r * 7 + j]));
                v = sd == sd ? sd : nan;
            }
            p.std_out[r * 7 + j] = (!bad && ((word >> j) & 1)) ? 0.0 : v;
        }
    }
    if (p.sens && p.half_width > 0) {
        ssens_side_blocks(p, r, at, 0);
        ssens_side_blocks(p, r, at, 1);
    }
}

// which phases a request runs: a request without sens and std ends with the verdict; one for grad alone with assemble
SEQIK_HD bool ssens_wants_verdict(const SmoothSensProblem &p) { return p.sens || p.std_out || p.flags; }
SEQIK_HD bool ssens_wants_cov(const SmoothSensProblem &p) { return p.std_out != nullptr; }
SEQIK_HD bool ssens_wants_finish(const SmoothSensProblem &p) { return p.std_out || (p.sens && p.half_width > 0); }

// ------------------------------------------------ the rule run on the host ------------------------------------------------
inline void ssens_run_host(const SmoothSensProblem &p)
{
    const int64_t R = p.sp.n_traj * p.sp.n_frames;
    for (int64_t r = 0; r < R; ++r) ssens_assemble(p, r);
    if (!ssens_wants_verdict(p)) return;
    for (int64_t i = 0; i < 2 * p.sp.n_traj; ++i) ssens_schur_sweep(p, i >> 1, (int)(i & 1));
    for (int64_t r = 0; r < R; ++r) ssens_combine(p, r);
    if (ssens_wants_cov(p))
        for (int64_t i = 0; i < 2 * p.sp.n_traj; ++i) ssens_cov_sweep(p, i >> 1, (int)(i & 1));
    if (ssens_wants_finish(p))
        for (int64_t r = 0; r < R; ++r) ssens_finish(p, r);
}

}  // namespace seqik
