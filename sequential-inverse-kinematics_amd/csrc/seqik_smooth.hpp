// seqik_smooth.hpp -- trajectory refinement (include/seqik_smooth.h): the device rule, host-runnable.
//
// A trajectory is one (sequence, leg) pair, frames t = 0..N-1.  One bounded Levenberg-Marquardt per trajectory minimises
//     C(Q) = sum_t c_t(q_t) + sum_pairs sum_j s_j (q_{t,j} - q_{t-1,j})^2,   s_j = smooth[j] * len^2,
// c_t the data term of seqik_refine.hpp, a pair (t-1, t) existing where both frames are good.  The header states the rule;
// this file fixes its arithmetic.  The rule is cut into PHASES, each a function of one work item (a frame, a (frame,
// column) pair or a trajectory) that reads only what earlier phases stored in the workspace: the kernels of
// seqik_smooth.hip run one phase per launch over all items, smooth_run_host below runs the same functions in loops, and
// the two agree bit for bit (-ffp-contract=off, correctly rounded sqrt and /; the only values items of one phase combine
// are flag bits, by OR).
//
//   init       q = clamp(angles); a frame that is bad under rule 1 of seqik_refine.h is marked and takes no part
//   cost       e_t = c_t(x_t), then for j ascending e_t = e_t + s_j * (d_j * d_j), d_j = x_{t,j} - x_{t-1,j} (pair only);
//              0 for a bad frame.  C = the sum of e_0..e_{P-1} over the aligned binary tree, P the power of two >= N,
//              e_N.. = +0.0: level by level e[2 i m] = e[2 i m] + e[2 i m + m], m = 1, 2, 4, ...
//   assemble   A, g of refine_normal_equations at q_t; then for u = t - 1 and then u = t + 1, where that pair exists, for j
//              ascending g_j = g_j + s_j * (q_{t,j} - q_{u,j}) and A_jj = A_jj + s_j.  held as in seqik_refine.hpp on this g.
//   stop       7n's tests on the whole trajectory, in 7n's order
//   setup      row t of the block-tridiagonal system: D = A + lambda diag(d) (d_j = A_jj, <= 0 replaced by DBL_MIN), L =
//              -diag(s) where the pair (t-1, t) exists, U = -diag(s) where (t, t+1) exists, b = -g; a held DOF's row and
//              column of D are the identity's, its entry of b and every entry of L and U that couples it are 0 (an entry
//              of L couples DOF j of t with DOF j of t - 1: it stays only when both are free); a bad frame is an identity
//              row.  Only the lower triangle of D is stored or read, at every stride.
//   normalise  Cholesky of D_u in refine_solve's order; EL = D^-1 L, EU = D^-1 U column by column, eb = D^-1 b, each by
//              refine_solve's forward and back substitution
//   reduce     stride h: D'[i][c] = (D[i][c] - sum_k L[i][k] EU_{t-h}[k][c]) - sum_k U[i][k] EL_{t+h}[k][c],
//              L'[i][c] = -(sum_k L[i][k] EL_{t-h}[k][c]),  U'[i][c] = -(sum_k U[i][k] EU_{t+h}[k][c]),
//              b'[i] = (b[i] - sum_k L[i][k] eb_{t-h}[k]) - sum_k U[i][k] eb_{t+h}[k];  every sum is p_0, then + p_1, ... + p_6;
//              a neighbour outside 0..N-1: that term is left out and that L' or U' is 0.  Rows are double-buffered.
//   final      delta_t = D_t^-1 b_t by the same factorisation.  A pivot that is not positive, anywhere: the trial is unusable.
//   trial      q'_t = q_t on held DOFs, clamp(q_t + delta_t) on the others; e_t as above at q' (frame t forms q'_{t-1}
//              itself); an angle outside the domain makes the trial unusable
//   decide     C' by the tree; accept, stall, or damp as seqik_refine.hpp does, once per trajectory
//   finish     angles_out, frame_info, cost, info
//
// Work split of setup, normalise and reduce: eight items per row, item c < 7 owns column c of the 7 x 7 blocks, item 7 the
// right-hand side.  A lane holding four blocks does not fit the register file without spilling; a column of each does.
#pragma once
#include <stdint.h>

#include "seqik_refine.hpp"

namespace seqik {

constexpr int kSmoothRow = 154;       // doubles of a row of the system: D 49, L 49, U 49, b 7
constexpr int kSmoothNorm = 105;      // doubles of a normalised row: EL 49, EU 49, eb 7
constexpr int kSmoothLanes = 8;       // work items per row in setup, normalise and reduce
constexpr int32_t SMOOTH_ASSEMBLE = 0, SMOOTH_TRIAL = 1, SMOOTH_STOPPED = 2;  // SmoothTraj::status
constexpr int32_t SMOOTH_LARGE = 1, SMOOTH_UNUSABLE = 2, SMOOTH_MOVED = 4;    // SmoothTraj::flags

struct SmoothOptions {
    double smooth[7];
    double gtol, ftol;
    int32_t max_iter, pad_;
};

struct SmoothTraj {
    double lambda, cost, cost0;
    int32_t iters, rejects, reason, status, flags, last;
};

// Doubles of workspace per leg-frame besides e: q, qn, g, delta (7 each), A (49), two row buffers, the normalised rows.
constexpr int kSmoothFrameDoubles = 4 * 7 + 49 + 2 * kSmoothRow + kSmoothNorm;

struct SmoothProblem {
    const double *angles;     // [R][7], R = n_traj * n_frames
    const double *pose;       // [R][5][3]
    const double *kp_weight;  // nullable, [R][4]
    double *angles_out;       // [R][7]; may be `angles`
    int32_t *frame_info;      // nullable, [R]
    double *cost;             // nullable, [n_traj][2]
    int32_t *info;            // nullable, [n_traj][3]
    // the workspace
    double *q, *qn, *g, *delta;  // [R][7]
    double *A;                   // [R][49], lower triangle
    double *rows[2];             // [R][kSmoothRow]
    double *E;                   // [R][kSmoothNorm]
    double *e;                   // [n_traj][n_pad]
    SmoothTraj *traj;            // [n_traj]
    int32_t *held;               // [R]: bits 0..6 held, REFINE_BAD_INPUT
    int32_t *active;             // [1]: trajectories still running, counted by the stop phase
    int64_t n_frames, n_traj, n_pad;
    int32_t n_legs, pad_;
    SmoothOptions opt;
    FkLeg legs[kFkMaxLegs];
    LegBounds bounds[kFkMaxLegs];
};

// the power of two >= n (n >= 1)
inline int64_t smooth_pad(int64_t n)
{
    int64_t p = 1;
    while (p < n) p *= 2;
    return p;
}

// Bytes of workspace for n_traj trajectories of n_frames, and the pointers of `p` into `base` (every piece starts a
// multiple of 256 bytes from it; null: only the size is wanted).
inline size_t smooth_carve(SmoothProblem &p, char *base)
{
    const size_t R = (size_t)p.n_traj * (size_t)p.n_frames, T = (size_t)p.n_traj;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *at = base ? base + off : nullptr;
        off += (bytes + 255) / 256 * 256;
        return at;
    };
    p.q = (double *)take(8 * 7 * R);
    p.qn = (double *)take(8 * 7 * R);
    p.g = (double *)take(8 * 7 * R);
    p.delta = (double *)take(8 * 7 * R);
    p.A = (double *)take(8 * 49 * R);
    p.rows[0] = (double *)take(8 * (size_t)kSmoothRow * R);
    p.rows[1] = (double *)take(8 * (size_t)kSmoothRow * R);
    p.E = (double *)take(8 * (size_t)kSmoothNorm * R);
    p.e = (double *)take(8 * T * (size_t)p.n_pad);
    p.traj = (SmoothTraj *)take(sizeof(SmoothTraj) * T);
    p.held = (int32_t *)take(4 * R);
    p.active = (int32_t *)take(4);
    return off;
}

SEQIK_HD void smooth_flag(int32_t *flags, int32_t bits)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(flags, bits);
#else
    *flags |= bits;
#endif
}

struct SmoothAt {
    int64_t traj, t;
    int leg;
};

SEQIK_HD SmoothAt smooth_at(const SmoothProblem &p, int64_t r)
{
    SmoothAt a;
    a.traj = r / p.n_frames;
    a.t = r - a.traj * p.n_frames;
    a.leg = (int)(a.traj % p.n_legs);
    return a;
}

SEQIK_HD bool smooth_bad(const SmoothProblem &p, int64_t r) { return (p.held[r] & REFINE_BAD_INPUT) != 0; }

// whether the pair (r - 1, r) exists; `t` the frame of r
SEQIK_HD bool smooth_pair(const SmoothProblem &p, int64_t r, int64_t t) { return t > 0 && !smooth_bad(p, r - 1) && !smooth_bad(p, r); }

SEQIK_HD void smooth_stiffness(const SmoothProblem &p, int leg, double *s)
{
    const FkLeg &fl = p.legs[leg];
    const double len = ((fl.nseg[0] + fl.nseg[1]) + fl.nseg[2]) + fl.nseg[3];
    const double len2 = len * len;
#pragma unroll
    for (int j = 0; j < 7; ++j) s[j] = p.opt.smooth[j] * len2;
}

// Weights and targets of a leg-frame as refine_leg_frame reads them -> whether they are usable under rule 1.
SEQIK_HD bool smooth_targets(const FkLeg &fl, const double *pose, const double *kp_weight, double (&w)[4], double (&t)[4][3])
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        w[k] = kp_weight ? kp_weight[k] : 1.0;
        ok = ok && is_finite(fl.nseg[k]) && is_finite(w[k]) && w[k] >= 0.0;
    }
    double o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o[c] = pose[c];
        ok = ok && is_finite(o[c]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double v = 0.0;
            if (w[k] != 0.0) {  // a key point without weight is not read
                v = pose[3 * (k + 1) + c];
                ok = ok && is_finite(v);
                v = v - o[c];
            }
            t[k][c] = v;
        }
    }
    return ok;
}

// ---- init: one item per frame ----
SEQIK_HD void smooth_init(const SmoothProblem &p, int64_t r)
{
    const SmoothAt at = smooth_at(p, r);
    const LegBounds &sb = p.bounds[at.leg];
    double w[4], t[4][3], q[7];
    bool ok = smooth_targets(p.legs[at.leg], p.pose + r * 15, p.kp_weight ? p.kp_weight + r * 4 : nullptr, w, t);
#pragma unroll
    for (int d = 0; d < 7; ++d) {
        q[d] = p.angles[r * 7 + d];
        ok = ok && angle_in_domain(q[d]);
    }
#pragma unroll
    for (int d = 0; d < 7; ++d) p.q[r * 7 + d] = ok ? refine_clamp(q[d], sb.lb[d], sb.ub[d]) : 0.0;
    p.held[r] = ok ? 0 : REFINE_BAD_INPUT;
    if (p.n_frames + at.t < p.n_pad) p.e[at.traj * p.n_pad + p.n_frames + at.t] = 0.0;  // the padding of the tree (n_pad < 2 N)
    if (at.t == 0) {
        SmoothTraj &tr = p.traj[at.traj];
        tr.lambda = kRefineLambda0;
        tr.cost = tr.cost0 = 0.0;
        tr.iters = tr.rejects = tr.reason = tr.flags = tr.last = 0;
        tr.status = SMOOTH_ASSEMBLE;
    }
}

// ---- cost of frame r at the angles x, its previous neighbour at xp (read only where the pair exists) ----
SEQIK_HD double smooth_frame_cost(const SmoothProblem &p, int64_t r, const SmoothAt &at, const double *x, const double *xp)
{
    double w[4], t[4][3], res[4][3];
    smooth_targets(p.legs[at.leg], p.pose + r * 15, p.kp_weight ? p.kp_weight + r * 4 : nullptr, w, t);
    JacChain ch;
    seq_chain_walk(p.legs[at.leg], x, ch);
    double e = refine_residual(ch, t, w, res);
    if (smooth_pair(p, r, at.t)) {
        double s[7];
        smooth_stiffness(p, at.leg, s);
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const double d = x[j] - xp[j];
            e = e + s[j] * (d * d);
        }
    }
    return e;
}

// the starting cost's e_t: one item per frame
SEQIK_HD void smooth_start_cost(const SmoothProblem &p, int64_t r)
{
    const SmoothAt at = smooth_at(p, r);
    double e = 0.0;
    if (!smooth_bad(p, r)) {
        double x[7], xp[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            x[j] = p.q[r * 7 + j];
            xp[j] = at.t > 0 ? p.q[(r - 1) * 7 + j] : 0.0;
        }
        e = smooth_frame_cost(p, r, at, x, xp);
    }
    p.e[at.traj * p.n_pad + at.t] = e;
}

// ---- the tree: level m of trajectory `traj`, item i < n_pad / (2 m) ----
SEQIK_HD void smooth_tree_add(const SmoothProblem &p, int64_t traj, int64_t m, int64_t i)
{
    double *e = p.e + traj * p.n_pad;
    e[2 * i * m] = e[2 * i * m] + e[2 * i * m + m];
}

// ---- assemble: one item per frame of a trajectory that stands at a new point ----
SEQIK_HD void smooth_assemble(const SmoothProblem &p, int64_t r)
{
    const SmoothAt at = smooth_at(p, r);
    if (p.traj[at.traj].status != SMOOTH_ASSEMBLE || smooth_bad(p, r)) return;
    const LegBounds &sb = p.bounds[at.leg];
    const FkLeg &fl = p.legs[at.leg];
    double w[4], t[4][3], res[4][3], q[7], A[7][7], g[7], s[7];
    smooth_targets(fl, p.pose + r * 15, p.kp_weight ? p.kp_weight + r * 4 : nullptr, w, t);
#pragma unroll
    for (int j = 0; j < 7; ++j) q[j] = p.q[r * 7 + j];
    JacChain ch;
    seq_chain_walk(fl, q, ch);
    refine_residual(ch, t, w, res);
    refine_normal_equations(ch, w, res, A, g);
    smooth_stiffness(p, at.leg, s);
    if (smooth_pair(p, r, at.t)) {
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            g[j] = g[j] + s[j] * (q[j] - p.q[(r - 1) * 7 + j]);
            A[j][j] = A[j][j] + s[j];
        }
    }
    if (at.t + 1 < p.n_frames && smooth_pair(p, r + 1, at.t + 1)) {
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            g[j] = g[j] + s[j] * (q[j] - p.q[(r + 1) * 7 + j]);
            A[j][j] = A[j][j] + s[j];
        }
    }
    const double len = ((fl.nseg[0] + fl.nseg[1]) + fl.nseg[2]) + fl.nseg[3];
    const double gbar = p.opt.gtol * (len * len);
    int32_t held = 0;
    bool small = true;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const bool h = (q[j] <= sb.lb[j] && g[j] > 0.0) || (q[j] >= sb.ub[j] && g[j] < 0.0);
        held |= h ? 1 << j : 0;
        small = small && (h || fabs(g[j]) <= gbar);
        p.g[r * 7 + j] = g[j];
#pragma unroll
        for (int i = 0; i <= j; ++i) p.A[r * 49 + j * 7 + i] = A[j][i];
    }
    p.held[r] = held;
    if (!small) smooth_flag(&p.traj[at.traj].flags, SMOOTH_LARGE);
}

// ---- stop: one item per trajectory; counts the trajectories that go on ----
SEQIK_HD void smooth_stop(const SmoothProblem &p, int64_t traj)
{
    SmoothTraj &tr = p.traj[traj];
    if (tr.status == SMOOTH_STOPPED) return;
    if (tr.status == SMOOTH_ASSEMBLE) {
        tr.status = SMOOTH_TRIAL;
        if (tr.last) {
            tr.reason = REFINE_STOP_DECREASE;
            tr.status = SMOOTH_STOPPED;
        } else if (tr.iters >= p.opt.max_iter) {
            tr.reason = REFINE_STOP_MAX_ITER;
            tr.status = SMOOTH_STOPPED;
        } else if (!(tr.flags & SMOOTH_LARGE)) {
            tr.reason = REFINE_STOP_GRADIENT;
            tr.status = SMOOTH_STOPPED;
        }
    }
    tr.flags = 0;
    if (tr.status != SMOOTH_STOPPED) {
#if defined(__HIP_DEVICE_COMPILE__)
        atomicAdd(p.active, 1);
#else
        *p.active += 1;
#endif
    }
}

// ---- setup: item (r, c) ----
SEQIK_HD void smooth_setup(const SmoothProblem &p, int64_t r, int c)
{
    const SmoothAt at = smooth_at(p, r);
    if (p.traj[at.traj].status != SMOOTH_TRIAL) return;
    double *row = p.rows[0] + r * kSmoothRow;
    const bool bad = smooth_bad(p, r);
    const int32_t held = p.held[r];
    if (c == 7) {
#pragma unroll
        for (int i = 0; i < 7; ++i) row[147 + i] = (bad || ((held >> i) & 1)) ? 0.0 : -p.g[r * 7 + i];
        return;
    }
    const bool free_c = !bad && !((held >> c) & 1);
    const double lambda = p.traj[at.traj].lambda;
    double s[7];
    smooth_stiffness(p, at.leg, s);
    double sc = s[0];
#pragma unroll
    for (int j = 1; j < 7; ++j) sc = c == j ? s[j] : sc;
    const bool lower = free_c && smooth_pair(p, r, at.t) && !((p.held[at.t > 0 ? r - 1 : r] >> c) & 1);
    const bool next = at.t + 1 < p.n_frames;
    const bool upper = free_c && next && smooth_pair(p, r + 1, at.t + 1) && !((p.held[next ? r + 1 : r] >> c) & 1);
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        row[49 + i * 7 + c] = (i == c && lower) ? -sc : 0.0;
        row[98 + i * 7 + c] = (i == c && upper) ? -sc : 0.0;
        if (i == c) {
            double v = 1.0;
            if (free_c) {
                const double a = p.A[r * 49 + c * 7 + c];
                const double d = a <= 0.0 ? kRefineTiny : a;
                v = a + lambda * d;
            }
            row[i * 7 + c] = v;
        } else if (i > c) {
            row[i * 7 + c] = (free_c && !((held >> i) & 1)) ? p.A[r * 49 + i * 7 + c] : 0.0;
        }
    }
}

// Cholesky of the lower triangle of M in place, refine_solve's order -> whether every pivot was positive
SEQIK_HD bool smooth_cholesky(double (&M)[7][7])
{
    bool pd = true;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        double s = M[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s = s - M[j][k] * M[j][k];
        pd = pd && (s > 0.0);
        const double l = sqrt(s);
        M[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < 7; ++i) {
            double v = M[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v = v - M[i][k] * M[j][k];
            M[i][j] = v / l;
        }
    }
    return pd;
}

// x = (M M^T)^-1 y, in place in y, refine_solve's substitutions
SEQIK_HD void smooth_substitute(const double (&M)[7][7], double *y)
{
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        double v = y[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v = v - M[i][k] * y[k];
        y[i] = v / M[i][i];
    }
#pragma unroll
    for (int i = 6; i >= 0; --i) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < 7; ++k) v = v - M[k][i] * y[k];
        y[i] = v / M[i][i];
    }
}

// the lower triangle of D of `row` factorised into M -> whether every pivot was positive
SEQIK_HD bool smooth_factor(const double *row, double (&M)[7][7])
{
#pragma unroll
    for (int i = 0; i < 7; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) M[i][j] = row[i * 7 + j];
    }
    return smooth_cholesky(M);
}

// ---- normalise: item (r, c) ----
SEQIK_HD void smooth_normalise(const SmoothProblem &p, int64_t r, int c, int cur)
{
    const int64_t traj = r / p.n_frames;
    if (p.traj[traj].status != SMOOTH_TRIAL) return;
    const double *row = p.rows[cur] + r * kSmoothRow;
    double *E = p.E + r * kSmoothNorm;
    double M[7][7], y[7];
    const bool pd = smooth_factor(row, M);
    if (c == 7) {
        if (!pd) smooth_flag(&p.traj[traj].flags, SMOOTH_UNUSABLE);
#pragma unroll
        for (int i = 0; i < 7; ++i) y[i] = row[147 + i];
        smooth_substitute(M, y);
#pragma unroll
        for (int i = 0; i < 7; ++i) E[98 + i] = y[i];
        return;
    }
#pragma unroll 1
    for (int which = 0; which < 2; ++which) {  // EL, then EU
#pragma unroll
        for (int i = 0; i < 7; ++i) y[i] = row[49 + 49 * which + i * 7 + c];
        smooth_substitute(M, y);
#pragma unroll
        for (int i = 0; i < 7; ++i) E[49 * which + i * 7 + c] = y[i];
    }
}

// p_0, then + p_1, ... + p_6 of x[k] * y[k]
SEQIK_HD double smooth_dot7(const double *x, const double *y)
{
    double s = x[0] * y[0];
#pragma unroll
    for (int k = 1; k < 7; ++k) s = s + x[k] * y[k];
    return s;
}

// ---- reduce at stride h: item (r, c), rows[cur] -> rows[cur ^ 1] ----
SEQIK_HD void smooth_reduce(const SmoothProblem &p, int64_t r, int c, int64_t h, int cur)
{
    const SmoothAt at = smooth_at(p, r);
    if (p.traj[at.traj].status != SMOOTH_TRIAL) return;
    const double *row = p.rows[cur] + r * kSmoothRow;
    double *out = p.rows[cur ^ 1] + r * kSmoothRow;
    const bool has_m = at.t - h >= 0, has_p = at.t + h < p.n_frames;
    const double *Em = p.E + (has_m ? r - h : r) * kSmoothNorm, *Ep = p.E + (has_p ? r + h : r) * kSmoothNorm;
    if (c == 7) {
        double bm[7], bp[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            bm[k] = Em[98 + k];
            bp[k] = Ep[98 + k];
        }
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            double li[7], ui[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                li[k] = row[49 + i * 7 + k];
                ui[k] = row[98 + i * 7 + k];
            }
            double v = row[147 + i];
            const double lm = smooth_dot7(li, bm), up = smooth_dot7(ui, bp);
            v = has_m ? v - lm : v;
            v = has_p ? v - up : v;
            out[147 + i] = v;
        }
        return;
    }
    double elm[7], eum[7], elp[7], eup[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        elm[k] = Em[k * 7 + c];
        eum[k] = Em[49 + k * 7 + c];
        elp[k] = Ep[k * 7 + c];
        eup[k] = Ep[49 + k * 7 + c];
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        double li[7], ui[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            li[k] = row[49 + i * 7 + k];
            ui[k] = row[98 + i * 7 + k];
        }
        const double l_el = smooth_dot7(li, elm), u_eu = smooth_dot7(ui, eup);
        out[49 + i * 7 + c] = has_m ? -l_el : 0.0;
        out[98 + i * 7 + c] = has_p ? -u_eu : 0.0;
        if (i >= c) {
            const double l_eu = smooth_dot7(li, eum), u_el = smooth_dot7(ui, elp);
            double d = row[i * 7 + c];
            d = has_m ? d - l_eu : d;
            d = has_p ? d - u_el : d;
            out[i * 7 + c] = d;
        }
    }
}

// ---- final: one item per frame, delta = D^-1 b of rows[cur] ----
SEQIK_HD void smooth_final(const SmoothProblem &p, int64_t r, int cur)
{
    const int64_t traj = r / p.n_frames;
    if (p.traj[traj].status != SMOOTH_TRIAL) return;
    const double *row = p.rows[cur] + r * kSmoothRow;
    double M[7][7], y[7];
    if (!smooth_factor(row, M)) smooth_flag(&p.traj[traj].flags, SMOOTH_UNUSABLE);
#pragma unroll
    for (int i = 0; i < 7; ++i) y[i] = row[147 + i];
    smooth_substitute(M, y);
#pragma unroll
    for (int i = 0; i < 7; ++i) p.delta[r * 7 + i] = y[i];
}

// the trial point of frame r into x -> bit 0: every angle inside the domain, bit 1: it differs from q
SEQIK_HD int smooth_trial_point(const SmoothProblem &p, int64_t r, int leg, double *x)
{
    const LegBounds &sb = p.bounds[leg];
    const int32_t held = p.held[r];
    bool usable = true, moved = false;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const double q = p.q[r * 7 + j];
        x[j] = ((held >> j) & 1) ? q : refine_clamp(q + p.delta[r * 7 + j], sb.lb[j], sb.ub[j]);
        usable = usable && angle_in_domain(x[j]);
        moved = moved || x[j] != q;
    }
    return (usable ? 1 : 0) | (moved ? 2 : 0);
}

// ---- trial: one item per frame ----
SEQIK_HD void smooth_trial(const SmoothProblem &p, int64_t r)
{
    const SmoothAt at = smooth_at(p, r);
    if (p.traj[at.traj].status != SMOOTH_TRIAL) return;
    double e = 0.0;
    if (!smooth_bad(p, r)) {
        double x[7], xp[7];
        const int v = smooth_trial_point(p, r, at.leg, x);
        if (smooth_pair(p, r, at.t)) smooth_trial_point(p, r - 1, at.leg, xp);
#pragma unroll
        for (int j = 0; j < 7; ++j) p.qn[r * 7 + j] = x[j];
        const int32_t flags = ((v & 1) ? 0 : SMOOTH_UNUSABLE) | ((v & 2) ? SMOOTH_MOVED : 0);
        if (flags) smooth_flag(&p.traj[at.traj].flags, flags);
        if (v & 1) e = smooth_frame_cost(p, r, at, x, xp);  // (outside the domain the chain is not walked: the trial is lost anyway)
    }
    p.e[at.traj * p.n_pad + at.t] = e;
}

// ---- decide: one item per trajectory, after the tree -> whether qn becomes q ----
SEQIK_HD bool smooth_decide(const SmoothProblem &p, int64_t traj)
{
    SmoothTraj &tr = p.traj[traj];
    if (tr.status != SMOOTH_TRIAL) return false;
    const double c_new = p.e[traj * p.n_pad], c = tr.cost;
    const bool usable = !(tr.flags & SMOOTH_UNUSABLE), moved = (tr.flags & SMOOTH_MOVED) != 0;
    tr.flags = 0;
    if (usable && c_new < c) {
        tr.last = c - c_new <= p.opt.ftol * c;
        tr.cost = c_new;
        tr.iters += 1;
        const double l = tr.lambda / 3.0;
        tr.lambda = l < kRefineLambdaMin ? kRefineLambdaMin : l;
        tr.status = SMOOTH_ASSEMBLE;
        return true;
    }
    tr.rejects += 1;
    if (usable && moved && c_new - c <= p.opt.ftol * c) {  // the cost no longer tells the two points apart
        tr.reason = REFINE_STOP_DECREASE;
        tr.status = SMOOTH_STOPPED;
        return false;
    }
    tr.lambda = tr.lambda * 4.0;
    if (tr.lambda > kRefineLambdaMax) {
        tr.reason = REFINE_STOP_DAMPING;
        tr.status = SMOOTH_STOPPED;
    }
    return false;
}

// the starting cost of a trajectory, after the tree
SEQIK_HD void smooth_start(const SmoothProblem &p, int64_t traj)
{
    p.traj[traj].cost = p.traj[traj].cost0 = p.e[traj * p.n_pad];
}

// ---- finish: one item per frame ----
SEQIK_HD void smooth_finish(const SmoothProblem &p, int64_t r)
{
    const SmoothAt at = smooth_at(p, r);
    const bool bad = smooth_bad(p, r);
    const double nan = __builtin_nan("");
#pragma unroll
    for (int j = 0; j < 7; ++j) p.angles_out[r * 7 + j] = bad ? nan : p.q[r * 7 + j];
    if (p.frame_info) p.frame_info[r] = p.held[r];
    if (at.t == 0) {
        const SmoothTraj &tr = p.traj[at.traj];
        if (p.cost) {
            p.cost[at.traj * 2] = tr.cost0;
            p.cost[at.traj * 2 + 1] = tr.cost;
        }
        if (p.info) {
            p.info[at.traj * 3] = tr.reason;
            p.info[at.traj * 3 + 1] = tr.iters;
            p.info[at.traj * 3 + 2] = tr.rejects;
        }
    }
}

// ------------------------------------------------ the rule run on the host ------------------------------------------------

// the trees of the trajectories whose e was just written: all of them at the start, then those in a trial
inline void smooth_tree_host(const SmoothProblem &p, bool start)
{
    for (int64_t traj = 0; traj < p.n_traj; ++traj) {
        if (!start && p.traj[traj].status != SMOOTH_TRIAL) continue;
        for (int64_t m = 1; m < p.n_pad; m *= 2)
            for (int64_t i = 0; i < p.n_pad / (2 * m); ++i) smooth_tree_add(p, traj, m, i);
    }
}

// The block-tridiagonal solve on rows[0] of the trajectories in status SMOOTH_TRIAL -> delta
inline void smooth_solve_host(const SmoothProblem &p)
{
    const int64_t R = p.n_traj * p.n_frames;
    int cur = 0;
    for (int64_t h = 1; h < p.n_frames; h *= 2) {
        for (int64_t r = 0; r < R; ++r)
            for (int c = 0; c < kSmoothLanes; ++c) smooth_normalise(p, r, c, cur);
        for (int64_t r = 0; r < R; ++r)
            for (int c = 0; c < kSmoothLanes; ++c) smooth_reduce(p, r, c, h, cur);
        cur ^= 1;
    }
    for (int64_t r = 0; r < R; ++r) smooth_final(p, r, cur);
}

// The whole rule; p's workspace is host memory -> the trial rounds run
inline int64_t smooth_run_host(const SmoothProblem &p)
{
    const int64_t R = p.n_traj * p.n_frames;
    int64_t rounds = 0;
    for (int64_t r = 0; r < R; ++r) smooth_init(p, r);
    for (int64_t r = 0; r < R; ++r) smooth_start_cost(p, r);
    smooth_tree_host(p, true);
    for (int64_t traj = 0; traj < p.n_traj; ++traj) smooth_start(p, traj);
    for (;;) {
        for (int64_t r = 0; r < R; ++r) smooth_assemble(p, r);
        *p.active = 0;
        for (int64_t traj = 0; traj < p.n_traj; ++traj) smooth_stop(p, traj);
        if (*p.active == 0) break;
        ++rounds;
        for (int64_t r = 0; r < R; ++r)
            for (int c = 0; c < kSmoothLanes; ++c) smooth_setup(p, r, c);
        smooth_solve_host(p);
        for (int64_t r = 0; r < R; ++r) smooth_trial(p, r);
        smooth_tree_host(p, false);
        for (int64_t traj = 0; traj < p.n_traj; ++traj) {
            if (smooth_decide(p, traj))
                for (int64_t i = traj * p.n_frames * 7; i < (traj + 1) * p.n_frames * 7; ++i) p.q[i] = p.qn[i];
        }
    }
    for (int64_t r = 0; r < R; ++r) smooth_finish(p, r);
    return rounds;
}

}  // namespace seqik
