// TEST INFRASTRUCTURE ONLY -- not part of the product, never loaded by seqikpy_amd.
//
// Runs the trajectory refinement's device rule (csrc/seqik_smooth.hpp, `__host__ __device__`) on the HOST, phase after
// phase in plain loops, so that the CPU-only test tier can hold it to its properties, to numpy and to scipy; the GPU tier
// compares the kernels with it bit for bit.  Built by tests/smooth_support.py through harness_build.build_harness.
#include <string.h>
#include <vector>

#include "../../sequential-inverse-kinematics_amd/csrc/seqik_smooth.hpp"

namespace {

void size_problem(seqik::SmoothProblem &p, int64_t n_traj, int32_t n_legs, int64_t n_frames, std::vector<char> &ws)
{
    memset(&p, 0, sizeof p);
    p.n_traj = n_traj; p.n_legs = n_legs; p.n_frames = n_frames;
    p.n_pad = seqik::smooth_pad(n_frames);
    ws.assign(seqik::smooth_carve(p, nullptr) + 8, 0);
    seqik::smooth_carve(p, ws.data() + (8 - (uintptr_t)ws.data() % 8) % 8);
}

// smooth_run_host's loop over the same phase functions, looking between the phases at what the rule itself does not
// report: paths[traj] = {trials lost to a pivot that was not positive, trials lost to an angle outside the domain, the
// trial round after which the trajectory stopped (0: before any trial)} -> the trial rounds run.  The tests hold its
// outputs to smooth_run_host's bit for bit.
int64_t run_watched(const seqik::SmoothProblem &p, int64_t *paths)
{
    using namespace seqik;
    const int64_t R = p.n_traj * p.n_frames;
    int64_t rounds = 0;
    std::vector<char> pivot((size_t)p.n_traj);
    for (int64_t i = 0; i < 3 * p.n_traj; ++i) paths[i] = 0;
    for (int64_t r = 0; r < R; ++r) smooth_init(p, r);
    for (int64_t r = 0; r < R; ++r) smooth_start_cost(p, r);
    smooth_tree_host(p, true);
    for (int64_t traj = 0; traj < p.n_traj; ++traj) smooth_start(p, traj);
    for (;;) {
        for (int64_t r = 0; r < R; ++r) smooth_assemble(p, r);
        *p.active = 0;
        for (int64_t traj = 0; traj < p.n_traj; ++traj) {
            const bool ran = p.traj[traj].status != SMOOTH_STOPPED;
            smooth_stop(p, traj);
            if (ran && p.traj[traj].status == SMOOTH_STOPPED) paths[3 * traj + 2] = rounds;
        }
        if (*p.active == 0) break;
        ++rounds;
        for (int64_t r = 0; r < R; ++r)
            for (int c = 0; c < kSmoothLanes; ++c) smooth_setup(p, r, c);
        smooth_solve_host(p);
        for (int64_t traj = 0; traj < p.n_traj; ++traj) {
            pivot[traj] = p.traj[traj].status == SMOOTH_TRIAL && (p.traj[traj].flags & SMOOTH_UNUSABLE);
            paths[3 * traj] += pivot[traj];
        }
        for (int64_t r = 0; r < R; ++r) smooth_trial(p, r);
        for (int64_t traj = 0; traj < p.n_traj; ++traj)
            paths[3 * traj + 1] += p.traj[traj].status == SMOOTH_TRIAL && (p.traj[traj].flags & SMOOTH_UNUSABLE) && !pivot[traj];
        smooth_tree_host(p, false);
        for (int64_t traj = 0; traj < p.n_traj; ++traj) {
            const bool ran = p.traj[traj].status == SMOOTH_TRIAL;
            if (smooth_decide(p, traj))
                for (int64_t i = traj * p.n_frames * 7; i < (traj + 1) * p.n_frames * 7; ++i) p.q[i] = p.qn[i];
            if (ran && p.traj[traj].status == SMOOTH_STOPPED) paths[3 * traj + 2] = rounds;
        }
    }
    for (int64_t r = 0; r < R; ++r) smooth_finish(p, r);
    return rounds;
}

}  // namespace

// The layouts of include/seqik_smooth.h with the options spelled out; *rounds (nullable) receives the trial rounds run.
// The segment lengths are taken as they are (the C ABI refuses a non-finite one before it reaches the rule).
// `paths` (nullable, [n_seq * n_legs][3]): the decision paths each trajectory took, see run_watched.
extern "C" int harness_smooth_legs_paths(const double *angles, const double *pose, int64_t n_seq, int32_t n_legs,
                                         int64_t n_frames, const SeqikLegParams *legs, const double *kp_weight,
                                         const double *smooth, int32_t max_iter, double gtol, double ftol, double *angles_out,
                                         int32_t *frame_info, double *cost, int32_t *info, int64_t *rounds, int64_t *paths)
{
    if (!angles || !pose || !angles_out || !legs || !smooth || max_iter < 1 || max_iter > 1000 || n_legs < 1 || n_legs > 8)
        return SEQIK_ERR_BAD_ARG;
    if (n_seq * n_legs * n_frames == 0) return SEQIK_OK;
    seqik::SmoothProblem p;
    std::vector<char> ws;
    size_problem(p, n_seq * n_legs, n_legs, n_frames, ws);
    p.angles = angles; p.pose = pose; p.kp_weight = kp_weight;
    p.angles_out = angles_out; p.frame_info = frame_info; p.cost = cost; p.info = info;
    for (int j = 0; j < 7; ++j) p.opt.smooth[j] = smooth[j];
    p.opt.max_iter = max_iter; p.opt.gtol = gtol; p.opt.ftol = ftol;
    for (int l = 0; l < seqik::kFkMaxLegs; ++l) {
        seqik::make_fk_leg(legs[l < n_legs ? l : 0], p.legs[l]);
        seqik::make_leg_bounds(legs[l < n_legs ? l : 0], p.bounds[l]);
    }
    const int64_t r = paths ? run_watched(p, paths) : seqik::smooth_run_host(p);
    if (rounds) *rounds = r;
    return SEQIK_OK;
}

extern "C" int harness_smooth_legs(const double *angles, const double *pose, int64_t n_seq, int32_t n_legs, int64_t n_frames,
                                   const SeqikLegParams *legs, const double *kp_weight, const double *smooth,
                                   int32_t max_iter, double gtol, double ftol, double *angles_out, int32_t *frame_info,
                                   double *cost, int32_t *info, int64_t *rounds)
{
    return harness_smooth_legs_paths(angles, pose, n_seq, n_legs, n_frames, legs, kp_weight, smooth, max_iter, gtol, ftol,
                                     angles_out, frame_info, cost, info, rounds, nullptr);
}

// The linear solve alone, one trajectory: rows [n][154] (D 49 row-major of which the lower triangle is read, L 49, U 49,
// b 7) -> delta [n][7]; returns 1 when a pivot was not positive (the trial would be a rejection), else 0.
extern "C" int harness_smooth_solve(const double *rows, int64_t n, double *delta)
{
    if (!rows || !delta || n < 1) return SEQIK_ERR_BAD_ARG;
    seqik::SmoothProblem p;
    std::vector<char> ws;
    size_problem(p, 1, 1, n, ws);
    p.traj[0].status = seqik::SMOOTH_TRIAL;
    memcpy(p.rows[0], rows, sizeof(double) * seqik::kSmoothRow * (size_t)n);
    seqik::smooth_solve_host(p);
    memcpy(delta, p.delta, sizeof(double) * 7 * (size_t)n);
    return (p.traj[0].flags & seqik::SMOOTH_UNUSABLE) ? 1 : 0;
}
