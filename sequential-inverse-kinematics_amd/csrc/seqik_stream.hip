// seqik_stream.hip -- slab-streaming pipeline over host buffers (include/seqik.h, "Streaming").
//
// BASELINE config 5: a recording set that does not have to fit (or live) in HBM is pushed through
// the stage kernels in slabs.  A slab is n_seq sequences x n_legs x n_frames; the reference's
// counterpart is one run_ik_and_fk call per piece of a recording (seqikpy/leg_inverse_kinematics.py:324)
// with AlignPose.align_leg applied beforehand (seqikpy/alignment.py:436-487; here fused into the
// kernel prologue through SeqikAffine).
//
// Pipeline: HIP streams for H2D copy, compute (one per slot, up to three, so that the tail of one slab's
// kernels overlaps the head of the next -- one when slabs are carried) and D2H copy, and n_slots
// device slots, chained by events only -- the host thread blocks solely when it wants to reuse a slot whose results
// have not reached the host yet:
//
//   submit(k):  wait done[slot]  ->  h2d: copy pose -> record up[slot]
//               compute: wait up[slot] -> 4 stage kernels (+ carry kernels) -> record solved[slot]
//               d2h: wait solved[slot] -> copy angles (+ FK) -> record done[slot]
//
// PCIe is full duplex, so slab k + 1 goes up while slab k is solved and slab k - 1 comes down.
// Host buffers should be pinned (seqik_host_alloc / seqik_host_register): hipMemcpyAsync from
// pageable memory is staged by the runtime and serialises the pipeline (it still gives the
// right answer).
//
// carry != 0: the slabs are consecutive pieces IN TIME of the same n_seq recordings; frame 0 of
// slab k + 1 is warm-started from the last frame of slab k (kept on the device, no host round
// trip), exactly as the reference's frame loop would have continued (:272).
//
// Skip mode (include/seqik_stream_gaps.h): the compute step of a slab becomes compact -> solve the compacted slab ->
// (carry) select the state -> expand, all on the slot's compute stream and from buffers the slot owns.  A carried skip
// stream always solves with an init block: it starts as the seed state (bit-equivalent to none) and a chain replaces
// its row only when a slab gave it a non-missing frame -- n_valid is read on the device, where the compaction wrote it.
#include <hip/hip_runtime.h>
#include <string.h>
#include <new>
#include <vector>

#include "seqik_gaps.hpp"
#include "seqik_runtime.hpp"
#include "../../include/seqik_stream_gaps.h"

namespace {

using seqik::bad_arg;

// last-frame joint angles of every chain -> init block [chain][7] of the next slab
__global__ void __launch_bounds__(256) seqik_carry_kernel(const double *angles, double *init, int64_t n_chains,
                                                          int64_t n_frames, int64_t ang_chain, int64_t ang_dof,
                                                          int64_t ang_frame)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_chains * 7) return;
    const int64_t c = i / 7;
    const int dof = (int)(i - c * 7);
    init[i] = angles[c * ang_chain + dof * ang_dof + (n_frames - 1) * ang_frame];
}

// skip mode: the state of chain c becomes the compact angles [chain][n_frames][7] at its last non-missing frame; a chain
// whose slab had none keeps its row (no store).  One lane per (chain, DOF).
__global__ void __launch_bounds__(256) seqik_carry_skip_kernel(const double *cangles, const int32_t *n_valid, double *init,
                                                               int64_t n_chains, int64_t n_frames)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_chains * 7) return;
    const int64_t c = i / 7;
    const int64_t slot = seqik::gaps_carry_slot(n_valid[c]);
    if (slot < 0 || slot >= n_frames) return;  // (n_valid <= n_frames by construction: never read outside the chain)
    init[i] = cangles[(c * n_frames + slot) * 7 + (i - c * 7)];
}

struct Slot {
    double *d_pose = nullptr, *d_angles = nullptr, *d_fk = nullptr;
    // skip mode: the compacted slab and its solve
    double *d_cpose = nullptr, *d_cangles = nullptr, *d_cfk = nullptr;
    int32_t *d_map = nullptr, *d_n_valid = nullptr;
    hipEvent_t up = nullptr, solved = nullptr, done = nullptr;
    bool in_flight = false;
};

}  // namespace

struct SeqikStream {
    int device = 0;
    int32_t n_legs = 0;
    int64_t slab_seq = 0, n_frames = 0;
    bool want_fk = false, carry = false, generic = false;
    bool skip = false;          // opened with seqik_stream_open_skip
    bool have_layout = false;
    SeqikLayout layout{};
    std::vector<SeqikLegParams> legs;
    std::vector<SeqikAffine> affine;
    SeqikOptions opt{};
    hipStream_t h2d = nullptr, compute[3] = {nullptr, nullptr, nullptr}, d2h = nullptr;
    int n_compute = 1;
    std::vector<Slot> slots;
    double *d_init = nullptr;   // carry: [slab_seq * n_legs][7]
    double *d_seed = nullptr;   // carried skip stream: the seed state of every chain, never written after open
    bool have_init = false;     // a previous slab has left its last frame in d_init (skip mode: d_init always holds a state)
    int64_t carry_seq = -1;     // n_seq of the slabs of a carried run (must stay the same)
    int64_t submitted = 0;
};

namespace {

void destroy(SeqikStream *s)
{
    if (!s) return;
    seqik::DeviceScope scope;
    (void)scope.enter(s->device);
    for (hipStream_t c : s->compute) if (c) (void)hipStreamSynchronize(c);
    if (s->h2d) (void)hipStreamSynchronize(s->h2d);
    if (s->d2h) (void)hipStreamSynchronize(s->d2h);
    for (Slot &q : s->slots) {
        (void)hipFree(q.d_pose); (void)hipFree(q.d_angles); (void)hipFree(q.d_fk);
        (void)hipFree(q.d_cpose); (void)hipFree(q.d_cangles); (void)hipFree(q.d_cfk);
        (void)hipFree(q.d_map); (void)hipFree(q.d_n_valid);
        if (q.up) (void)hipEventDestroy(q.up);
        if (q.solved) (void)hipEventDestroy(q.solved);
        if (q.done) (void)hipEventDestroy(q.done);
    }
    (void)hipFree(s->d_init);
    (void)hipFree(s->d_seed);
    if (s->h2d) (void)hipStreamDestroy(s->h2d);
    for (hipStream_t c : s->compute) if (c) (void)hipStreamDestroy(c);
    if (s->d2h) (void)hipStreamDestroy(s->d2h);
    delete s;
}

int open_impl(SeqikStream *s)
{
    seqik::DeviceScope scope;
    HIP_TRY(seqik::resolve_device(s->device, &s->device));
    HIP_TRY(scope.enter(s->device));
    HIP_TRY(hipStreamCreateWithFlags(&s->h2d, hipStreamNonBlocking));
    // carried slabs depend on each other: one in-order stream.  Otherwise one compute stream per slot, up to three
    // (10 M frames x 6 legs with FK: 1 stream 0.47 s, 2 0.40 s, 3 0.38 s; without FK 2 0.26 s, 3 0.24 s).  That is
    // five streams with the copies: they only overlap on separate hardware queues, i.e. with GPU_MAX_HW_QUEUES >= 8
    // (HIP's default of 4 made the third compute stream a loss: 1.48e8 -> 1.19e8 leg-frames/s).
    s->n_compute = s->carry ? 1 : (int)(s->slots.size() < 3 ? s->slots.size() : 3);
    for (int i = 0; i < s->n_compute; ++i) HIP_TRY(hipStreamCreateWithFlags(&s->compute[i], hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&s->d2h, hipStreamNonBlocking));
    const size_t lf = (size_t)s->slab_seq * s->n_legs * s->n_frames;
    // a custom layout may pad a chain's block (chain stride > dense size): the slots hold whole chain blocks
    const size_t n_ch = (size_t)s->slab_seq * s->n_legs;
    const size_t pose_elems = s->have_layout ? (size_t)s->layout.pose_chain * n_ch : 15 * lf;
    const size_t ang_elems = s->have_layout ? (size_t)s->layout.ang_chain * n_ch : 7 * lf;
    for (Slot &q : s->slots) {
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&q.d_pose), sizeof(double) * pose_elems));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&q.d_angles), sizeof(double) * ang_elems));
        if (s->want_fk) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&q.d_fk), sizeof(double) * 27 * lf));
        if (s->skip) {
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&q.d_cpose), sizeof(double) * 15 * lf));
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&q.d_cangles), sizeof(double) * 7 * lf));
            if (s->want_fk) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&q.d_cfk), sizeof(double) * 27 * lf));
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&q.d_map), sizeof(int32_t) * lf));
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&q.d_n_valid), sizeof(int32_t) * n_ch));
        }
        HIP_TRY(hipEventCreateWithFlags(&q.up, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&q.solved, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&q.done, hipEventDisableTiming));
    }
    if (s->carry) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s->d_init), sizeof(double) * 7 * s->slab_seq * s->n_legs));
    if (s->carry && s->skip) {
        // every chain starts from the seed state; the pristine copy is what reset_carry restores
        std::vector<double> seed(7 * n_ch);
        for (size_t c = 0; c < n_ch; ++c) seqik::stream_seed_state(s->legs[c % s->n_legs], s->generic, &seed[7 * c]);
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s->d_seed), sizeof(double) * 7 * n_ch));
        HIP_TRY(hipMemcpy(s->d_seed, seed.data(), sizeof(double) * 7 * n_ch, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(s->d_init, seed.data(), sizeof(double) * 7 * n_ch, hipMemcpyHostToDevice));
    }
    return SEQIK_OK;
}

// seqik_stream_open and seqik_stream_open_skip
int open_stream(const char *who, bool skip, SeqikStream **out, int32_t n_legs, const SeqikLegParams *legs,
                const SeqikAffine *affine, int64_t slab_seq, int64_t n_frames, const SeqikLayout *layout, int32_t want_fk,
                int32_t n_slots, int32_t carry, int32_t generic, const SeqikOptions *opt)
{
    if (!out) return bad_arg(who, "null handle pointer");
    *out = nullptr;
    if (!legs || n_legs <= 0 || n_legs > 8 || slab_seq <= 0 || n_frames <= 0 || n_slots < 1 || n_slots > 16)
        return bad_arg(who, "bad sizes (n_legs 1..8, slab_seq > 0, n_frames > 0, n_slots 1..16)");
    if (skip && layout) return bad_arg(who, "skip mode supports the dense layout only (layout must be null)");
    if (skip && n_frames > INT32_MAX) return bad_arg(who, "n_frames must be below 2^31 (the frame map is int32)");
    int rc = generic ? seqik_validate_legs_generic(legs, n_legs) : seqik_validate_legs(legs, n_legs, 1, 4);
    if (rc != SEQIK_OK) return rc;
    if (skip && (rc = seqik::check_segments(who, legs, n_legs)) != SEQIK_OK) return rc;
    SeqikStream *s = new (std::nothrow) SeqikStream;
    if (!s) return bad_arg(who, "out of host memory");
    s->device = opt ? opt->device : -1;  // resolved to the current device in open_impl
    s->n_legs = n_legs; s->slab_seq = slab_seq; s->n_frames = n_frames;
    s->want_fk = want_fk != 0; s->carry = carry != 0; s->generic = generic != 0; s->skip = skip;
    s->legs.assign(legs, legs + n_legs);
    if (affine) s->affine.assign(affine, affine + n_legs);
    if (layout) {
        // every element a kernel touches must lie inside its chain's block, and the blocks of a slab are copied
        // as one contiguous piece of n_seq * n_legs chain strides
        const int64_t T = n_frames;
        const bool ok = layout->pose_row > 0 && layout->pose_frame > 0 && layout->ang_dof > 0 && layout->ang_frame > 0 &&
                        4 * layout->pose_row + (T - 1) * layout->pose_frame + 3 <= layout->pose_chain &&
                        6 * layout->ang_dof + (T - 1) * layout->ang_frame + 1 <= layout->ang_chain;
        if (!ok) {
            delete s;
            return bad_arg(who, "layout strides must be positive and every key point / "
                                "angle of a chain must lie inside its chain stride");
        }
        s->layout = *layout;
        s->have_layout = true;
    }
    if (opt) {
        s->opt = *opt;
        s->opt.stage_events = nullptr; s->opt.chunk_stats = nullptr; s->opt.chunk_flags = nullptr; s->opt.chunk_states = nullptr;
        s->opt.chunk_resume = 0; s->opt.frame_lead = 0;
    }
    s->slots.resize(n_slots);
    rc = open_impl(s);
    if (rc != SEQIK_OK) { destroy(s); return rc; }
    *out = s;
    return SEQIK_OK;
}

}  // namespace

extern "C" {

void *seqik_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)seqik::fail(SEQIK_ERR_HIP, "hipHostMalloc failed%s");
        return nullptr;
    }
    return p;
}

void seqik_host_free(void *p)
{
    if (p) (void)hipHostFree(p);
}

int seqik_host_register(void *p, size_t bytes)
{
    if (!p) return bad_arg("seqik_host_register", "null pointer");
    HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterDefault));
    return SEQIK_OK;
}

int seqik_host_unregister(void *p)
{
    if (!p) return bad_arg("seqik_host_unregister", "null pointer");
    HIP_TRY(hipHostUnregister(p));
    return SEQIK_OK;
}

int seqik_stream_open(SeqikStream **out, int32_t n_legs, const SeqikLegParams *legs, const SeqikAffine *affine,
                      int64_t slab_seq, int64_t n_frames, const SeqikLayout *layout, int32_t want_fk,
                      int32_t n_slots, int32_t carry, int32_t generic, const SeqikOptions *opt)
{
    return open_stream("seqik_stream_open", false, out, n_legs, legs, affine, slab_seq, n_frames, layout, want_fk, n_slots,
                       carry, generic, opt);
}

int seqik_stream_open_skip(SeqikStream **out, int32_t n_legs, const SeqikLegParams *legs, const SeqikAffine *affine,
                           int64_t slab_seq, int64_t n_frames, const SeqikLayout *layout, int32_t want_fk,
                           int32_t n_slots, int32_t carry, int32_t generic, const SeqikOptions *opt)
{
    return open_stream("seqik_stream_open_skip", true, out, n_legs, legs, affine, slab_seq, n_frames, layout, want_fk,
                       n_slots, carry, generic, opt);
}

int seqik_stream_seed_state(const SeqikLegParams *legs, int32_t n_legs, int32_t generic, double *state)
{
    if (!legs || !state) return bad_arg("seqik_stream_seed_state", "null pointer");
    if (n_legs < 0) return bad_arg("seqik_stream_seed_state", "negative n_legs");
    for (int32_t l = 0; l < n_legs; ++l) seqik::stream_seed_state(legs[l], generic != 0, state + 7 * l);
    return SEQIK_OK;
}

int seqik_stream_submit(SeqikStream *s, const double *pose, int64_t n_seq, double *angles, double *fk)
{
    if (!s || !pose || !angles) return bad_arg("seqik_stream_submit", "null pointer");
    if (n_seq < 0 || n_seq > s->slab_seq) return bad_arg("seqik_stream_submit", "n_seq exceeds the slab size");
    if (s->want_fk && !fk) return bad_arg("seqik_stream_submit", "the stream was opened with want_fk but fk is null");
    if (n_seq == 0) return SEQIK_OK;
    if (s->carry) {
        if (s->carry_seq >= 0 && s->carry_seq != n_seq)
            return bad_arg("seqik_stream_submit", "a carried run needs the same n_seq in every slab");
        s->carry_seq = n_seq;
    }
    seqik::DeviceScope scope;
    HIP_TRY(scope.enter(s->device));
    Slot &q = s->slots[s->submitted % (int64_t)s->slots.size()];
    if (q.in_flight) { HIP_TRY(hipEventSynchronize(q.done)); q.in_flight = false; }
    const size_t lf = (size_t)n_seq * s->n_legs * s->n_frames;
    // a custom layout may leave gaps only inside a chain block (chain stride >= dense size), so the
    // slab is copied as the contiguous block of n_seq * n_legs chains in either case
    const size_t pose_elems = s->have_layout ? (size_t)s->layout.pose_chain * n_seq * s->n_legs : 15 * lf;
    const size_t ang_elems = s->have_layout ? (size_t)s->layout.ang_chain * n_seq * s->n_legs : 7 * lf;
    HIP_TRY(hipMemcpyAsync(q.d_pose, pose, sizeof(double) * pose_elems, hipMemcpyHostToDevice, s->h2d));
    HIP_TRY(hipEventRecord(q.up, s->h2d));
    hipStream_t compute = s->compute[s->submitted % s->n_compute];
    HIP_TRY(hipStreamWaitEvent(compute, q.up, 0));
    const SeqikLayout *lay = s->have_layout ? &s->layout : nullptr;
    const SeqikAffine *aff = s->affine.empty() ? nullptr : s->affine.data();
    // (a carried skip stream always has a state: the seed state until a slab or set_carry replaces it)
    const double *d_init = (s->carry && (s->skip || s->have_init)) ? s->d_init : nullptr;
    // skip mode solves the compacted slab into the slot's compact buffers
    const int32_t gflags = (s->generic ? SEQIK_GAPS_GENERIC : SEQIK_GAPS_SEQ) | (aff ? SEQIK_GAPS_AFFINE : 0);
    const double *d_solve_pose = s->skip ? q.d_cpose : q.d_pose;
    double *d_solve_angles = s->skip ? q.d_cangles : q.d_angles, *d_solve_fk = s->skip ? q.d_cfk : q.d_fk;
    int rc = SEQIK_OK;
    if (s->skip)
        rc = seqik_gaps_compact_device(q.d_pose, n_seq, s->n_legs, s->n_frames, gflags, s->legs.data(), q.d_cpose, q.d_map,
                                       q.d_n_valid, compute);
    if (rc != SEQIK_OK) return rc;
    if (s->generic)
        rc = seqik_solve_generic_device(d_solve_pose, n_seq, s->n_legs, s->n_frames, s->legs.data(), d_solve_angles,
                                        d_solve_fk, nullptr, nullptr, d_init, lay, aff, &s->opt, compute);
    else
        rc = seqik_solve_seq_device(d_solve_pose, n_seq, s->n_legs, s->n_frames, s->legs.data(), 1, 4, d_solve_angles,
                                    d_solve_fk, nullptr, nullptr, d_init, lay, aff, &s->opt, compute);
    if (rc != SEQIK_OK) return rc;
    if (s->carry && s->skip) {
        const int64_t n_chains = n_seq * s->n_legs;
        const unsigned blocks = (unsigned)((n_chains * 7 + 255) / 256);
        hipLaunchKernelGGL(seqik_carry_skip_kernel, dim3(blocks), dim3(256), 0, compute, q.d_cangles, q.d_n_valid,
                           s->d_init, n_chains, s->n_frames);
        HIP_TRY(hipGetLastError());
        s->have_init = true;
    } else if (s->carry) {
        const int64_t n_chains = n_seq * s->n_legs;
        const int64_t ac = lay ? lay->ang_chain : s->n_frames * 7, ad = lay ? lay->ang_dof : 1, af = lay ? lay->ang_frame : 7;
        const unsigned blocks = (unsigned)((n_chains * 7 + 255) / 256);
        hipLaunchKernelGGL(seqik_carry_kernel, dim3(blocks), dim3(256), 0, compute, q.d_angles, s->d_init, n_chains,
                           s->n_frames, ac, ad, af);
        HIP_TRY(hipGetLastError());
        s->have_init = true;
    }
    if (s->skip) {
        rc = seqik_gaps_expand_device(q.d_map, n_seq, s->n_legs, s->n_frames, gflags, q.d_cangles, q.d_cfk, nullptr, nullptr,
                                      q.d_angles, q.d_fk, nullptr, nullptr, compute);
        if (rc != SEQIK_OK) return rc;
    }
    HIP_TRY(hipEventRecord(q.solved, compute));
    HIP_TRY(hipStreamWaitEvent(s->d2h, q.solved, 0));
    HIP_TRY(hipMemcpyAsync(angles, q.d_angles, sizeof(double) * ang_elems, hipMemcpyDeviceToHost, s->d2h));
    if (s->want_fk) HIP_TRY(hipMemcpyAsync(fk, q.d_fk, sizeof(double) * 27 * lf, hipMemcpyDeviceToHost, s->d2h));
    HIP_TRY(hipEventRecord(q.done, s->d2h));
    q.in_flight = true;
    s->submitted += 1;
    return SEQIK_OK;
}

int seqik_stream_wait(SeqikStream *s)
{
    if (!s) return bad_arg("seqik_stream_wait", "null handle");
    seqik::DeviceScope scope;
    HIP_TRY(scope.enter(s->device));
    for (Slot &q : s->slots)
        if (q.in_flight) { HIP_TRY(hipEventSynchronize(q.done)); q.in_flight = false; }
    // every slab is back: a watchdog fault in one of them must not pass silently (this pipeline's own streams only)
    int rc = SEQIK_OK;
    for (int i = 0; i < s->n_compute; ++i) {
        const int r = seqik_check_faults_stream(s->compute[i]);
        if (r != SEQIK_OK) rc = r;
    }
    return rc;
}

int seqik_stream_reset_carry(SeqikStream *s)
{
    if (!s) return bad_arg("seqik_stream_reset_carry", "null handle");
    if (s->carry && s->skip) {
        // back to the seed state, ordered on the compute stream behind the slab before: no host synchronisation
        seqik::DeviceScope scope;
        HIP_TRY(scope.enter(s->device));
        HIP_TRY(hipMemcpyAsync(s->d_init, s->d_seed, sizeof(double) * 7 * s->slab_seq * s->n_legs, hipMemcpyDeviceToDevice,
                               s->compute[0]));
    }
    s->have_init = false;
    s->carry_seq = -1;
    return SEQIK_OK;
}

int seqik_stream_set_carry(SeqikStream *s, const double *init, int64_t n_seq, int32_t on_device)
{
    if (!s || !init) return bad_arg("seqik_stream_set_carry", "null pointer");
    if (!s->carry) return bad_arg("seqik_stream_set_carry", "the stream was not opened with carry");
    if (n_seq <= 0 || n_seq > s->slab_seq) return bad_arg("seqik_stream_set_carry", "n_seq exceeds the slab size");
    seqik::DeviceScope scope;
    HIP_TRY(scope.enter(s->device));
    // ordered on the compute stream: behind the slab before (whose carry kernel writes the same buffer), in front of the next
    HIP_TRY(hipMemcpyAsync(s->d_init, init, sizeof(double) * 7 * n_seq * s->n_legs,
                        on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->compute[0]));
    if (!on_device) HIP_TRY(hipStreamSynchronize(s->compute[0]));  // the caller's host buffer may go away
    s->have_init = true;
    s->carry_seq = n_seq;
    return SEQIK_OK;
}

int seqik_stream_get_carry(SeqikStream *s, double *state, int64_t n_seq)
{
    if (!s || !state) return bad_arg("seqik_stream_get_carry", "null pointer");
    if (!s->carry) return bad_arg("seqik_stream_get_carry", "the stream was not opened with carry");
    if (n_seq <= 0 || n_seq > s->slab_seq) return bad_arg("seqik_stream_get_carry", "n_seq exceeds the slab size");
    if (!s->skip && !s->have_init)
        return bad_arg("seqik_stream_get_carry", "the stream has no state yet (no slab submitted, no set_carry)");
    seqik::DeviceScope scope;
    HIP_TRY(scope.enter(s->device));
    // behind the carry kernel of the last slab submitted (carried streams have one compute stream)
    HIP_TRY(hipMemcpyAsync(state, s->d_init, sizeof(double) * 7 * n_seq * s->n_legs, hipMemcpyDeviceToHost, s->compute[0]));
    HIP_TRY(hipStreamSynchronize(s->compute[0]));
    return SEQIK_OK;
}

int seqik_stream_close(SeqikStream *s)
{
    destroy(s);
    return SEQIK_OK;
}

}  // extern "C"
