// seqik_head_launch.hpp -- the host side of a head / antenna angle launch, once for seqik_head.hip (aligned key points)
// and seqik_head_align.hip (raw key points, the alignment fused into the kernel): HeadArgs filled from the arguments the
// entry points share, the launch plan, the launch through the plan's choice of kernel, and the device buffers of the
// host entry points.  The argument rules are check_head_args (seqik_runtime.hpp).  Host code only: the kernels stay in
// the units.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "seqik_head.hpp"
#include "seqik_runtime.hpp"

namespace seqik {

// what every head entry point is given, in the order of its parameters (host or device pointers alike)
inline HeadArgs head_args(const double *r_head, const double *l_head, int64_t n_frames, int32_t n_points, const double *neck,
                          int64_t neck_stride, double rest_head_pitch, double rest_antenna_pitch, int32_t compute_ant,
                          const double *head_roll, double *angles)
{
    HeadArgs a;
    a.r_head = r_head; a.l_head = l_head; a.neck = neck; a.neck_stride = neck_stride;
    a.rec = 3 * (int64_t)n_points; a.roll_in = compute_ant ? head_roll : nullptr;
    a.rest_head_pitch = rest_head_pitch; a.rest_antenna_pitch = rest_antenna_pitch;
    a.angles = angles; a.n_frames = n_frames; a.compute_ant = compute_ant;
    return a;
}

// ---- the launch plan ----
enum HeadVariant { kHeadGivenRoll, kHeadStaged, kHeadPerLane };  // the kernels of a unit, in this order

struct HeadPlan {
    int64_t blocks;  // workgroups of 256 threads
    HeadVariant variant;
};

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// r_aligned / l_aligned: the nullable aligned-record outputs of the fused kernels
inline HeadPlan plan_head(const HeadArgs &a, const void *r_aligned = nullptr, const void *l_aligned = nullptr)
{
    // (round 5: 64 workgroups per CU in the grid instead of 8 -- at most six are resident (LDS), the rest queue up and each
    // makes fewer grid-stride rounds: 16 M frames 0.483 -> 0.473 ms, 64 M 1.955 -> 1.902 ms; profiles/r05_head_blocks_per_cu.txt)
    static const int per_cu = getenv("SEQIK_HEAD_BLOCKS_PER_CU") ? atoi(getenv("SEQIK_HEAD_BLOCKS_PER_CU")) : 64;
    HeadPlan p;
    p.blocks = (a.n_frames + 255) / 256;
    if (p.blocks > 256 * (int64_t)per_cu) p.blocks = 256 * (int64_t)per_cu;  // grid-stride beyond per_cu blocks per CU
    // staged loads / stores move a wavefront's 64 two-point records as 16-byte pieces, so every array that takes part must
    // be 16-byte aligned (an output that was not asked for is), and they read the antenna tips too: only worth it when
    // those are used
    const bool staged = a.compute_ant && a.rec == 6 && aligned16(a.r_head) && aligned16(a.l_head) &&
                        aligned16(r_aligned) && aligned16(l_aligned);
    p.variant = a.roll_in ? kHeadGivenRoll : staged ? kHeadStaged : kHeadPerLane;
    return p;
}

template <typename Args> using HeadKernel = void (*)(Args);

// kernels: a unit's instantiations by HeadVariant.  SEQIK_OK, or the error of the launch
template <typename Args>
int launch_head(const HeadKernel<Args> (&kernels)[3], const HeadPlan &p, const Args &k, void *hip_stream)
{
    hipLaunchKernelGGL(kernels[p.variant], dim3((unsigned)p.blocks), dim3(256), 0, static_cast<hipStream_t>(hip_stream), k);
    return launched();
}

// ---- the device buffers every host entry point declares, for the arrays of `host` (head_args of its host pointers) ----
struct HeadBuffers {  // (begin() assigns the members where declare() saw them: a local of the entry point)
    double *head_roll, *r_head, *l_head, *neck, *angles;
    void declare(HostCall &call, const HeadArgs &host)
    {
        const size_t n = (size_t)host.n_frames;
        call.upload(head_roll, n, host.roll_in);
        call.upload(r_head, (size_t)host.rec * n, host.r_head);
        call.upload(l_head, (size_t)host.rec * n, host.l_head);
        call.upload(neck, host.neck_stride ? 3 * n : 3, host.neck);
        call.download(angles, 7 * n, host.angles, (host.compute_ant ? 7 : 3) * n);
    }
};

}  // namespace seqik
