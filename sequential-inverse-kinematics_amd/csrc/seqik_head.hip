// seqik_head.hip -- head / antenna angle kernel and its C ABI entry points (include/seqik.h).  The host side of a launch
// (argument rules, grid, choice of kernel, the host entry point's buffers) is seqik_head_launch.hpp, shared with
// seqik_head_align.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "seqik_core.hpp"
#include "seqik_head_launch.hpp"

namespace {

using seqik::bad_arg;
using seqik::wave_lds_fence;

typedef double d2 __attribute__((ext_vector_type(2)));

// One frame per lane, grid-stride.  Per frame 96 B in (two AoS records of 48 B) and 56 B out (seven SoA rows): the
// kernel is meant to run at the rate of a copy.  What that took (scripts/microbench/head_split.hip):
//   * every load of a frame is issued before its first store (the seven angles go to registers first): input and
//     output may alias as far as the compiler knows, so a store in the middle held the later loads back -- two memory
//     round trips per frame, 2.2 -> 1.75 ms for 64 M frames;
//   * STAGED: a wavefront's 64 records are one contiguous 3 KiB block per array; it comes in as three fully coalesced
//     16-byte-per-lane loads (1 KiB each, non-temporal: read once) into LDS and the lanes pick their records from
//     there; the outputs leave as non-temporal stores.  1.75 -> 1.67 ms; a copy with the same traffic takes 1.58 ms.
//     (Non-temporal loads WITHOUT the staging are a loss, 2.1 ms: the three strided loads of a lane then miss each
//     other's lines.)  Needs 16-byte aligned inputs and whole wavefronts; everything else takes the per-lane loads.
// GIVEN_ROLL: the derotation uses the caller's head roll (a.roll_in) -- its own instantiation, so that the sin / cos it
// needs stay out of the usual kernel's registers.
template <bool STAGED, bool GIVEN_ROLL = false>
__global__ void __launch_bounds__(256) seqik_head_kernel(seqik::HeadArgs a)
{
    __shared__ d2 s_stage[STAGED ? 4 * 384 : 1];  // per wavefront: 2 arrays x 3072 B = 384 x 16 B
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, n = a.n_frames;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool ant = a.compute_ant != 0;
    const int n_out = ant ? 7 : 3;
    for (int64_t t0 = (int64_t)blockIdx.x * blockDim.x; t0 < n; t0 += stride) {
        const int64_t t = t0 + threadIdx.x;
        const int64_t w0 = t0 + wave * 64;  // first frame of this wavefront
        double out[7];
        if (STAGED && w0 + 64 <= n) {
            d2 *st = s_stage + wave * 384;
            const d2 *gr = reinterpret_cast<const d2 *>(a.r_head + w0 * 6);
            const d2 *gl = reinterpret_cast<const d2 *>(a.l_head + w0 * 6);
            const d2 r0 = __builtin_nontemporal_load(gr + lane), r1 = __builtin_nontemporal_load(gr + 64 + lane),
                     r2 = __builtin_nontemporal_load(gr + 128 + lane);
            const d2 l0 = __builtin_nontemporal_load(gl + lane), l1 = __builtin_nontemporal_load(gl + 64 + lane),
                     l2 = __builtin_nontemporal_load(gl + 128 + lane);
            st[lane] = r0; st[64 + lane] = r1; st[128 + lane] = r2;
            st[192 + lane] = l0; st[256 + lane] = l1; st[320 + lane] = l2;
            wave_lds_fence();
            seqik::head_angles_compute(reinterpret_cast<const double *>(st) + lane * 6,
                                       reinterpret_cast<const double *>(st + 192) + lane * 6, a.neck + t * a.neck_stride,
                                       a.rest_head_pitch, a.rest_antenna_pitch, ant, out, GIVEN_ROLL ? a.roll_in + t : nullptr);
            wave_lds_fence();  // the next iteration's LDS writes stay behind these reads
#pragma unroll
            for (int j = 0; j < 7; ++j)
                if (j < n_out) __builtin_nontemporal_store(out[j], a.angles + j * n + t);
        } else if (t < n) {
            seqik::head_angles_compute(a.r_head + t * a.rec, a.l_head + t * a.rec, a.neck + t * a.neck_stride,
                                       a.rest_head_pitch, a.rest_antenna_pitch, ant, out, GIVEN_ROLL ? a.roll_in + t : nullptr);
#pragma unroll
            for (int j = 0; j < 7; ++j)
                if (j < n_out) a.angles[j * n + t] = out[j];
        }
    }
}

// angle_between_segments for general vectors: one pair per lane; a stride of 0 broadcasts one vector to every row
__global__ void __launch_bounds__(256) seqik_signed_angle_kernel(const double *v1, int64_t s1, const double *v2, int64_t s2,
                                                                 double ax, double ay, double az, int64_t n, double *out)
{
    const double axis[3] = {ax, ay, az};
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
        out[t] = seqik::signed_angle3(v1 + t * s1, v2 + t * s2, axis);
}

// by seqik::HeadVariant: per-lane loads + given roll, staged, per-lane
const seqik::HeadKernel<seqik::HeadArgs> kHeadKernels[3] = {seqik_head_kernel<false, true>, seqik_head_kernel<true>,
                                                            seqik_head_kernel<false>};
constexpr const char *kWho = "seqik_head_angles";

}  // namespace

extern "C" {

int seqik_head_angles_device(const double *d_r_head, const double *d_l_head, int64_t n_frames, const double *d_neck,
                             int64_t neck_stride, double rest_head_pitch, double rest_antenna_pitch,
                             int32_t compute_ant, double *d_angles, void *hip_stream)
{
    return seqik_head_angles_ex_device(d_r_head, d_l_head, n_frames, 2, d_neck, neck_stride, rest_head_pitch,
                                       rest_antenna_pitch, compute_ant, nullptr, d_angles, hip_stream);
}

int seqik_head_angles_ex_device(const double *d_r_head, const double *d_l_head, int64_t n_frames, int32_t n_points,
                                const double *d_neck, int64_t neck_stride, double rest_head_pitch,
                                double rest_antenna_pitch, int32_t compute_ant, const double *d_head_roll,
                                double *d_angles, void *hip_stream)
{
    if (int rc = seqik::check_head_args(kWho, d_r_head, d_l_head, d_neck, d_angles, n_frames, neck_stride, n_points, compute_ant))
        return rc;
    if (n_frames == 0) return SEQIK_OK;
    const seqik::HeadArgs a = seqik::head_args(d_r_head, d_l_head, n_frames, n_points, d_neck, neck_stride, rest_head_pitch,
                                               rest_antenna_pitch, compute_ant, d_head_roll, d_angles);
    return seqik::launch_head(kHeadKernels, seqik::plan_head(a), a, hip_stream);
}

int seqik_head_angles(const double *r_head, const double *l_head, int64_t n_frames, const double *neck,
                      int64_t neck_stride, double rest_head_pitch, double rest_antenna_pitch, int32_t compute_ant,
                      double *angles, const SeqikOptions *opt)
{
    return seqik_head_angles_ex(r_head, l_head, n_frames, 2, neck, neck_stride, rest_head_pitch, rest_antenna_pitch,
                                compute_ant, nullptr, angles, opt);
}

int seqik_head_angles_ex(const double *r_head, const double *l_head, int64_t n_frames, int32_t n_points, const double *neck,
                         int64_t neck_stride, double rest_head_pitch, double rest_antenna_pitch, int32_t compute_ant,
                         const double *head_roll, double *angles, const SeqikOptions *opt)
{
    if (int rc = seqik::check_head_args(kWho, r_head, l_head, neck, angles, n_frames, neck_stride, n_points, compute_ant))
        return rc;
    if (n_frames == 0) return SEQIK_OK;
    seqik::HostCall call;
    seqik::HeadBuffers d;
    d.declare(call, seqik::head_args(r_head, l_head, n_frames, n_points, neck, neck_stride, rest_head_pitch,
                                     rest_antenna_pitch, compute_ant, head_roll, angles));
    if (int rc = call.begin(opt ? opt->device : -1)) return rc;
    return call.finish(seqik_head_angles_ex_device(d.r_head, d.l_head, n_frames, n_points, d.neck, neck_stride,
                                                   rest_head_pitch, rest_antenna_pitch, compute_ant, d.head_roll, d.angles,
                                                   call.stream()));
}

int seqik_signed_angles(const double *v1, int64_t v1_stride, const double *v2, int64_t v2_stride, const double *axis,
                        int64_t n, double *out, const SeqikOptions *opt)
{
    if (!v1 || !v2 || !axis || !out || n < 0 || (v1_stride != 0 && v1_stride != 3) || (v2_stride != 0 && v2_stride != 3))
        return bad_arg("seqik_signed_angles", "bad argument");
    if (n == 0) return SEQIK_OK;
    seqik::HostCall call;
    double *d1, *d2v, *d_o;
    call.upload(d1, v1_stride ? 3 * n : 3, v1);
    call.upload(d2v, v2_stride ? 3 * n : 3, v2);
    call.download(d_o, n, out);
    if (int rc = call.begin(opt ? opt->device : -1)) return rc;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(seqik_signed_angle_kernel, dim3((unsigned)blocks), dim3(256), 0, call.stream(), d1, v1_stride, d2v,
                       v2_stride, axis[0], axis[1], axis[2], n, d_o);
    return call.finish(seqik::launched());
}

}  // extern "C"
