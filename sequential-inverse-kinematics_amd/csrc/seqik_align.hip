// seqik_align.hip -- the reductions of AlignPose on the GPU (include/seqik.h, "Alignment statistics").
//
// AlignPose.align_leg (seqikpy/alignment.py:436-487) is an affine map whose constants come from whole-recording
// statistics (seqikpy/alignment.py:83-87, 392-434):
//   fixed_coxa[a]   = mean of the 0.45 and 0.55 quantiles of the coxa coordinate a          (get_fixed_pos)
//   mean length[i]  = mean of the 0.45 and 0.55 quantiles of |key point i+1 - key point i|   (get_mean_length)
// i.e. per leg SEVEN per-frame series, of each of which np.quantile needs the order statistics around two ranks.
// On the host this costs ~5 s per million frames and six legs -- more than ten times the solve -- so for long
// recordings it is the bottleneck of "alignment fused into the kernel prologue" (BASELINE config 5).
//
// Here: a kernel extracts the seven series per leg from the RAW key points (with numpy's rounding sequence:
// sqrt((dx*dx + dy*dy) + dz*dz)), hipCUB radix-sorts each series (plain library sort; order statistics are
// exact whatever the algorithm), and the requested ranks are returned -- the sort loop, the pick kernel and the
// handle's open / close are seqik_order_stats.hpp, shared with seqik_head_align.hip.  The caller applies numpy's own
// interpolation / mean / scale formulas to them (seqikpy_amd/alignment.py), so the affine constants are
// bit-identical to the reference's.  Slabs can be added one at a time (streaming): the order of the frames does
// not matter.
#include <hip/hip_runtime.h>

#include "seqik_order_stats.hpp"

namespace {

using seqik::bad_arg;

constexpr int kSeries = 7;  // coxa x, y, z; coxa, femur, tibia, tarsus length

// series[(leg * 7 + j) * capacity + offset + seq * n_frames + t]
__global__ void __launch_bounds__(256) seqik_align_extract_kernel(
    const double *pose, int64_t n_seq, int32_t n_legs, int64_t n_frames, int64_t pose_chain, int64_t pose_row,
    int64_t pose_frame, double *series, int64_t capacity, int64_t offset)
{
    const int64_t total = n_seq * n_legs * n_frames;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t t = i % n_frames;
        const int64_t c = i / n_frames;  // chain = seq * n_legs + leg
        const int leg = (int)(c % n_legs);
        const int64_t seq = c / n_legs;
        const double *p = pose + c * pose_chain + t * pose_frame;
        double kp[5][3];
#pragma unroll
        for (int r = 0; r < 5; ++r)
#pragma unroll
            for (int a = 0; a < 3; ++a) kp[r][a] = p[r * pose_row + a];
        double *out = series + (int64_t)leg * kSeries * capacity + offset + seq * n_frames + t;
#pragma unroll
        for (int a = 0; a < 3; ++a) out[a * capacity] = kp[0][a];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double dx = kp[r + 1][0] - kp[r][0], dy = kp[r + 1][1] - kp[r][1], dz = kp[r + 1][2] - kp[r][2];
            // np.linalg.norm(np.diff(...), axis=2): sqrt(add.reduce(x * x)) = sqrt((dx*dx + dy*dy) + dz*dz)
            out[(3 + r) * capacity] = sqrt((dx * dx + dy * dy) + dz * dz);
        }
    }
}

}  // namespace

struct SeqikAlignStats : seqik::SeriesHandle {  // d_series: [n_legs][7][capacity]
    int32_t n_legs = 0;
    int64_t capacity = 0, count = 0;  // frames per leg: room / filled
    double *d_stage = nullptr;        // staging for host slabs
    size_t stage_bytes = 0;
    ~SeqikAlignStats() { (void)hipFree(d_stage); }  // (_close deletes the handle on its device)
};

extern "C" {

int seqik_align_stats_open(SeqikAlignStats **out, int32_t n_legs, int64_t capacity_frames, const SeqikOptions *opt)
{
    if (!out) return bad_arg("seqik_align_stats_open", "null handle pointer");
    *out = nullptr;
    if (n_legs <= 0 || n_legs > 8 || capacity_frames <= 0)
        return bad_arg("seqik_align_stats_open", "bad sizes (n_legs 1..8, capacity_frames > 0)");
    if (int rc = seqik::open_series("seqik_align_stats_open", opt, (size_t)kSeries * n_legs * capacity_frames, out)) return rc;
    (*out)->n_legs = n_legs;
    (*out)->capacity = capacity_frames;
    return SEQIK_OK;
}

int seqik_align_stats_add(SeqikAlignStats *s, const double *pose, int32_t pose_on_device, int64_t n_seq,
                          int64_t n_frames, const SeqikLayout *layout, void *hip_stream)
{
    if (!s || !pose) return bad_arg("seqik_align_stats_add", "null pointer");
    if (n_seq < 0 || n_frames < 0) return bad_arg("seqik_align_stats_add", "negative size");
    if (n_seq == 0 || n_frames == 0) return SEQIK_OK;
    int64_t add = 0;
    if (__builtin_mul_overflow(n_seq, n_frames, &add) || add > s->capacity - s->count)
        return bad_arg("seqik_align_stats_add", "more frames than the capacity");
    // the layout is judged before the first HIP call: a refused call leaves the handle and the device untouched
    int64_t pc = n_frames * 15, pr = 3, pf = 15;  // (n_frames <= capacity: no overflow)
    if (layout) { pc = layout->pose_chain; pr = layout->pose_row; pf = layout->pose_frame; }
    size_t stage_bytes = 0;
    if (!pose_on_device) {
        // host memory is staged as ONE contiguous piece of n_seq * n_legs chain strides (as seqik_stream_open's slabs
        // are), so every element the kernel addresses must lie inside its chain's stride
        int64_t rows = 0, frames = 0, last = 0;
        const bool ok = pc > 0 && pr > 0 && pf > 0 && !__builtin_mul_overflow((int64_t)4, pr, &rows) &&
                        !__builtin_mul_overflow(n_frames - 1, pf, &frames) &&
                        !__builtin_add_overflow(rows, frames, &last) && !__builtin_add_overflow(last, (int64_t)3, &last) &&
                        last <= pc;
        if (!ok)
            return bad_arg("seqik_align_stats_add",
                           "host layout: all three pose strides must be > 0 and every key point of a chain must lie "
                           "inside its chain stride (4*pose_row + (n_frames-1)*pose_frame + 3 <= pose_chain)");
        if (__builtin_mul_overflow((size_t)pc, (size_t)n_seq * (size_t)s->n_legs, &stage_bytes) ||
            __builtin_mul_overflow(stage_bytes, sizeof(double), &stage_bytes))
            return bad_arg("seqik_align_stats_add", "host layout: the slab's size overflows");
    } else {  // device memory: the caller owns the extent
        if (pc < 0 || pr <= 0 || pf <= 0) return bad_arg("seqik_align_stats_add", "layout strides must be positive");
        if (pc == 0 && (n_seq > 1 || s->n_legs > 1))
            return bad_arg("seqik_align_stats_add", "device layout: pose_chain must be > 0 for more than one chain");
    }
    seqik::DeviceScope scope;
    HIP_TRY(scope.enter(s->device));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const double *d_pose = pose;
    if (!pose_on_device) {
        const size_t bytes = stage_bytes;
        if (bytes > s->stage_bytes) {
            if (s->d_stage) { HIP_TRY(hipStreamSynchronize(stream)); (void)hipFree(s->d_stage); s->d_stage = nullptr; s->stage_bytes = 0; }
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s->d_stage), bytes));
            s->stage_bytes = bytes;
        }
        HIP_TRY(hipMemcpyAsync(s->d_stage, pose, bytes, hipMemcpyHostToDevice, stream));
        d_pose = s->d_stage;
    }
    const int64_t total = add * s->n_legs;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(seqik_align_extract_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_pose, n_seq, s->n_legs,
                       n_frames, pc, pr, pf, s->d_series, s->capacity, s->count);
    HIP_TRY(hipGetLastError());
    if (!pose_on_device) HIP_TRY(hipStreamSynchronize(stream));  // the staging buffer / the caller's slab may be reused
    s->count += add;
    return SEQIK_OK;
}

int seqik_align_stats_finish(SeqikAlignStats *s, const int64_t *ranks, int32_t n_ranks, double *out, void *hip_stream)
{
    if (!s || !ranks || !out) return bad_arg("seqik_align_stats_finish", "null pointer");
    if (n_ranks <= 0 || n_ranks > 16) return bad_arg("seqik_align_stats_finish", "n_ranks must be 1..16");
    if (s->count == 0) return bad_arg("seqik_align_stats_finish", "no frames were added");
    if (s->count > 0x7fffffffLL) return bad_arg("seqik_align_stats_finish", "more than 2^31 frames per leg");
    seqik::DeviceScope scope;
    HIP_TRY(scope.enter(s->device));
    // the sorts run on a pooled context's stream: what _add enqueued on the caller's stream is waited for first
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(hip_stream)));
    const int64_t count = s->count;  // every series: its first `count` of `capacity` values, one set of ranks
    return seqik::order_statistics(s->device, s->d_series, s->capacity, kSeries * s->n_legs, count, ranks, 1, n_ranks,
                                   [count](int) { return seqik::RankPick{count, 0}; }, out);
}

int seqik_align_stats_reset(SeqikAlignStats *s)
{
    if (!s) return bad_arg("seqik_align_stats_reset", "null handle");
    s->count = 0;
    return SEQIK_OK;
}

int seqik_align_stats_close(SeqikAlignStats *s) { return seqik::close_series(s); }

}  // extern "C"
