// seqik_order_stats.hpp -- what the two statistics units share (seqik_align.hip: seven series per leg; seqik_head_align.hip:
// five per side of the head): the handle that holds the extracted series, and the order statistics of those series -- one
// full-width hipCUB radix sort per series and a kernel that picks the requested ranks.  The extraction kernels and what a
// series means stay in the units.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <new>
#include <stdint.h>

#include "seqik_runtime.hpp"

namespace {  // (a kernel of the unit that includes this, like the unit's own)

// out[r] = sorted[min(max(ranks[r], 0), limit - 1)]: ranks of ONE sorted series, which counts `limit` values
__global__ void seqik_head_align_pick_kernel(const double *sorted, int64_t limit, const int64_t *ranks, int32_t n_ranks,
                                             double *out)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_ranks) return;
    int64_t k = ranks[r];
    if (k < 0) k = 0;
    if (k > limit - 1) k = limit - 1;  // limit >= 1 (checked by the caller): 0 <= k < limit <= n
    out[r] = sorted[k];
}

}  // namespace

namespace seqik {

// ---- the handle: a statistics handle derives from this ----
struct SeriesHandle {
    int device = 0;
    double *d_series = nullptr;  // the unit's layout, `doubles` values in all
};

// _open: a new Handle on the device `opt` names, with room for `doubles` series values
template <typename Handle>
int open_series(const char *who, const SeqikOptions *opt, size_t doubles, Handle **out)
{
    Handle *s = new (std::nothrow) Handle;
    if (!s) return bad_arg(who, "out of host memory");
    DeviceScope scope;
    hipError_t e = resolve_device(opt ? opt->device : -1, &s->device);
    if (e == hipSuccess) e = scope.enter(s->device);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s->d_series), sizeof(double) * doubles);
    if (e != hipSuccess) { delete s; return hip_fail(e, who); }
    *out = s;
    return SEQIK_OK;
}

// _close: the handle is deleted on its device, behind everything a caller's stream may still hold for it
template <typename Handle>
int close_series(Handle *s)
{
    if (!s) return SEQIK_OK;
    DeviceScope scope;
    (void)scope.enter(s->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(s->d_series);
    delete s;
    return SEQIK_OK;
}

// ---- order statistics ----
struct RankPick {
    int64_t limit;  // the ranks are clamped to 0 .. limit - 1, 1 <= limit <= n (values from `limit` on: +inf, or not there)
    int row;        // which row of the ranks
};

// Series i = 0 .. n_series - 1 is the n doubles at d_series + i * pitch; pick_of(i) -> RankPick says what is wanted of
// it.  h_ranks [rank_rows][n_ranks] and out [n_series][n_ranks] are host arrays.  A host-buffer call: it leases a pooled
// context, and its scratch -- ONE series' worth of sorted values and hipCUB's temporaries -- is a piece of that
// context's arena.  Each series is sorted at full width (a segmented sort would put one block on each of these huge
// segments) and its ranks are picked before the next sort reuses the buffer; the series themselves are left as they are.
// Everything that wrote the series must have completed.
template <typename PickOf>
int order_statistics(int device, const double *d_series, int64_t pitch, int n_series, int64_t n, const int64_t *h_ranks,
                     int rank_rows, int32_t n_ranks, PickOf pick_of, double *out)
{
    DeviceScope scope;
    HIP_TRY(scope.enter(device));
    size_t tmp_bytes = 0;  // (a size query: no work is enqueued)
    HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, d_series, static_cast<double *>(nullptr), (int)n, 0, 64,
                                              nullptr));
    HostCall call;
    double *d_sorted = nullptr, *d_out = nullptr;
    int64_t *d_ranks = nullptr;
    char *d_tmp = nullptr;
    call.scratch(d_sorted, (size_t)n);
    call.scratch(d_tmp, tmp_bytes);
    call.upload(d_ranks, (size_t)rank_rows * n_ranks, h_ranks);
    call.download(d_out, (size_t)n_series * n_ranks, out);
    if (int rc = call.begin(device)) return rc;
    for (int i = 0; i < n_series; ++i) {
        hipError_t e = hipcub::DeviceRadixSort::SortKeys(d_tmp, tmp_bytes, d_series + i * pitch, d_sorted, (int)n, 0, 64,
                                                         call.stream());
        if (e != hipSuccess) return hip_fail(e, "hipcub::DeviceRadixSort::SortKeys");
        const RankPick p = pick_of(i);
        hipLaunchKernelGGL(seqik_head_align_pick_kernel, dim3(1), dim3(64), 0, call.stream(), d_sorted, p.limit,
                           d_ranks + p.row * n_ranks, n_ranks, d_out + i * n_ranks);
        if (int rc = launched()) return rc;
    }
    return call.finish(SEQIK_OK);
}

}  // namespace seqik
