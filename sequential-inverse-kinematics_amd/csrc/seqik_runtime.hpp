// seqik_runtime.hpp -- host runtime shared by the translation units of the library (seqik_runtime.hip): the thread-local
// error text, the pooled contexts of the host-buffer calls and HostCall, the one helper those calls are written on; plus
// the argument checks and launch arithmetic more than one unit needs.  Host code only: no kernel is compiled from it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <math.h>
#include <vector>

#include "../../include/seqik.h"
#include "seqik_device_scope.hpp"

namespace seqik {

// ---- errors: every function sets the calling thread's message (seqik_last_error) and returns the code ----
int fail(int code, const char *fmt, const char *detail = "");  // fmt holds one %s
int hip_fail(hipError_t e, const char *what);                  // "<what>: <HIP's error string>", SEQIK_ERR_HIP
int bad_arg(const char *who, const char *msg);                 // "<who>: <msg>", SEQIK_ERR_BAD_ARG

#define HIP_TRY(expr)                                                  \
    do {                                                               \
        hipError_t e_ = (expr);                                        \
        if (e_ != hipSuccess) return seqik::hip_fail(e_, #expr);       \
    } while (0)

// SEQIK_OK, or the error of the kernel launch just made
inline int launched()
{
    HIP_TRY(hipGetLastError());
    return SEQIK_OK;
}

// ---- checks and launch arithmetic shared by the feature units ----
constexpr int kFkRow = 27;  // doubles of FK per leg-frame: the largest per-leg-frame array of any entry point

// workgroups of `waves_per_block` wavefronts that hold `waves` wavefronts
inline int64_t blocks_for(int64_t waves, int waves_per_block) { return (waves + waves_per_block - 1) / waves_per_block; }

// n_seq * n_legs * n_frames into *n_total; the byte count of `row` doubles per leg-frame must fit in 63 bits
inline int leg_frames_fit(const char *who, int64_t n_seq, int32_t n_legs, int64_t n_frames, int64_t *n_total,
                          int row = kFkRow)
{
    const int64_t lim = INT64_MAX / (8 * row);
    if (n_seq != 0 && n_frames != 0 && (n_seq > lim / n_legs || n_seq * n_legs > lim / n_frames))
        return bad_arg(who, "too many leg-frames");
    *n_total = n_seq * n_legs * n_frames;
    return SEQIK_OK;
}

inline int check_segments(const char *who, const SeqikLegParams *legs, int32_t n_legs)
{
    for (int l = 0; l < n_legs; ++l)
        for (int k = 0; k < 4; ++k)
            if (!isfinite(legs[l].seg[k])) return bad_arg(who, "non-finite segment length");
    return SEQIK_OK;
}

// The argument rules of every head / antenna entry point (seqik_head.hip, seqik_head_align.hip): one neck or one per
// frame, at least one key point per side, two for the antenna angles.
inline int check_head_args(const char *who, const void *r_head, const void *l_head, const void *neck, const void *angles,
                           int64_t n_frames, int64_t neck_stride, int32_t n_points, int32_t compute_ant)
{
    if (!r_head || !l_head || !neck || !angles) return bad_arg(who, "null pointer");
    if (n_frames < 0 || n_frames > INT64_MAX / (8 * 3 * (int64_t)(n_points > 0 ? n_points : 1)))
        return bad_arg(who, "n_frames is negative or too large");
    if (neck_stride != 0 && neck_stride != 3) return bad_arg(who, "neck_stride must be 0 or 3");
    if (n_points < 1) return bad_arg(who, "n_points must be at least 1");
    if (compute_ant && n_points < 2)
        return bad_arg(who, "the antenna angles need two key points per side (antenna base and tip); pass "
                            "compute_ant = 0 for single-point records");
    return SEQIK_OK;
}

// Tiles of F = 64 k frames of one chain for the one-wavefront-per-tile passes (seqik_gaps.hip, seqik_resample.hip): k = 1
// unless a chain has more than 65 536 frames, then as small as keeps a chain at <= kMaxTiles tiles (their scan kernels
// hold a chain's tiles in 16 rows of 64 lanes).
constexpr int kMaxTiles = 1024;
inline void tile_geometry(int64_t n_frames, int64_t *tile, int64_t *tiles)
{
    const int64_t blocks64 = (n_frames + 63) / 64;
    *tile = 64 * ((blocks64 + kMaxTiles - 1) / kMaxTiles);  // k >= 1
    *tiles = (n_frames + *tile - 1) / *tile;
}

// ---- pooled contexts ----
// Context of a host-buffer call: a stream and one grow-only device arena that the call's device buffers are carved
// from.  Contexts are pooled per device: a call takes a free one (or makes one) and gives it back, so repeated calls
// neither create streams nor call hipMalloc / hipFree (which drains the device), and -- because the stream lives on --
// the solver's hand-off workspace keyed by it is reused instead of stranded.  Concurrent host threads get distinct
// contexts; seqik_release_workspaces() frees the idle ones.
struct HostCtx {
    int device = -1;
    hipStream_t stream = nullptr;
    char *arena = nullptr;
    size_t arena_bytes = 0;
    bool busy = false;
};
int acquire_ctx(HostCtx **out);            // a context of the CURRENT device
void release_ctx(HostCtx *c);
int ctx_reserve(HostCtx *c, size_t bytes);  // arena of at least `bytes` (may synchronise the stream and reallocate)
// seqik_release_workspaces(): frees every idle context; *any_busy = a call is running on another thread
int release_idle_contexts(bool *any_busy);

// One host-buffer call.  The entry point DECLARES its device buffers -- each once: element type, count, and the host
// array to upload from and / or download to -- and then
//     begin(device)   enters the device, leases a context, reserves the arena ONCE for the sum of what was declared,
//                     assigns the device pointers from that same list, and enqueues the uploads and fills in
//                     declaration order;
//     stream()        is where the entry point enqueues its kernels (the _device entry point);
//     finish(rc)      rc != SEQIK_OK: returns it; else enqueues the downloads in declaration order and synchronises.
// A buffer whose count is 0, or whose host array was declared and is null (an optional output the caller did not ask
// for), takes no bytes and its device pointer is null.  On every path out, failures included, the destructor
// synchronises the stream before the context returns to the pool: copies and kernels queued so far may still be using
// the arena or the caller's arrays.
class HostCall {
public:
    struct Buf {
        void **dev;
        size_t bytes, down_bytes;
        const void *up;
        void *down;
        int fill;  // byte value of a hipMemsetAsync in front of the kernels, -1: none
        Buf &filled(int byte) { fill = byte; return *this; }
    };
    // device only
    template <typename T> Buf &scratch(T *&dev, size_t count) { return add(dev, count, true, nullptr, nullptr, count); }
    // host -> device before the kernels; null `from`: absent
    template <typename T> Buf &upload(T *&dev, size_t count, const T *from) { return add(dev, count, from != nullptr, from, nullptr, count); }
    // device -> host behind the kernels (the first down_count elements); null `to`: absent
    template <typename T> Buf &download(T *&dev, size_t count, T *to) { return add(dev, count, to != nullptr, nullptr, to, count); }
    template <typename T> Buf &download(T *&dev, size_t count, T *to, size_t down_count) { return add(dev, count, to != nullptr, nullptr, to, down_count); }
    // as scratch (always there), downloaded when `to` is not null
    template <typename T> Buf &produce(T *&dev, size_t count, T *to) { return add(dev, count, true, nullptr, to, count); }
    // downloaded to `host`, and uploaded from it first when `upload_first`
    template <typename T> Buf &inout(T *&dev, size_t count, T *host, bool upload_first) { return add(dev, count, host != nullptr, upload_first ? host : nullptr, host, count); }

    int begin(int device);
    hipStream_t stream() const { return ctx_->stream; }
    int finish(int rc);
    ~HostCall();

private:
    template <typename T>
    Buf &add(T *&dev, size_t count, bool present, const void *up, void *down, size_t down_count)
    {
        // (the caller's T * is written as a void * in begin(), the hipMalloc idiom: every T here is an object type whose
        // pointers share void *'s representation, and begin() is compiled in another translation unit)
        dev = nullptr;
        if (bufs_.empty()) bufs_.reserve(16);  // one allocation per call: no entry point declares more
        const size_t n = present ? count : 0;
        bufs_.push_back(Buf{reinterpret_cast<void **>(&dev), sizeof(T) * n, sizeof(T) * (n ? down_count : 0),
                            n ? up : nullptr, n ? down : nullptr, -1});
        return bufs_.back();
    }
    std::vector<Buf> bufs_;
    DeviceScope scope_;
    HostCtx *ctx_ = nullptr;
};

}  // namespace seqik

extern "C" void seqik_set_error(int code, const char *msg);
