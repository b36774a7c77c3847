// seqik_runtime.hip -- host runtime of libseqik_hip.so (seqik_runtime.hpp): the thread-local error text, the pool of
// host-call contexts and HostCall.  No kernels: an edit here changes no device code.
#include <stdio.h>
#include <mutex>

#include "seqik_runtime.hpp"

namespace seqik {

namespace {
thread_local char g_err[512] = "";
std::mutex g_ctx_mutex;
std::vector<HostCtx *> g_ctx;
size_t padded(size_t bytes) { return (bytes + 255) & ~(size_t)255; }  // arena pieces are 256-byte aligned
}  // namespace

int fail(int code, const char *fmt, const char *detail)
{
    snprintf(g_err, sizeof(g_err), fmt, detail);
    return code;
}

int hip_fail(hipError_t e, const char *what)
{
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return SEQIK_ERR_HIP;
}

int bad_arg(const char *who, const char *msg)
{
    snprintf(g_err, sizeof(g_err), "%s: %s", who, msg);
    return SEQIK_ERR_BAD_ARG;
}

int acquire_ctx(HostCtx **out)
{
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    for (HostCtx *c : g_ctx)
        if (c->device == dev && !c->busy) { c->busy = true; *out = c; return SEQIK_OK; }
    HostCtx *c = new HostCtx;
    c->device = dev;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return hip_fail(e, "hipStreamCreate"); }
    c->busy = true;
    g_ctx.push_back(c);
    *out = c;
    return SEQIK_OK;
}

void release_ctx(HostCtx *c)
{
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    c->busy = false;
}

int ctx_reserve(HostCtx *c, size_t bytes)
{
    if (c->arena_bytes >= bytes) return SEQIK_OK;
    if (c->arena) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipFree(c->arena));
        c->arena = nullptr;
        c->arena_bytes = 0;
    }
    const size_t want = bytes + bytes / 8;  // a little head room: slightly longer recordings do not reallocate
    if (hipMalloc(reinterpret_cast<void **>(&c->arena), want) == hipSuccess) { c->arena_bytes = want; return SEQIK_OK; }
    (void)hipGetLastError();
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->arena), bytes));
    c->arena_bytes = bytes;
    return SEQIK_OK;
}

int release_idle_contexts(bool *any_busy)
{
    *any_busy = false;
    std::lock_guard<std::mutex> ctx_lock(g_ctx_mutex);
    for (size_t i = 0; i < g_ctx.size();) {
        HostCtx *c = g_ctx[i];
        if (c->busy) { *any_busy = true; ++i; continue; }  // a call is running on another thread
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->arena) HIP_TRY(hipFree(c->arena));
        HIP_TRY(hipStreamDestroy(c->stream));
        delete c;
        g_ctx.erase(g_ctx.begin() + i);
    }
    return SEQIK_OK;
}

int HostCall::begin(int device)
{
    HIP_TRY(scope_.enter(device));
    if (int rc = acquire_ctx(&ctx_)) return rc;
    size_t need = 0;
    for (const Buf &b : bufs_) need += padded(b.bytes);
    if (int rc = ctx_reserve(ctx_, need)) return rc;
    char *p = ctx_->arena;
    for (const Buf &b : bufs_) {
        *b.dev = b.bytes ? p : nullptr;
        p += padded(b.bytes);
    }
    for (const Buf &b : bufs_) {
        if (b.up) HIP_TRY(hipMemcpyAsync(*b.dev, b.up, b.bytes, hipMemcpyHostToDevice, ctx_->stream));
        if (b.bytes && b.fill >= 0) HIP_TRY(hipMemsetAsync(*b.dev, b.fill, b.bytes, ctx_->stream));
    }
    return SEQIK_OK;
}

int HostCall::finish(int rc)
{
    if (rc != SEQIK_OK) return rc;
    for (const Buf &b : bufs_)
        if (b.down) HIP_TRY(hipMemcpyAsync(b.down, *b.dev, b.down_bytes, hipMemcpyDeviceToHost, ctx_->stream));
    HIP_TRY(hipStreamSynchronize(ctx_->stream));
    return SEQIK_OK;
}

HostCall::~HostCall()
{
    if (!ctx_) return;
    (void)hipStreamSynchronize(ctx_->stream);
    release_ctx(ctx_);
}

}  // namespace seqik

extern "C" {

const char *seqik_last_error(void) { return seqik::g_err; }

// for callers that compose their own text
void seqik_set_error(int code, const char *msg) { (void)seqik::fail(code, "%s", msg); }

}  // extern "C"
