// seqik_resample.hip -- PCHIP resampling of joint-angle records: the C ABI entry points of include/seqik_resample.h.
// The kernels, argument checks and launch code are in seqik_resample_kernels.hpp (shared with seqik_resample_der.hip).
#include "seqik_resample_kernels.hpp"

extern "C" {

int64_t seqik_resample_count(int64_t n_frames, double original_ts, double new_ts)
{
    return count_checked("seqik_resample_count", n_frames, original_ts, new_ts);
}

size_t seqik_resample_workspace_bytes(int64_t n_chains, int64_t n_frames, int32_t flags)
{
    if (!(flags & SEQIK_RESAMPLE_BRIDGE) || n_chains <= 0 || n_frames <= 0) return 0;
    return (size_t)n_chains * (size_t)n_frames * 2 * sizeof(int32_t);
}

int seqik_resample_pchip_device(const double *d_y, int64_t n_chains, int64_t n_frames, int32_t width,
                                double original_ts, double new_ts, int32_t flags, int32_t max_gap, double *d_out,
                                int64_t n_out, void *d_workspace, void *hip_stream)
{
    const char *who = "seqik_resample_pchip_device";
    int rc = resample_validate(who, d_y, n_chains, n_frames, width, original_ts, new_ts, flags, d_out, n_out);
    if (rc != SEQIK_OK) return rc;
    return resample_enqueue<false>(who, d_y, n_chains, n_frames, width, original_ts, new_ts, flags, max_gap, d_out, nullptr,
                                   nullptr, n_out, d_workspace, hip_stream);
}

int seqik_resample_pchip(const double *y, int64_t n_chains, int64_t n_frames, int32_t width, double original_ts,
                         double new_ts, int32_t flags, int32_t max_gap, double *out, int64_t n_out, int32_t device)
{
    int rc = resample_validate("seqik_resample_pchip", y, n_chains, n_frames, width, original_ts, new_ts, flags, out, n_out);
    if (rc != SEQIK_OK) return rc;
    if (n_chains == 0) return SEQIK_OK;
    const size_t n_rows = (size_t)width * (size_t)n_chains;
    seqik::HostCall call;
    double *d_y, *d_out;
    char *d_ws;
    call.upload(d_y, n_rows * (size_t)n_frames, y);
    call.download(d_out, n_rows * (size_t)n_out, out);
    call.scratch(d_ws, seqik_resample_workspace_bytes(n_chains, n_frames, flags));
    if ((rc = call.begin(device)) != SEQIK_OK) return rc;
    return call.finish(seqik_resample_pchip_device(d_y, n_chains, n_frames, width, original_ts, new_ts, flags, max_gap, d_out,
                                                   n_out, d_ws, call.stream()));
}

}  // extern "C"
