// seqik_resample_der.hip -- the resampled value, first and second derivative of the PCHIP interpolant: the C ABI entry
// points of include/seqik_resample_der.h.  The kernels are those of seqik_resample_kernels.hpp in their DER
// instantiation: one staging pass per tile whatever number of planes is asked for.
#include "seqik_resample_kernels.hpp"
#include "../../include/seqik_resample_der.h"

namespace {

// the checks of seqik_resample_pchip[_device], with "out" standing for the planes that were asked for
int der_validate(const char *who, const double *y, int64_t n_chains, int64_t n_frames, int32_t width, double ots, double nts,
                 int32_t flags, const double *value, const double *d1, const double *d2, int64_t n_out)
{
    if (!value && !d1 && !d2) return bad_arg(who, "out_value, out_d1 and out_d2 are all null: ask for at least one");
    return resample_validate(who, y, n_chains, n_frames, width, ots, nts, flags, value ? value : (d1 ? d1 : d2), n_out);
}

}  // namespace

extern "C" {

int seqik_resample_der_device(const double *d_y, int64_t n_chains, int64_t n_frames, int32_t width, double original_ts,
                              double new_ts, int32_t flags, int32_t max_gap, double *d_value, double *d_d1, double *d_d2,
                              int64_t n_out, void *d_workspace, void *hip_stream)
{
    const char *who = "seqik_resample_der_device";
    int rc = der_validate(who, d_y, n_chains, n_frames, width, original_ts, new_ts, flags, d_value, d_d1, d_d2, n_out);
    if (rc != SEQIK_OK) return rc;
    return resample_enqueue<true>(who, d_y, n_chains, n_frames, width, original_ts, new_ts, flags, max_gap, d_value, d_d1,
                                  d_d2, n_out, d_workspace, hip_stream);
}

int seqik_resample_der(const double *y, int64_t n_chains, int64_t n_frames, int32_t width, double original_ts,
                       double new_ts, int32_t flags, int32_t max_gap, double *out_value, double *out_d1, double *out_d2,
                       int64_t n_out, int32_t device)
{
    int rc = der_validate("seqik_resample_der", y, n_chains, n_frames, width, original_ts, new_ts, flags, out_value, out_d1,
                          out_d2, n_out);
    if (rc != SEQIK_OK) return rc;
    if (n_chains == 0) return SEQIK_OK;
    const size_t n_rows = (size_t)width * (size_t)n_chains;
    seqik::HostCall call;
    double *d_y, *d_value, *d_d1, *d_d2;
    char *d_ws;
    call.upload(d_y, n_rows * (size_t)n_frames, y);
    call.download(d_value, n_rows * (size_t)n_out, out_value);
    call.download(d_d1, n_rows * (size_t)n_out, out_d1);
    call.download(d_d2, n_rows * (size_t)n_out, out_d2);
    call.scratch(d_ws, seqik_resample_workspace_bytes(n_chains, n_frames, flags));
    if ((rc = call.begin(device)) != SEQIK_OK) return rc;
    return call.finish(seqik_resample_der_device(d_y, n_chains, n_frames, width, original_ts, new_ts, flags, max_gap, d_value,
                                                 d_d1, d_d2, n_out, d_ws, call.stream()));
}

}  // extern "C"
