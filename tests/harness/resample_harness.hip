// TEST INFRASTRUCTURE ONLY -- not part of the product, never loaded by seqikpy_amd.
//
// Runs the per-sample rules of PCHIP resampling (csrc/seqik_resample.hpp, `__host__ __device__`) on the HOST, one chain
// at a time, so that the CPU-only test tier can check them against scipy and the GPU tier can compare the kernels with
// them bit for bit.  Built by tests/test_resample.py with `hipcc --offload-host-only`.
#include <vector>

#include "../../sequential-inverse-kinematics_amd/csrc/seqik_resample.hpp"

// numpy's length of np.arange(0, n * ots, nts) as the rules compute it (no argument checks)
extern "C" double harness_resample_count(int64_t n, double ots, double nts)
{
    return seqik::resample_count_f64(n, ots, nts);
}

// y [n][width] -> out [n_out][width]; prev / next [n] (nullable) receive the neighbour tables in bridge mode
extern "C" int harness_resample_chain(const double *y, int32_t n, int32_t width, double ots, double nts, int32_t flags,
                                      int32_t max_gap, double *out, int32_t n_out, int32_t *prev, int32_t *next)
{
    if (n < 2 || width < 1 || width > seqik::kResampleMaxWidth || (flags & ~SEQIK_RESAMPLE_BRIDGE)) return -1;
    seqik::ResampleParams p;
    p.ots = ots;
    p.inv_ots = 1.0 / ots;
    p.nts = nts;
    p.n_frames = n;
    p.n_out = n_out;
    p.width = width;
    p.flags = flags;
    p.max_gap = max_gap;
    std::vector<int32_t> tp, tn;
    if ((flags & SEQIK_RESAMPLE_BRIDGE) && (!prev || !next)) {
        tp.resize(n);
        tn.resize(n);
        prev = tp.data();
        next = tn.data();
    }
    seqik::resample_chain(y, p, prev, next, out);
    return 0;
}

// a strided subset of one chain's samples: out[k][width] = sample first + k * stride (prev / next: tables made above)
extern "C" void harness_resample_samples(const double *y, int32_t n, int32_t width, double ots, double nts, int32_t flags,
                                         int32_t max_gap, const int32_t *prev, const int32_t *next, int64_t first,
                                         int64_t stride, int64_t count, double *out)
{
    seqik::ResampleParams p;
    p.ots = ots;
    p.inv_ots = 1.0 / ots;
    p.nts = nts;
    p.n_frames = n;
    p.n_out = 0;
    p.width = width;
    p.flags = flags;
    p.max_gap = max_gap;
    for (int64_t k = 0; k < count; ++k)
        for (int c = 0; c < width; ++c)
            out[k * width + c] = seqik::resample_sample(y, prev, next, p, (int32_t)(first + k * stride), c);
}

extern "C" void harness_resample_tables(const double *y, int32_t n, int32_t width, int32_t *prev, int32_t *next)
{
    seqik::resample_tables_chain(y, n, width, prev, next);
}
