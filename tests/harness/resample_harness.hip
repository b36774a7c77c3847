// TEST INFRASTRUCTURE ONLY -- not part of the product, never loaded by seqikpy_amd.
//
// Runs the per-sample rules of PCHIP resampling and of its derivatives (csrc/seqik_resample.hpp, `__host__ __device__`)
// on the HOST, one chain at a time, so that the CPU-only test tier can check them against scipy and a 200-bit yardstick
// and the GPU tier can compare the kernels with them bit for bit.  Built by tests/test_resample.py with
// `hipcc --offload-host-only -ffp-contract=off`; tests/test_resample_der.py loads the same library.
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
    std::vector<int32_t> tp, tn;
    if ((flags & SEQIK_RESAMPLE_BRIDGE) && (!prev || !next)) {
        tp.resize(n);
        tn.resize(n);
        prev = tp.data();
        next = tn.data();
    }
    seqik::resample_chain(y, seqik::resample_params(ots, nts, n, n_out, width, flags, max_gap), prev, next, out);
    return 0;
}

// y [n][width] -> those of value / d1 / d2 [n_out][width] that are not null
extern "C" int harness_resample_chain_der(const double *y, int32_t n, int32_t width, double ots, double nts, int32_t flags,
                                          int32_t max_gap, double *value, double *d1, double *d2, int32_t n_out)
{
    if (n < 2 || width < 1 || width > seqik::kResampleMaxWidth || (flags & ~SEQIK_RESAMPLE_BRIDGE)) return -1;
    std::vector<int32_t> prev(n), next(n);
    seqik::resample_chain_der(y, seqik::resample_params(ots, nts, n, n_out, width, flags, max_gap), prev.data(),
                              next.data(), value, d1, d2);
    return 0;
}

// a strided subset of one chain's samples: out[k][width] = sample first + k * stride (prev / next: tables made above)
extern "C" void harness_resample_samples(const double *y, int32_t n, int32_t width, double ots, double nts, int32_t flags,
                                         int32_t max_gap, const int32_t *prev, const int32_t *next, int64_t first,
                                         int64_t stride, int64_t count, double *out)
{
    const seqik::ResampleParams p = seqik::resample_params(ots, nts, n, 0, width, flags, max_gap);
    for (int64_t k = 0; k < count; ++k)
        for (int c = 0; c < width; ++c)
            out[k * width + c] = seqik::resample_sample(y, prev, next, p, (int32_t)(first + k * stride), c);
}

extern "C" void harness_resample_tables(const double *y, int32_t n, int32_t width, int32_t *prev, int32_t *next)
{
    seqik::resample_tables_chain(y, n, width, prev, next);
}

// pchip_deriv at every knot of y [n][width] from its neighbours (bridge mode: its VALID neighbours; a missing knot, or a
// chain with fewer than two valid ones, gets NaN) -> d [n][width]
extern "C" int harness_knot_derivatives(const double *y, int32_t n, int32_t width, double ots, int32_t flags, double *d)
{
    if (n < 2 || width < 1 || width > seqik::kResampleMaxWidth) return -1;
    const bool bridge = flags & SEQIK_RESAMPLE_BRIDGE;
    std::vector<int32_t> prev(n), next(n);
    if (bridge) seqik::resample_tables_chain(y, n, width, prev.data(), next.data());
    for (int32_t g = 0; g < n; ++g)
        for (int c = 0; c < width; ++c) {
            double &out = d[(int64_t)g * width + c];
            out = seqik::resample_nan();
            seqik::PchipNeighbours k;
            if (!seqik::resample_neighbours(prev.data(), next.data(), bridge, g, n, k)) continue;
            auto knot = [&](int32_t j, bool has) {
                return seqik::PchipKnot{has ? seqik::resample_x(j, ots) : 0.0, has ? y[(int64_t)j * width + c] : 0.0, has};
            };
            out = seqik::pchip_deriv(knot(k.m2, k.hm2), knot(k.m1, k.hm1), knot(g, true), knot(k.p1, k.hp1), knot(k.p2, k.hp2));
        }
    return 0;
}
