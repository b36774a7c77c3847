// TEST INFRASTRUCTURE ONLY -- not part of the product, never loaded by seqikpy_amd.
//
// Runs the per-sample rules of the resampler's derivatives (csrc/seqik_resample.hpp: resample_sample_der /
// resample_chain_der, `__host__ __device__`) on the HOST, one chain at a time: the CPU-only tier checks them against a
// 200-bit yardstick and scipy, the GPU tier compares the kernels with them bit for bit.  Built by
// tests/test_resample_der.py with `hipcc --offload-host-only -ffp-contract=off`, like resample_harness.hip.
#include <vector>

#include "../../sequential-inverse-kinematics_amd/csrc/seqik_resample.hpp"

namespace {

seqik::ResampleParams params(int32_t n, int32_t width, double ots, double nts, int32_t flags, int32_t max_gap, int32_t n_out)
{
    seqik::ResampleParams p;
    p.ots = ots;
    p.inv_ots = 1.0 / ots;
    p.nts = nts;
    p.n_frames = n;
    p.n_out = n_out;
    p.width = width;
    p.flags = flags;
    p.max_gap = max_gap;
    return p;
}

}  // namespace

// y [n][width] -> those of value / d1 / d2 [n_out][width] that are not null
extern "C" int harness_resample_chain_der(const double *y, int32_t n, int32_t width, double ots, double nts, int32_t flags,
                                          int32_t max_gap, double *value, double *d1, double *d2, int32_t n_out)
{
    if (n < 2 || width < 1 || width > seqik::kResampleMaxWidth || (flags & ~SEQIK_RESAMPLE_BRIDGE)) return -1;
    std::vector<int32_t> prev(n), next(n);
    seqik::resample_chain_der(y, params(n, width, ots, nts, flags, max_gap, n_out), prev.data(), next.data(), value, d1, d2);
    return 0;
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
            if (bridge && prev[g] != g) continue;
            const int32_t m1 = bridge ? (g > 0 ? prev[g - 1] : -1) : g - 1;
            const int32_t p1 = bridge ? (g + 1 < n ? next[g + 1] : n) : g + 1;
            const bool hm1 = m1 >= 0, hp1 = p1 < n;
            if (!hm1 && !hp1) continue;
            const int32_t m2 = !hm1 ? -1 : (bridge ? (m1 > 0 ? prev[m1 - 1] : -1) : m1 - 1);
            const int32_t p2 = !hp1 ? n : (bridge ? (p1 + 1 < n ? next[p1 + 1] : n) : p1 + 1);
            auto knot = [&](int32_t k, bool has) {
                return seqik::PchipKnot{has ? seqik::resample_x(k, ots) : 0.0, has ? y[(int64_t)k * width + c] : 0.0, has};
            };
            out = seqik::pchip_deriv(knot(m2, hm1 && !hp1 && m2 >= 0), knot(m1, hm1), knot(g, true), knot(p1, hp1),
                                     knot(p2, !hm1 && hp1 && p2 < n));
        }
    return 0;
}
