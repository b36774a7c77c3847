// TEST INFRASTRUCTURE ONLY -- not part of the product, never loaded by seqikpy_amd.
//
// Runs the per-frame rules of skip mode (csrc/seqik_gaps.hpp, `__host__ __device__`) on the HOST, one chain at a time,
// so that the CPU-only test tier can check compaction and expansion against a numpy construction and the whole contract
// against the host-run solvers (tests/harness/host_harness.hip).  Built by tests/gaps_model.py with
// `hipcc --offload-host-only`.
#include "../../sequential-inverse-kinematics_amd/csrc/seqik_gaps.hpp"
#include "../../sequential-inverse-kinematics_amd/csrc/seqik_runtime.hpp"

// the library's tile geometry (only the inline function is used; nothing of the runtime is linked) for every n_frames in
// n_first..n_last
extern "C" void harness_tile_geometry(int64_t n_first, int64_t n_last, int64_t *tile, int64_t *tiles)
{
    for (int64_t n = n_first; n <= n_last; ++n) seqik::tile_geometry(n, tile + (n - n_first), tiles + (n - n_first));
}

// pose [n][5][3] -> cpose [n][5][3], map [n]; returns n_valid (or -1 on bad flags)
extern "C" int64_t harness_gaps_compact(const double *pose, int64_t n, int32_t flags, const SeqikLegParams *leg,
                                        double *cpose, int32_t *map)
{
    if (flags & ~(SEQIK_GAPS_GENERIC | SEQIK_GAPS_AFFINE)) return -1;
    seqik::GapsLeg gl;
    seqik::make_gaps_leg(*leg, gl);
    return seqik::gaps_compact_chain(pose, n, seqik::gaps_rows(flags), gl, cpose, map);
}

extern "C" void harness_gaps_expand_f64(const int32_t *map, int64_t n, const double *compact, int32_t width, double *out)
{
    seqik::gaps_expand_chain<double>(map, n, compact, width, __builtin_nan(""), out);
}

extern "C" void harness_gaps_expand_i32(const int32_t *map, int64_t n, const int32_t *compact, int32_t width, int32_t fill,
                                        int32_t *out)
{
    seqik::gaps_expand_chain<int32_t>(map, n, compact, width, fill, out);
}
