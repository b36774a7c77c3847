// TEST INFRASTRUCTURE ONLY -- not part of the product, never loaded by seqikpy_amd.
//
// Runs the forward-kinematics device function (csrc/seqik_fk.hpp, `__host__ __device__`) on the HOST, one leg-frame
// after the other, so that the CPU-only test tier can compare it bit for bit with the FK rows the solvers' device code
// writes (tests/harness/host_harness.hip) and with the oracle.  Built by tests/test_forward_kinematics.py with
// `hipcc --offload-host-only`.  Also hands out the launch plan of the angle-map units (csrc/seqik_leg_map.hpp: host code).
#include "../../sequential-inverse-kinematics_amd/csrc/seqik_leg_map.hpp"

// angles [n][7] (DOFS order), origin nullable [n][origin_stride] (15: a pose array, its key point 0; 3: origins),
// fk [n][9][3], dist nullable [n][4] (needs origin_stride 15: measured against that pose)
extern "C" int harness_fk(const double *angles, int64_t n, const SeqikLegParams *leg, int32_t kind, const double *origin,
                          int64_t origin_stride, double *fk, double *dist)
{
    if (kind != seqik::FK_KIND_SEQ && kind != seqik::FK_KIND_GENERIC) return SEQIK_ERR_BAD_ARG;
    if (dist && (!origin || origin_stride != 15)) return SEQIK_ERR_BAD_ARG;
    seqik::FkLeg fl;
    seqik::make_fk_leg(*leg, fl);
    for (int64_t i = 0; i < n; ++i) {
        const double *o = origin ? origin + i * origin_stride : nullptr;
        if (kind == seqik::FK_KIND_SEQ) seqik::fk_leg_frame<seqik::FK_KIND_SEQ>(fl, angles + i * 7, o, fk + i * 27);
        else seqik::fk_leg_frame<seqik::FK_KIND_GENERIC>(fl, angles + i * 7, o, fk + i * 27);
        if (dist) seqik::fk_fit_distances(fk + i * 27, o, dist + i * 4);
    }
    return SEQIK_OK;
}

// plan_leg_map as the entry points call it -> out [4]: staged, threads per workgroup, workgroups, bytes of LDS
extern "C" void harness_leg_map_plan(const char *prefix, int64_t n_total, int32_t staged_allowed, int32_t max_block_per_lane,
                                     int32_t max_block_staged, int32_t lds_doubles_per_wave, int64_t *out)
{
    const seqik::LegMapPlan p = seqik::plan_leg_map(prefix, n_total, staged_allowed != 0, max_block_per_lane,
                                                    max_block_staged, lds_doubles_per_wave);
    out[0] = p.staged; out[1] = p.block; out[2] = p.blocks; out[3] = (int64_t)p.lds_bytes;
}
