// TEST INFRASTRUCTURE ONLY -- not part of the product, never loaded by seqikpy_amd.
//
// Runs the link-frames device function (csrc/seqik_frames.hpp, `__host__ __device__`) on the HOST, one leg-frame after
// the other, so that the CPU-only test tier can compare it bit for bit with the forward kinematics (fk_harness.hip) and,
// within a tolerance, with the IKPy stand-in; the GPU tier compares the kernel with it bit for bit.  Built by
// tests/test_link_frames.py with `hipcc --offload-host-only`.
#include "../../sequential-inverse-kinematics_amd/csrc/seqik_frames.hpp"
#include "staged_pass.hpp"

// angles [n][7] (DOFS order), origin nullable [n][3], frames [n][9][3][4]
extern "C" int harness_link_frames(const double *angles, int64_t n, const SeqikLegParams *leg, int32_t kind,
                                   const double *origin, double *frames)
{
    if (kind != seqik::FK_KIND_SEQ && kind != seqik::FK_KIND_GENERIC) return SEQIK_ERR_BAD_ARG;
    seqik::FkLeg fl;
    seqik::make_fk_leg(*leg, fl);
    for (int64_t i = 0; i < n; ++i) {
        const double *o = origin ? origin + i * 3 : nullptr;
        double *out = frames + i * seqik::kFramesRow;
        if (kind == seqik::FK_KIND_SEQ) seqik::link_frames_leg_frame<seqik::FK_KIND_SEQ>(fl, angles + i * 7, o, out);
        else seqik::link_frames_leg_frame<seqik::FK_KIND_GENERIC>(fl, angles + i * 7, o, out);
    }
    return SEQIK_OK;
}

// The kernel's staged pass on the host (staged_pass.hpp), n a multiple of 16: must equal harness_link_frames bit for bit.
extern "C" int harness_link_frames_staged(const double *angles, int64_t n, const SeqikLegParams *leg, int32_t kind,
                                          const double *origin, double *frames)
{
    if ((kind != seqik::FK_KIND_SEQ && kind != seqik::FK_KIND_GENERIC) || n % 16) return SEQIK_ERR_BAD_ARG;
    seqik::FkLeg fl;
    seqik::make_fk_leg(*leg, fl);
    staged_pass_host<seqik::kFramesQuad>(n, frames, [&](int64_t rec, seqik::QuadSink<seqik::kFramesQuad> &sink) {
        const double *o = origin ? origin + rec * 3 : nullptr;
        if (kind == seqik::FK_KIND_SEQ) seqik::link_frames_walk<seqik::FK_KIND_SEQ>(fl, angles + rec * 7, o, sink);
        else seqik::link_frames_walk<seqik::FK_KIND_GENERIC>(fl, angles + rec * 7, o, sink);
    });
    return SEQIK_OK;
}
