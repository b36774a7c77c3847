// TEST INFRASTRUCTURE ONLY -- not part of the product, never loaded by seqikpy_amd.
//
// Runs the per-element rules of the antenna alignment (csrc/seqik_head_align.hpp, `__host__ __device__`) on the HOST, one
// frame after the other, so that the CPU-only test tier can compare them bit for bit with numpy and with the reference's
// aligned output; the GPU tier compares the kernels with numpy on the host.  Also hands out the launch plan of the head
// kernels (csrc/seqik_head_launch.hpp, host code).  Built by tests/test_head_alignment.py with `hipcc --offload-host-only`.
#include "../../sequential-inverse-kinematics_amd/csrc/seqik_head_align.hpp"
#include "../../sequential-inverse-kinematics_amd/csrc/seqik_head_launch.hpp"

// plan_head as the head entry points call it (the pointers are only looked at, never followed; r_aligned / l_aligned:
// the fused kernel's optional outputs, null for the plain one) -> out [2]: workgroups, seqik::HeadVariant
extern "C" void harness_head_plan(int64_t n_frames, int32_t n_points, int32_t compute_ant, const double *r_head,
                                  const double *l_head, const double *head_roll, const double *r_aligned,
                                  const double *l_aligned, int64_t *out)
{
    const seqik::HeadPlan p = seqik::plan_head(
        seqik::head_args(r_head, l_head, n_frames, n_points, nullptr, 0, 0.0, 0.0, compute_ant, head_roll, nullptr), r_aligned,
        l_aligned);
    out[0] = p.blocks;
    out[1] = p.variant;
}

// One side.  head [n][n_points][3], thorax [n][n_thorax_points][3] -> d [n], len [n], mask [n] (1 = stationary; the last
// two frames are no candidates); returns the number of stationary frames.
extern "C" int64_t harness_head_align_series(const double *head, const double *thorax, int64_t n, int32_t n_points,
                                             int32_t n_thorax_points, double threshold, double *d, double *len,
                                             uint8_t *mask)
{
    const int64_t rec = 3 * (int64_t)n_points, th_rec = 3 * (int64_t)n_thorax_points;
    for (int64_t t = 0; t < n; ++t) {
        const double *p = head + t * rec, *th = thorax + t * th_rec;
        d[t] = seqik::head_base_to_thorax(p, th, th + th_rec - 3);
        len[t] = seqik::head_antenna_length(p, p + 3);
    }
    int64_t count = 0;
    for (int64_t t = 0; t < n; ++t) {
        mask[t] = t + 2 < n && seqik::head_is_stationary(d[t], d[t + 1], d[t + 2], threshold);
        count += mask[t];
    }
    return count;
}

// The fused rule: RAW records + affine[2] (R, L) -> angles [7][n] (rows 3..6 only with compute_ant) and the aligned
// records r_aligned / l_aligned [n][min(n_points, 2)][3].
extern "C" void harness_head_angles_raw(const double *r_head, const double *l_head, int64_t n, int32_t n_points,
                                        const double *neck, int64_t neck_stride, double rest_head_pitch,
                                        double rest_antenna_pitch, int32_t compute_ant, const double *head_roll,
                                        const SeqikHeadAffine *affine, double *angles, double *r_aligned,
                                        double *l_aligned)
{
    const int64_t rec = 3 * (int64_t)n_points;
    const int out_rec = n_points >= 2 ? 6 : 3, n_out = compute_ant ? 7 : 3;
    for (int64_t t = 0; t < n; ++t) {
        double out[7], ra[6], la[6];
        seqik::head_angles_raw_compute(r_head + t * rec, l_head + t * rec, n_points, affine, neck + t * neck_stride,
                                       rest_head_pitch, rest_antenna_pitch, compute_ant != 0, out,
                                       (compute_ant && head_roll) ? head_roll + t : nullptr, ra, la);
        for (int j = 0; j < n_out; ++j) angles[j * n + t] = out[j];
        for (int j = 0; j < out_rec; ++j) { r_aligned[t * out_rec + j] = ra[j]; l_aligned[t * out_rec + j] = la[j]; }
    }
}

// The plain head rule (csrc/seqik_head.hpp) on already aligned records, for the comparison with the fused one.
extern "C" void harness_head_angles_plain(const double *r_head, const double *l_head, int64_t n, int32_t n_points,
                                          const double *neck, int64_t neck_stride, double rest_head_pitch,
                                          double rest_antenna_pitch, int32_t compute_ant, const double *head_roll,
                                          double *angles)
{
    const seqik::HeadArgs a = seqik::head_args(r_head, l_head, n, n_points, neck, neck_stride, rest_head_pitch,
                                               rest_antenna_pitch, compute_ant, head_roll, angles);
    for (int64_t t = 0; t < n; ++t) seqik::head_angles_frame(a, t);
}
