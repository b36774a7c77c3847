// seqik_head_align.hpp -- the per-element rules of the antenna alignment (include/seqik_head_align.h): the two
// distances AlignPose.align_head reduces, its stationary-frame test, its per-frame map, and the head / antenna angles of
// one RAW frame (map, then the closed forms of seqik_head.hpp unchanged).  `__host__ __device__`: the kernels of
// seqik_head_align.hip and tests/harness/head_align_harness.hip run the same text.
//
// Everything here is pinned to numpy bit for bit, so no product is fused into a sum: the library's flag set
// (-ffp-contract=off) keeps `a * b + c` as two rounded operations, and nothing below calls an fma.
#pragma once
#include "seqik_head.hpp"
#include "../../include/seqik_head_align.h"

namespace seqik {

constexpr int kHeadSeries = 5;  // per side: base x, y, z and d over the stationary set, len over all frames

// np.linalg.norm(p - q) of two 3-vectors: sqrt(add.reduce(v * v)) = sqrt((dx*dx + dy*dy) + dz*dz)
SEQIK_HD double head_norm3(double dx, double dy, double dz) { return sqrt((dx * dx + dy * dy) + dz * dz); }

// d: antenna base to the middle of the first and the last thorax key point (thorax_mid_pts, alignment.py)
SEQIK_HD double head_base_to_thorax(const double *base, const double *thorax_first, const double *thorax_last)
{
    const double mx = 0.5 * (thorax_first[0] + thorax_last[0]), my = 0.5 * (thorax_first[1] + thorax_last[1]),
                 mz = 0.5 * (thorax_first[2] + thorax_last[2]);
    return head_norm3(base[0] - mx, base[1] - my, base[2] - mz);
}

// len: antenna base to antenna tip, np.linalg.norm(np.diff(head, axis=1), axis=2)[:, 0]
SEQIK_HD double head_antenna_length(const double *base, const double *tip)
{
    return head_norm3(tip[0] - base[0], tip[1] - base[1], tip[2] - base[2]);
}

// frame i is stationary: np.diff(np.diff(d))[i] < threshold.  Signed, not absolute (the reference's quirk); false when
// any of the three distances is NaN.
SEQIK_HD bool head_is_stationary(double d0, double d1, double d2, double threshold)
{
    return (d2 - d1) - (d1 - d0) < threshold;
}

// aligned = (raw - origin) * scale + template_base: subtract, multiply, add, each rounded
SEQIK_HD void head_align_point(const double *raw, const SeqikHeadAffine &af, double scale, double *out)
{
#pragma unroll
    for (int a = 0; a < 3; ++a) out[a] = (raw[a] - af.origin[a]) * scale + af.template_base[a];
}

// One side's record: base with scale_base, tip (n_points >= 2) with scale_tip.  out: 6 doubles (3 used for one point).
SEQIK_HD void head_align_record(const double *raw, int n_points, const SeqikHeadAffine &af, double *out)
{
    head_align_point(raw, af, af.scale_base, out);
    if (n_points >= 2) head_align_point(raw + 3, af, af.scale_tip, out + 3);
}

// The seven angles of one RAW frame: rr / lr = the frame's raw records (right / left), affine[0] = R, affine[1] = L.
// ra / la receive the aligned records (6 doubles each); the rest as head_angles_compute, which sees exactly the values
// AlignPose.align_head would have stored.
SEQIK_HD void head_angles_raw_compute(const double *rr, const double *lr, int n_points, const SeqikHeadAffine *affine,
                                      const double *neck, double rest_head_pitch, double rest_antenna_pitch,
                                      bool compute_ant, double *out, const double *roll_given, double *ra, double *la)
{
    head_align_record(rr, n_points, affine[0], ra);
    head_align_record(lr, n_points, affine[1], la);
    head_angles_compute(ra, la, neck, rest_head_pitch, rest_antenna_pitch, compute_ant, out, roll_given);
}

}  // namespace seqik
