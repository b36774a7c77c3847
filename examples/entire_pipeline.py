"""End-to-end pipeline on MI355X: align -> head / antenna angles -> sequential leg IK -> one pickle.

Counterpart of the reference's examples/example_entire_pipeline.py (which notes "takes about 40 minutes"
for the shipped 6000-frame recording).  Input: a pickled anipose pose (pose3d.h5) or an already
converted segment dictionary (converted_dict.pkl) under --path.

    python examples/entire_pipeline.py -p <dir with pose3d.* or converted_dict.pkl> [--serial] [--gpu-alignment]

--gpu-alignment: the whole-recording statistics of the alignment are taken on the GPU (legs and antennae) and the
per-frame maps run inside the kernels, which read the RAW key points: legs and head go to the GPU in one submission
(pipeline.run_body_ik).  The files written are the same, bit for bit.
"""
import argparse
import os
import sys
import time
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sequential-inverse-kinematics_amd"))

import numpy as np  # noqa: E402

from seqikpy_amd.alignment import AlignPose, convert_from_anipose_to_dict  # noqa: E402
from seqikpy_amd.data import BOUNDS, INITIAL_ANGLES, NMF_TEMPLATE, PTS2ALIGN  # noqa: E402
from seqikpy_amd.head_inverse_kinematics import ANGLE_NAMES, HeadInverseKinematics  # noqa: E402
from seqikpy_amd.kinematic_chain import KinematicChainSeq  # noqa: E402
from seqikpy_amd.leg_inverse_kinematics import LegInvKinSeq  # noqa: E402
from seqikpy_amd.utils import save_file  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-p", "--path", required=True)
    ap.add_argument("--frame-chunks", action="store_true", help="(default since round 6; kept for older command lines)")
    ap.add_argument("--serial", action="store_true",
                    help="walk every recording frame by frame as the reference does (frame_parallel=False: bit-exact restatement of "
                         "the reference) instead of the default, concurrently solved and verified frame chunks (frame_parallel="
                         "'auto': 10-70x faster for one recording, equal to the serial walk to ~1e-5 rad)")
    ap.add_argument("--gpu-alignment", action="store_true",
                    help="alignment statistics on the GPU and the per-frame maps fused into the kernels (raw key points "
                         "in, one submission for legs and head); same output files")
    args = ap.parse_args()
    data_path = Path(args.path)
    t0 = time.time()
    if list(data_path.rglob("converted_dict.pkl")):
        align = AlignPose.from_file_path(data_path, file_name="converted_dict.pkl", legs_list=["RF", "LF"],
                                         include_claw=False, body_template=NMF_TEMPLATE, log_level="INFO")
    else:
        align = AlignPose.from_file_path(data_path, file_name="pose3d.*", legs_list=["RF", "LF"],
                                         convert_func=convert_from_anipose_to_dict, pts2align=PTS2ALIGN,
                                         include_claw=False, body_template=NMF_TEMPLATE, log_level="INFO")
    if args.gpu_alignment:
        run_fused(align, data_path, frame_parallel=False if args.serial else "auto")
        print(f"Total time taken to execute the code: {time.time() - t0:.2f} s")
        return
    aligned_pos = align.align_pose(export_path=data_path)
    head = HeadInverseKinematics(aligned_pos=aligned_pos, body_template=NMF_TEMPLATE, log_level="INFO")
    head_angles = head.compute_head_angles(export_path=data_path)
    seq_ik = LegInvKinSeq(aligned_pos=aligned_pos,
                          kinematic_chain_class=KinematicChainSeq(bounds_dof=BOUNDS, legs_list=["RF", "LF"], body_size=None),
                          initial_angles=INITIAL_ANGLES, log_level="INFO")
    leg_angles, forward_kinematics = seq_ik.run_ik_and_fk(export_path=data_path, frame_parallel=False if args.serial else "auto")
    save_file(data_path / "body_joint_angles.pkl", {**head_angles, **leg_angles})
    print(f"Total time taken to execute the code: {time.time() - t0:.2f} s")


def run_fused(align, data_path, frame_parallel):
    """--gpu-alignment: constants from the GPU statistics, raw key points to the kernels, the files of the default run."""
    from seqikpy_amd.pipeline import run_body_ik
    raw = align.pose_data_dict
    leg_affine, head_affine = align.leg_affines(on_gpu=True), align.head_affines(on_gpu=True)
    aligned_head = {}
    body, forward_kinematics = run_body_ik(raw, KinematicChainSeq(bounds_dof=BOUNDS, legs_list=["RF", "LF"], body_size=None),
                                           NMF_TEMPLATE, INITIAL_ANGLES, frame_parallel=frame_parallel,
                                           leg_affine=leg_affine, head_affine=head_affine, aligned_head=aligned_head)
    aligned_pos = {}
    for segment, array in raw.items():   # the order and content of AlignPose.align_pose()
        if "leg" in segment:
            fixed, scale, template = leg_affine[segment[:2]]
            aligned_pos[segment] = np.empty_like(array)
            aligned_pos[segment][:, 0, :] = np.zeros_like(array[:, 0, :]) + template
            aligned_pos[segment][:, 1:5, :] = (array[:, 1:5, :] - fixed) * scale + template
        elif "head" in segment:
            aligned_pos[segment] = aligned_head[segment]
    aligned_pos["Neck"] = aligned_head["Neck"]
    head_angles = {k: body[k] for k in ANGLE_NAMES}
    leg_angles = {k: v for k, v in body.items() if k not in head_angles}
    save_file(data_path / "pose3d_aligned.pkl", aligned_pos)
    save_file(data_path / "head_joint_angles.pkl", head_angles)
    save_file(data_path / "leg_joint_angles.pkl", leg_angles)
    save_file(data_path / "forward_kinematics.pkl", forward_kinematics)
    save_file(data_path / "body_joint_angles.pkl", {**head_angles, **leg_angles})


if __name__ == "__main__":
    main()
