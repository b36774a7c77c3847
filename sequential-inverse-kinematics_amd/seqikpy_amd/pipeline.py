"""Legs + head / antennae of one recording in ONE submission (BASELINE config 4).

The reference runs ``HeadInverseKinematics.compute_head_angles()`` and ``LegInvKinSeq.run_ik_and_fk()`` one after
the other and merges the two dictionaries into ``body_joint_angles.pkl``
(``examples/example_entire_pipeline.py:72-101``).  Here both go to the GPU together: the key points are uploaded
once, the leg kernel and the head / antenna kernel are enqueued on two HIP streams (device entry points of the C
ABI), one synchronisation, one download.  Results are the bits the two classes return separately.

torch is used for device memory and streams only.
"""
from typing import Dict, Optional, Tuple

import numpy as np

from . import _lib
from .data import DOFS, INITIAL_ANGLES
from .head_inverse_kinematics import ANGLE_NAMES, HeadInverseKinematics
from .kinematic_chain import KinematicChainSeq


def run_body_ik(aligned_pos: Dict[str, np.ndarray], kinematic_chain_class: KinematicChainSeq,
                body_template: Dict[str, np.ndarray], initial_angles: Optional[Dict] = None, device: int = -1,
                frame_parallel=None, stats: Optional[dict] = None,
                missing_key_points: str = "raise", leg_affine: Optional[Dict[str, tuple]] = None,
                head_affine: Optional[Dict[str, tuple]] = None,
                aligned_head: Optional[dict] = None) -> Tuple[Dict[str, np.ndarray], Dict[str, np.ndarray]]:
    """Returns ``(body_joint_angles, forward_kinematics)``: the 7 head / antenna angles (when ``R_head``, ``L_head``
    and ``Neck`` are present) + 7 angles per leg, and the ``"<leg>_leg" -> (N, 9, 3)`` joint positions.
    ``frame_parallel``: as ``LegInvKinSeq.run_ik_and_fk`` -- None / ``"auto"`` (default: verified frame chunks; the same
    device-side per-leg guard as every other entry point) or ``False`` (the reference's serial walk).  ``stats``: a dict
    that receives the chunk statistics of the launch.
    ``missing_key_points``: ``"raise"`` (default: a non-finite leg key point raises ``ValueError``, as scipy does in the
    reference) or ``"skip"``: every leg is solved as ``LegInvKinSeq.run_ik_and_fk(missing_key_points="skip")`` solves it
    -- frames with a non-finite key point are left out of the warm-start chain and come back as NaN angles and NaN FK
    rows (compact -> solve -> expand on the leg stream, ``_lib.solve_seq_gaps_device``).  It applies to the legs only:
    the head and antenna angles keep their behaviour in either mode (they are computed per frame, and a non-finite head
    key point gives non-finite angles for that frame).
    ``leg_affine`` (``AlignPose.leg_affines()``) and ``head_affine`` (``AlignPose.head_affines()``): with one given, that
    part of ``aligned_pos`` holds RAW key points and its alignment runs inside the kernels -- the legs through the
    solver's ``SeqikAffine`` prologue, the head through ``seqik_head_angles_raw_device`` (the neck is then the template's)
    -- still two streams, one synchronisation, one download; the results are the bits of the call on the host-aligned
    dictionary.  ``aligned_head``: a dict that receives the aligned ``R_head``, ``L_head`` and ``Neck`` the head kernel
    mapped (``head_affine`` only; what ``AlignPose.align_pose()`` returns for them)."""
    import torch
    from .leg_inverse_kinematics import default_frame_parallel
    if frame_parallel is None:
        frame_parallel = default_frame_parallel()
    if initial_angles is None:
        initial_angles = INITIAL_ANGLES
    kc = kinematic_chain_class
    segs = [(name, name.split("_")[0]) for name in aligned_pos
            if "leg" in name.lower() and f"{name.split('_')[0]}_Coxa" in kc.body_size]
    if not segs:
        raise ValueError("no leg of aligned_pos is covered by the kinematic chain's body_size")
    legs = [_lib.make_leg_params(leg, kc.bounds_dof, kc.body_size, initial_angles) for _, leg in segs]
    pose = np.stack([np.asarray(aligned_pos[name], dtype=np.float64)[:, :5, :] for name, _ in segs])[None]
    skip = _lib.check_missing_mode(missing_key_points)
    if not skip:
        _lib._check_finite(pose)
    n = pose.shape[2]
    affine = None if leg_affine is None else [_lib.make_affine(*leg_affine[leg]) for _, leg in segs]
    with_head = all(k in aligned_pos for k in (("R_head", "L_head", "Neck") if head_affine is None else ("R_head", "L_head")))
    with torch.cuda.device(device):
        leg_stream, head_stream = torch.cuda.Stream(), torch.cuda.Stream()
        d_pose = torch.from_numpy(pose).cuda(non_blocking=True)
        d_ang = torch.zeros((1, len(segs), n, 7), dtype=torch.float64, device="cuda")
        d_fk = torch.zeros((1, len(segs), n, 9, 3), dtype=torch.float64, device="cuda")
        # (allocated and zero-filled on the current stream BEFORE leg_stream waits for it: the kernels of the chunked call
        # write these statistics on leg_stream)
        d_stats = torch.zeros(_lib.N_CHUNK_STATS, dtype=torch.int32, device="cuda")
        cur = torch.cuda.current_stream()
        leg_stream.wait_stream(cur)
        if skip:
            L = len(segs)
            f64 = dict(dtype=torch.float64, device="cuda")
            gaps = dict(d_cpose=torch.empty_like(d_pose), d_map=torch.empty((1, L, n), dtype=torch.int32, device="cuda"),
                        d_n_valid=torch.empty((1, L), dtype=torch.int32, device="cuda"),
                        d_cangles=torch.empty((1, L, n, 7), **f64), d_cfk=torch.empty((1, L, n, 9, 3), **f64))
            _lib.solve_seq_gaps_device(d_pose, 1, L, n, legs, d_ang, d_fk=d_fk, stream=leg_stream,
                                       frame_chunk=-1 if frame_parallel else 0, d_chunk_stats=d_stats.data_ptr(),
                                       affine=affine, **gaps)
        else:
            _lib.solve_seq_device(d_pose.data_ptr(), 1, len(segs), n, legs, d_ang.data_ptr(), d_fk.data_ptr(),
                                  stream=leg_stream.cuda_stream, frame_chunk=-1 if frame_parallel else 0,
                                  d_chunk_stats=d_stats.data_ptr(), affine=affine)
        d_al = None
        if with_head and head_affine is not None:
            hk = HeadInverseKinematics.from_raw(aligned_pos, body_template, head_affine, log_level="ERROR")
            r, l_ = hk.raw_pos["R_head"], hk.raw_pos["L_head"]
            neck = np.ascontiguousarray(hk._template_neck()[:, 0, :])
            nh, kp = r.shape[:2]
            if kp < 2:
                raise ValueError("R_head / L_head must hold the antenna base and tip")
            d_r, d_l, d_n = (torch.from_numpy(a).cuda(non_blocking=True) for a in (r, l_, neck))
            d_head = torch.zeros((7, nh), dtype=torch.float64, device="cuda")
            if aligned_head is not None:
                d_al = [torch.zeros((nh, 2, 3), dtype=torch.float64, device="cuda") for _ in range(2)]
            head_stream.wait_stream(cur)
            _lib.head_angles_raw_device(d_r, d_l, nh, kp, d_n, 3 if (neck.shape[0] == nh and nh > 1) else 0,
                                        hk.rest_head_pitch, hk.rest_antenna_pitch, head_affine, d_head,
                                        d_r_aligned=d_al[0] if d_al else 0, d_l_aligned=d_al[1] if d_al else 0,
                                        stream=head_stream)
        elif with_head:
            hk = HeadInverseKinematics(aligned_pos, body_template, log_level="ERROR")
            r = np.ascontiguousarray(aligned_pos["R_head"], dtype=np.float64)
            l_ = np.ascontiguousarray(aligned_pos["L_head"], dtype=np.float64)
            neck = np.ascontiguousarray(np.asarray(aligned_pos["Neck"], dtype=np.float64)[:, 0, :])
            nh = r.shape[0]
            d_r, d_l, d_n = (torch.from_numpy(a).cuda(non_blocking=True) for a in (r, l_, neck))
            d_head = torch.zeros((7, nh), dtype=torch.float64, device="cuda")
            head_stream.wait_stream(cur)
            _lib._call("seqik_head_angles_device", d_r.data_ptr(), d_l.data_ptr(), nh, d_n.data_ptr(),
                       3 if (neck.shape[0] == nh and nh > 1) else 0, hk.rest_head_pitch, hk.rest_antenna_pitch, 1,
                       d_head.data_ptr(), head_stream.cuda_stream)
        leg_stream.synchronize()
        head_stream.synchronize()
        _lib.check_faults()   # the device entry points do not synchronise: a kernel fault is reported here
        ang, fk = d_ang.cpu().numpy(), d_fk.cpu().numpy()
        head = d_head.cpu().numpy() if with_head else None
        if d_al:
            aligned_head.update({"R_head": d_al[0].cpu().numpy(), "L_head": d_al[1].cpu().numpy(),
                                 "Neck": hk._template_neck()})
        if stats is not None:
            stats.update(_lib.chunk_stats_dict(d_stats.cpu().numpy()))
    body = {}
    if with_head:
        body.update({name: head[i].copy() for i, name in enumerate(ANGLE_NAMES)})
    fk_dict = {}
    for li, (name, leg) in enumerate(segs):
        for d, dof in enumerate(DOFS):
            body[f"Angle_{leg}_{dof}"] = ang[0, li, :, d].copy()
        fk_dict[name] = fk[0, li].copy()
    return body, fk_dict
