"""Leg inverse kinematics -- host-side mirror of the reference's
``seqikpy/leg_inverse_kinematics.py`` (``LegInvKinBase`` :25-133, ``LegInvKinSeq`` :136-403).

Same classes, constructor arguments, method names, dictionary outputs and exceptions; the
per-(frame, stage) ``ikpy``/``scipy`` solve loop (:259-282) is replaced by one call into the
HIP library (``include/seqik.h``) for all legs, stages and frames.  There is no CPU path: a
missing library or GPU raises.
"""
from abc import ABC, abstractmethod
from pathlib import Path
from typing import Dict, Literal, Optional, Tuple, Union
import logging

import os

import numpy as np

from . import _lib
from .data import DOFS, INITIAL_ANGLES, SEGMENTS
from .kinematic_chain import (Chain, KinematicChainBase, KinematicChainGeneric, KinematicChainSeq, LEG_NAMES, STAGE_DOFS,
                              STAGE_LINKS)
from .utils import save_file

logging.basicConfig(format=" %(asctime)s - %(levelname)s- %(message)s", handlers=[logging.StreamHandler()])


class LegInvKinBase(ABC):
    """Abstract class to calculate inverse kinematics for leg joints.

    Parameters
    ----------
    aligned_pos : Dict[str, np.ndarray]
        Aligned pose, ``"<side><segment>_leg" -> (N_frames, N_key_points, 3)``.
    kinematic_chain_class : KinematicChainBase
        Kinematic chain description of the legs.
    initial_angles : Dict[str, Dict[str, np.ndarray]], optional
        Seeds per leg and stage; defaults to ``data.INITIAL_ANGLES``.
    log_level : {"DEBUG", "INFO", "WARNING", "ERROR"}
    """

    def __init__(self, aligned_pos: Dict[str, np.ndarray], kinematic_chain_class: KinematicChainBase,
                 initial_angles: Optional[Dict[str, np.ndarray]] = None,
                 log_level: Literal["DEBUG", "INFO", "WARNING", "ERROR"] = "INFO") -> None:
        self.aligned_pos = aligned_pos
        self.kinematic_chain_class = kinematic_chain_class
        self.initial_angles = INITIAL_ANGLES if initial_angles is None else initial_angles
        self.logger = logging.getLogger(self.__class__.__name__)
        self.logger.setLevel(getattr(logging, log_level.upper(), None))
        #: HIP device ordinal used by this object
        self.device = -1  # HIP device ordinal; -1 = the calling thread's current device

    # -- per-frame seam (reference :62-77) ---------------------------------------------
    def calculate_ik(self, kinematic_chain: Chain, target_pos: np.ndarray,
                     initial_angles: np.ndarray = None) -> np.ndarray:
        """Joint angles of ``kinematic_chain`` that bring its end effector closest to ``target_pos``.

        One single-frame, single-stage launch of the HIP solver (the batched entry points are
        the fast path; this seam exists for API compatibility)."""
        return kinematic_chain.inverse_kinematics(target_position=target_pos, initial_position=initial_angles,
                                                  device=self.device if kinematic_chain.device < 0 else None)

    def calculate_fk(self, kinematic_chain: Chain, joint_angles: np.ndarray) -> np.ndarray:
        """Positions of every link frame of ``kinematic_chain`` at ``joint_angles`` (n_links, 3)."""
        if len(joint_angles) != len(kinematic_chain.links):
            raise ValueError(f"Your joints vector length is {len(joint_angles)} but you have "
                             f"{len(kinematic_chain.links)} links")
        frames = kinematic_chain.forward_kinematics(joint_angles, full_kinematics=True)
        out = np.zeros((len(kinematic_chain.links), 3))
        for i, frame in enumerate(frames):
            out[i] = frame[:3, 3]
        return out

    def get_scale_factor(self, vector: np.ndarray, length: float) -> float:
        """Ratio between ``length`` and the summed segment lengths of ``vector``."""
        return length / np.sum(np.linalg.norm(np.diff(vector, axis=0), axis=1))

    @abstractmethod
    def calculate_ik_stage(self, end_effector_pos, origin, initial_angles, segment_name, **kwargs) -> np.ndarray:
        ...

    @abstractmethod
    def run_ik_and_fk(self, export_path: Union[Path, str] = None, **kwargs
                      ) -> Tuple[Dict[str, np.ndarray], Dict[str, np.ndarray]]:
        ...

    # -- shared helpers ----------------------------------------------------------------
    def _leg_segments(self):
        """(segment_name, leg_name, array) of the legs this object will process, in dict order."""
        out = []
        for segment_name, segment_array in self.aligned_pos.items():
            if "leg" not in segment_name.lower():
                self.logger.debug("Segment %s is not a leg, continuing...", segment_name)
                continue
            leg_name = segment_name.split("_")[0]
            if leg_name not in self.kinematic_chain_class.body_size:
                self.logger.warning("Leg %s is not in the kinematic chain, continuing...", leg_name)
                continue
            out.append((segment_name, leg_name, segment_array))
        return out

    # -- forward kinematics from joint angles (include/seqik_fk.h) ------------------------
    #: chain kind of the angles this class produces (``_lib.forward_kinematics``)
    _fk_kind = "seq"

    def _fk_leg_params(self, leg_name):
        """SeqikLegParams carrying only what forward kinematics reads: the segment lengths."""
        lp = _lib.SeqikLegParams()
        for i, seg in enumerate(SEGMENTS):
            lp.seg[i] = float(self.kinematic_chain_class.body_size[f"{leg_name}_{seg}"])
        return lp

    def _fk_angles(self, joint_angles, leg_name):
        """(N, 7) array in DOFS order from ``Angle_<leg>_<dof>`` entries."""
        cols = []
        for dof in DOFS:
            key = f"Angle_{leg_name}_{dof}"
            if key not in joint_angles:
                raise ValueError(f"joint angles have no entry {key!r}")
            cols.append(np.asarray(joint_angles[key], dtype=np.float64).reshape(-1))
        if len({c.shape[0] for c in cols}) != 1:
            raise ValueError(f"the joint angles of {leg_name} have different frame counts: "
                             f"{sorted({c.shape[0] for c in cols})}")
        return np.stack(cols, axis=1)

    def _fk_key_points(self, leg_name, segment_array):
        """(N, 5, 3) key points the solver of this class fits: origin, then the four end effectors."""
        return np.asarray(segment_array, dtype=np.float64)[:, :5, :]

    def _fk_batches(self, joint_angles, origin=None, want_pose=False):
        """Per group of legs with the same frame count: (items, angles (1, L, N, 7), origin or pose array)."""
        ja = self.joint_angles_dict if joint_angles is None else joint_angles
        groups = {}
        for segment_name, leg_name, arr in self._leg_segments():
            ang = self._fk_angles(ja, leg_name)
            groups.setdefault(ang.shape[0], []).append((segment_name, leg_name, arr, ang))
        for n, items in groups.items():
            per_leg = []
            for segment_name, leg_name, arr, _ in items:
                if origin is not None and not want_pose:
                    o = np.asarray(origin, dtype=np.float64)
                    if o.shape not in ((3,), (n, 3)):
                        raise ValueError(f"origin must have shape (3,) or ({n}, 3), got {o.shape}")
                    per_leg.append(np.broadcast_to(o, (n, 3)))
                    continue
                n_pos = np.asarray(arr).shape[0]
                if n_pos != n:
                    raise ValueError(f"{segment_name}: the joint angles have {n} frames, aligned_pos has {n_pos}")
                kp = self._fk_key_points(leg_name, arr)
                per_leg.append(kp if want_pose else kp[:, 0])
            yield items, np.stack([a for *_, a in items])[None], np.stack(per_leg)[None]

    def run_fk(self, joint_angles: Optional[Dict[str, np.ndarray]] = None, export_path: Union[Path, str] = None,
               origin: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
        """Forward kinematics of every leg from joint angles alone, on the GPU (``seqik_forward_kinematics``).

        The reference obtains joint positions only inside its IK loop (``calculate_fk`` per frame and stage,
        leg_inverse_kinematics.py:71-77, stored for stage 4 at :279-282); this computes the same ``(N, 9, 3)`` rows for
        angles from any source -- an earlier run's ``leg_joint_angles.pkl``, ``utils.interpolate_joint_angles``, edited
        angles.  ``joint_angles`` defaults to ``self.joint_angles_dict`` (``Angle_<leg>_<dof>`` entries; a missing one
        raises ``ValueError``); the chain kind follows the class.  ``origin`` defaults to key point 0 of ``aligned_pos``
        (whose frame count must match) -- ``template_coxa`` for a ``LegInvKinSeq`` with ``leg_affine``; an explicit
        ``(3,)`` or ``(N, 3)`` array is used for every leg.  After ``run_ik_and_fk`` the result equals its forward
        kinematics dict bit for bit.  ``export_path``: writes ``forward_kinematics.pkl`` there.
        Returns ``{segment_name: (N, 9, 3)}`` in the order of ``aligned_pos``."""
        out = {}
        for items, angles, org in self._fk_batches(joint_angles, origin):
            legs = [self._fk_leg_params(leg_name) for _, leg_name, _, _ in items]
            fk = _lib.forward_kinematics(angles, legs, kind=self._fk_kind, origin=org, device=self.device)["fk"]
            for li, (segment_name, *_) in enumerate(items):
                out[segment_name] = fk[0, li].copy()
        out = {name: out[name] for name, _, _ in self._leg_segments()}
        if export_path is not None:
            save_file(Path(export_path) / "forward_kinematics.pkl", out)
            self.logger.info("Forward kinematics are saved at %s", export_path)
        return out

    def run_link_frames(self, joint_angles: Optional[Dict[str, np.ndarray]] = None, origin: Optional[np.ndarray] = None,
                        export_path: Union[Path, str] = None) -> Dict[str, np.ndarray]:
        """The 4 x 4 frame -- position and orientation -- of every link of every leg from joint angles alone, on the GPU
        (``seqik_link_frames``): ``{segment_name: (N, 9, 4, 4)}`` in the order of ``aligned_pos``, per frame what the
        reference's ``chain.forward_kinematics(q, full_kinematics=True)`` returns for the whole-leg chain of this class
        (link order: ``_lib.link_frames``), with the origin added to the translation column.

        ``joint_angles`` and ``origin`` default as in ``run_fk``; with the default origin the translation columns
        ``[..., :3, 3]`` equal ``run_fk``'s rows bit for bit.  ``export_path``: writes ``link_frames.pkl`` there."""
        out = {}
        for items, angles, org in self._fk_batches(joint_angles, origin):
            legs = [self._fk_leg_params(leg_name) for _, leg_name, _, _ in items]
            frames = _lib.link_frames(angles, legs, kind=self._fk_kind, origin=org, device=self.device)["frames"]
            for li, (segment_name, *_) in enumerate(items):
                out[segment_name] = frames[0, li].copy()
        out = {name: out[name] for name, _, _ in self._leg_segments()}
        if export_path is not None:
            save_file(Path(export_path) / "link_frames.pkl", out)
            self.logger.info("Link frames are saved at %s", export_path)
        return out

    def fit_error(self, joint_angles: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, np.ndarray]:
        """How far the reconstructed CTr, FTi, TiTa and claw lie from the key points they were fitted to:
        ``{segment_name: (N, 4)}`` Euclidean distances of forward-kinematics rows 4, 6, 7, 8 from key points 1..4 of
        ``aligned_pos`` (the targets of stages 1-4, leg_inverse_kinematics.py:279-282; the generic chain's claw target
        is the last key point).  Computed on the GPU with the forward kinematics (``seqik_forward_kinematics``, ``dist``)."""
        out = {}
        for items, angles, pose in self._fk_batches(joint_angles, want_pose=True):
            legs = [self._fk_leg_params(leg_name) for _, leg_name, _, _ in items]
            d = _lib.forward_kinematics(angles, legs, kind=self._fk_kind, pose=pose, want_dist=True,
                                        device=self.device)["dist"]
            for li, (segment_name, *_) in enumerate(items):
                out[segment_name] = d[0, li].copy()
        return {name: out[name] for name, _, _ in self._leg_segments()}

    # -- resampling of the joint angles (include/seqik_resample.h) --------------------------
    def run_resample(self, original_ts, new_ts, joint_angles: Optional[Dict[str, np.ndarray]] = None,
                     missing: str = "error", max_gap: Optional[int] = None, with_fk: bool = False,
                     origin: Optional[np.ndarray] = None, export_path: Union[Path, str] = None):
        """The legs' joint angles resampled from time step ``original_ts`` to ``new_ts`` on the GPU with the reference's
        interpolant (``utils.interpolate_joint_angles``: scipy's PCHIP; ``seqik_resample_pchip``).

        The angles (``joint_angles``, default: the last run's ``self.joint_angles_dict``) go as ``(L, N, 7)`` records in
        one call per frame count, so with ``missing="bridge"`` a leg-frame is bridged as a whole: the NaN frames that
        ``missing_key_points="skip"`` leaves are filled from the solved frames around them (``max_gap``: the longest run
        of missing frames that is filled; None: any).  ``missing="error"`` refuses non-finite angles as scipy does.
        Returns the resampled ``{"Angle_<leg>_<dof>": (n_out,)}`` dictionary (entries of other legs are not touched and
        not returned).

        ``with_fk=True`` also computes the forward kinematics of the resampled angles, from the device buffer the
        resampling wrote (``seqik_forward_kinematics_device``, no host round trip), and returns ``(angles,
        {segment_name: (n_out, 9, 3)})``.  ``origin``: one ``(3,)`` point per call, used for every leg; default: each
        leg's key point 0 as in ``run_fk`` when it is the same in every frame that has one, else ``ValueError`` (a moving
        origin cannot be resampled here).  ``export_path``: writes ``leg_joint_angles_resampled.pkl`` (and
        ``forward_kinematics_resampled.pkl``) there."""
        ja = self.joint_angles_dict if joint_angles is None else joint_angles
        groups = {}
        for segment_name, leg_name, arr in self._leg_segments():
            ang = self._fk_angles(ja, leg_name)
            groups.setdefault(ang.shape[0], []).append((segment_name, leg_name, arr, ang))
        angles_out, fk_out = {}, {}
        for n, items in groups.items():
            y = np.stack([a for *_, a in items])
            if not with_fk:
                res = _lib.resample_pchip(y, original_ts, new_ts, missing=missing, max_gap=max_gap, device=self.device)
                fk = None
            else:
                origins = np.stack([self._resample_origin(origin, segment_name, leg_name, arr)
                                    for segment_name, leg_name, arr, _ in items])
                legs = [self._fk_leg_params(leg_name) for _, leg_name, _, _ in items]
                res, fk = self._resample_with_fk(y, original_ts, new_ts, missing, max_gap, legs, origins)
            for li, (segment_name, leg_name, _, _) in enumerate(items):
                for di, dof in enumerate(DOFS):
                    angles_out[f"Angle_{leg_name}_{dof}"] = res[li, :, di].copy()
                if fk is not None:
                    fk_out[segment_name] = fk[li].copy()
        if export_path is not None:
            save_file(Path(export_path) / "leg_joint_angles_resampled.pkl", angles_out)
            if with_fk:
                save_file(Path(export_path) / "forward_kinematics_resampled.pkl", fk_out)
        if not with_fk:
            return angles_out
        return angles_out, {name: fk_out[name] for name, _, _ in self._leg_segments()}

    # -- joint-angle velocities and accelerations (include/seqik_resample_der.h) ------------
    def run_joint_velocities(self, original_ts, new_ts=None, joint_angles: Optional[Dict[str, np.ndarray]] = None,
                             missing: str = "error", max_gap: Optional[int] = None, acceleration: bool = False,
                             export_path: Union[Path, str] = None):
        """The legs' joint angular velocities on the GPU: the first derivative of the interpolant ``run_resample``
        evaluates (scipy's PCHIP, ``pchip_interpolate(..., der=1)``; ``seqik_resample_der``), in rad per unit of
        ``original_ts``, at the samples ``i * new_ts``.  ``new_ts=None`` means ``original_ts``: the rates at the
        recording's own frames (the knot derivatives).

        ``joint_angles``, ``missing`` and ``max_gap`` are ``run_resample``'s: the angles go as ``(L, N, 7)`` records in
        one call per frame count, so ``missing="bridge"`` bridges a leg-frame as a whole, and a rate is NaN exactly where
        the resampled angle is.  Returns ``{"Angle_<leg>_<dof>": (n_out,)}``; with ``acceleration=True`` the pair
        ``(velocities, accelerations)`` of such dictionaries (second derivative, rad per unit squared).
        ``export_path``: writes ``leg_joint_velocities.pkl`` (and ``leg_joint_accelerations.pkl``) there."""
        ja = self.joint_angles_dict if joint_angles is None else joint_angles
        new_ts = original_ts if new_ts is None else new_ts
        groups = {}
        for segment_name, leg_name, arr in self._leg_segments():
            ang = self._fk_angles(ja, leg_name)
            groups.setdefault(ang.shape[0], []).append((leg_name, ang))
        vel, acc = {}, {}
        for items in groups.values():
            res = _lib.resample_pchip_der(np.stack([a for _, a in items]), original_ts, new_ts,
                                          der=(1, 2) if acceleration else (1,), missing=missing, max_gap=max_gap,
                                          device=self.device)
            for li, (leg_name, _) in enumerate(items):
                for di, dof in enumerate(DOFS):
                    vel[f"Angle_{leg_name}_{dof}"] = res[0][li, :, di].copy()
                    if acceleration:
                        acc[f"Angle_{leg_name}_{dof}"] = res[1][li, :, di].copy()
        if export_path is not None:
            save_file(Path(export_path) / "leg_joint_velocities.pkl", vel)
            if acceleration:
                save_file(Path(export_path) / "leg_joint_accelerations.pkl", acc)
        return (vel, acc) if acceleration else vel

    # -- key-point Jacobians, conditioning and velocities (include/seqik_jacobian.h) --------
    def _jacobian_outputs(self, joint_angles, want_jac, want_sigma):
        """``_lib.leg_jacobians`` per group of legs with the same frame count -> ({segment_name: jac}, {...: sigma})."""
        jac, sigma = {}, {}
        for items, angles, _ in self._fk_batches(joint_angles, origin=np.zeros(3)):
            legs = [self._fk_leg_params(leg_name) for _, leg_name, _, _ in items]
            out = _lib.leg_jacobians(angles, legs, kind=self._fk_kind, want_jac=want_jac, want_sigma=want_sigma,
                                     device=self.device)
            for li, (segment_name, *_) in enumerate(items):
                if want_jac:
                    jac[segment_name] = out["jac"][0, li].copy()
                if want_sigma:
                    sigma[segment_name] = out["sigma"][0, li].copy()
        order = [name for name, _, _ in self._leg_segments()]
        return {n: jac[n] for n in order if n in jac}, {n: sigma[n] for n in order if n in sigma}

    def run_jacobians(self, joint_angles: Optional[Dict[str, np.ndarray]] = None,
                      export_path: Union[Path, str] = None) -> Dict[str, np.ndarray]:
        """How the fitted key points move when the angles move, for every leg, on the GPU (``seqik_leg_jacobians``):
        ``{segment_name: (N, 4, 3, 7)}`` in the order of ``aligned_pos``; ``[t, k, :, d]`` is the derivative of key point
        k + 1 of frame t (forward-kinematics rows 4, 6, 7, 8: coxa, femur and tibia end, claw) with respect to the angle
        of ``DOFS[d]``, length per radian, in the leg's own frame (it does not depend on the origin).  The chain kind
        follows the class; ``joint_angles`` defaults as in ``run_fk``.  Noise propagation from the key points to the angles of
        the sequential fit is not the pseudo-inverse of this matrix: see ``LegInvKinSeq.run_angle_sensitivity`` /
        ``angle_uncertainty``.  ``export_path``: writes ``leg_jacobians.pkl`` there."""
        out, _ = self._jacobian_outputs(joint_angles, True, False)
        if export_path is not None:
            save_file(Path(export_path) / "leg_jacobians.pkl", out)
            self.logger.info("Leg Jacobians are saved at %s", export_path)
        return out

    def conditioning(self, joint_angles: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, np.ndarray]:
        """How well the angles are determined by the key points they were fitted to, per frame, on the GPU
        (``seqik_leg_jacobians``, ``sigma``): the singular values of the Jacobian each least-squares solve works with.

        ``LegInvKinSeq``: ``{segment_name: (N, 4, 2)}``, per stage ``(sigma_max, sigma_min)`` of that stage's block.
        Stage 1 reads key point 1 (coxa end) and solves ThC_yaw, ThC_pitch; stage 2 reads key point 2 (femur end) and
        solves ThC_roll, CTr_pitch; stage 3 reads key point 3 (tibia end) and solves CTr_roll, FTi_pitch; stage 4 reads
        key point 4 (claw) and solves TiTa_pitch (one column: both entries are its norm).  A ``sigma_min`` that is small
        next to ``sigma_max`` -- or to the recording's median -- means that the stage's two angles are not both
        determined by its key point: some combination of them leaves the key point where it is (a kinematic
        singularity, e.g. a stretched joint and the roll about it), and the solved angles there are arbitrary along that
        combination.  ``LegInvKinGeneric``: ``{segment_name: (N, 3)}``, the singular values of the claw's 3 x 7 block,
        descending (seven angles from three coordinates: the problem is rank-deficient by construction; a small third
        value marks postures where the claw loses a direction of motion)."""
        return self._jacobian_outputs(joint_angles, False, True)[1]

    def run_key_point_velocities(self, original_ts, new_ts=None, joint_angles: Optional[Dict[str, np.ndarray]] = None,
                                 missing: str = "error", max_gap: Optional[int] = None,
                                 export_path: Union[Path, str] = None) -> Dict[str, np.ndarray]:
        """The velocities of the four fitted key points of every leg, on the GPU: ``{segment_name: (n_out, 4, 3)}``, the
        Jacobian at the resampled angles times the joint rates, in length per unit of ``original_ts``.

        The angles are resampled and differentiated on the device as in ``run_resample`` / ``run_joint_velocities``
        (``seqik_resample_der_device``: value and first derivative), and the Jacobian kernel runs on those device buffers
        (``seqik_leg_jacobians_device``) with no host round trip.  ``new_ts=None`` means ``original_ts``.  ``missing``
        and ``max_gap``: ``run_resample``'s; a velocity is NaN exactly where the resampled angle or rate is.
        ``export_path``: writes ``key_point_velocities.pkl`` there."""
        import torch
        ja = self.joint_angles_dict if joint_angles is None else joint_angles
        new_ts = original_ts if new_ts is None else new_ts
        flags, _ = _lib._resample_flags(missing, max_gap)
        groups = {}
        for segment_name, leg_name, arr in self._leg_segments():
            ang = self._fk_angles(ja, leg_name)
            groups.setdefault(ang.shape[0], []).append((segment_name, leg_name, ang))
        out = {}
        dev = torch.device("cuda", torch.cuda.current_device() if self.device < 0 else self.device)
        for N, items in groups.items():
            y = np.ascontiguousarray(np.stack([a for *_, a in items]), dtype=np.float64)
            L = y.shape[0]
            if N < 2:
                raise ValueError("The number of knots must be at least 2")
            if not flags and not np.isfinite(y).all():
                raise ValueError("`y` must contain only finite values (missing='bridge' resamples over the finite records)")
            n_out = _lib.resample_count(N, original_ts, new_ts)
            legs = [self._fk_leg_params(leg_name) for _, leg_name, _ in items]
            with torch.cuda.device(dev):
                d_y = torch.from_numpy(y).to(dev)
                d_val = torch.empty((L, n_out, 7), dtype=torch.float64, device=dev)
                d_d1 = torch.empty((L, n_out, 7), dtype=torch.float64, device=dev)
                d_ws = torch.empty((2, L, N), dtype=torch.int32, device=dev) if flags else 0
                d_vel = torch.empty((L, n_out, 4, 3), dtype=torch.float64, device=dev)
                stream = torch.cuda.current_stream().cuda_stream
                _lib.resample_der_device(d_y, L, N, 7, original_ts, new_ts, d_value=d_val, d_d1=d_d1, missing=missing,
                                         max_gap=max_gap, d_workspace=d_ws, stream=stream)
                _lib.leg_jacobians_device(d_val, 1, L, n_out, legs, kind=self._fk_kind, d_qdot=d_d1, d_vel=d_vel,
                                          stream=stream)
                torch.cuda.synchronize(dev)
                vel = d_vel.cpu().numpy()
            for li, (segment_name, *_) in enumerate(items):
                out[segment_name] = vel[li].copy()
        out = {name: out[name] for name, _, _ in self._leg_segments()}
        if export_path is not None:
            save_file(Path(export_path) / "key_point_velocities.pkl", out)
        return out

    def _resample_origin(self, origin, segment_name, leg_name, segment_array):
        if origin is not None:
            o = np.asarray(origin, dtype=np.float64)
            if o.shape != (3,):
                raise ValueError(f"origin must have shape (3,), got {o.shape}")
            return o
        kp0 = self._fk_key_points(leg_name, segment_array)[:, 0]
        rows = kp0[np.isfinite(kp0).all(axis=1)]
        if rows.shape[0] == 0 or not (rows == rows[0]).all():
            raise ValueError(f"{segment_name}: key point 0 is not the same in every frame; pass origin=(3,)")
        return rows[0].copy()

    def _resample_with_fk(self, y, original_ts, new_ts, missing, max_gap, legs, origins):
        """(L, N, 7) host angles -> resampled (L, n_out, 7) and FK (L, n_out, 9, 3), both computed on device buffers."""
        import torch
        flags, _ = _lib._resample_flags(missing, max_gap)
        y = np.ascontiguousarray(y, dtype=np.float64)
        L, N = y.shape[:2]
        if N < 2:
            raise ValueError("The number of knots must be at least 2")
        if not flags and not np.isfinite(y).all():
            raise ValueError("`y` must contain only finite values (missing='bridge' resamples over the finite records)")
        n_out = _lib.resample_count(N, original_ts, new_ts)
        dev = torch.device("cuda", torch.cuda.current_device() if self.device < 0 else self.device)
        with torch.cuda.device(dev):
            d_y = torch.from_numpy(y).to(dev)
            d_out = torch.empty((L, n_out, 7), dtype=torch.float64, device=dev)
            d_ws = torch.empty((2, L, N), dtype=torch.int32, device=dev) if flags else 0
            d_org = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(origins[:, None, :], (L, n_out, 3)))).to(dev)
            d_fk = torch.empty((L, n_out, 9, 3), dtype=torch.float64, device=dev)
            stream = torch.cuda.current_stream().cuda_stream
            _lib.resample_pchip_device(d_y, L, N, 7, original_ts, new_ts, d_out, missing=missing, max_gap=max_gap,
                                       d_workspace=d_ws, stream=stream)
            _lib.forward_kinematics_device(d_out.data_ptr(), 1, L, n_out, legs, d_fk.data_ptr(), kind=self._fk_kind,
                                           d_origin=d_org.data_ptr(), stream=stream)
            torch.cuda.synchronize(dev)
            return d_out.cpu().numpy(), d_fk.cpu().numpy()

    def _export(self, export_path, forward_kinematics_dict):
        if export_path is not None:
            save_file(Path(export_path) / "forward_kinematics.pkl", forward_kinematics_dict)
            save_file(Path(export_path) / "leg_joint_angles.pkl", self.joint_angles_dict)
            self.logger.info("Joint angles and forward kinematics are saved at %s", export_path)


def default_frame_parallel():
    """Default of ``frame_parallel`` in ``run_ik_and_fk``, ``run_ik_and_fk_many`` and ``pipeline.run_body_ik``: ``"auto"``
    (verified frame chunks for recordings of 48 frames and more) unless the environment variable SEQIK_FRAME_PARALLEL says
    ``0`` / ``false`` / ``off`` / ``serial`` (the reference's frame-by-frame walk for the whole process).

    Since round 6 (round-5 review, item 8).  One wavefront per (leg, stage) cannot walk a recording faster than it issues
    instructions: the serial walk of the shipped 6000-frame recording takes 112 ms (1.1e5 leg-frames/s, a tenth of the 1e6/s a
    drop-in is expected to reach), frame chunks 2.1 ms (5.8e6/s).  Both lie equally far from the reference's own shipped
    output -- 5.2e-5 rad at most, one value above 5e-5, the same one -- and 1.1e-5 rad from each other
    (tests/test_frame_chunks.py::test_default_of_frame_parallel_is_decided_by_evidence runs this in the GPU tier)."""
    v = os.environ.get("SEQIK_FRAME_PARALLEL", "").strip().lower()
    return False if v in ("0", "false", "no", "off", "serial") else "auto"


def chunk_report(out, leg_names, n_frames):
    """Per recording (sequence) and leg, where a chunked ``_lib.solve_seq`` result was hard: list over sequences of
    ``{leg: {...}}`` built from ``chunk_stats`` / ``chunk_flags``; empty dicts when the call was walked serially."""
    flags, st = out.get("chunk_flags"), out["chunk_stats"]
    if flags is None or st["chunks"] == 0:
        return [{} for _ in range(out["angles"].shape[0])]
    c = st["frames_per_chunk"]
    reports = []
    for s in range(flags.shape[0]):
        rep = {}
        for li, leg in enumerate(leg_names):
            f = flags[s, li]
            redone = (f & (_lib.CHUNK_FLAG_REPAIRED | _lib.CHUNK_FLAG_SWEPT)) != 0
            spans = [min(c, n_frames - k * c) for k in np.flatnonzero(redone)]
            rep[leg] = {"frames_per_chunk": c, "run_in_frames": st["run_in_frames"],
                        "failed_first_check": [int(k) * c for k in np.flatnonzero(f & _lib.CHUNK_FLAG_FAILED_FIRST)],
                        "frames_repaired": int(sum(spans)),
                        "walked_serially": bool((f & _lib.CHUNK_FLAG_SERIAL).any())}
        reports.append(rep)
    return reports


class LegInvKinSeq(LegInvKinBase):
    """Sequential inverse kinematics: four stages per frame, each matching one more joint.

    >>> seq_ik = LegInvKinSeq(aligned_pos, KinematicChainSeq(BOUNDS, ["RF", "LF"]), INITIAL_ANGLES)
    >>> leg_joint_angles, forward_kinematics = seq_ik.run_ik_and_fk(export_path=DATA_PATH)
    """

    def __init__(self, aligned_pos: Dict[str, np.ndarray], kinematic_chain_class: KinematicChainSeq,
                 initial_angles: Optional[Dict[str, np.ndarray]] = None,
                 log_level: Literal["DEBUG", "INFO", "WARNING", "ERROR"] = "INFO",
                 leg_affine: Optional[Dict[str, tuple]] = None) -> None:
        super().__init__(aligned_pos, kinematic_chain_class, initial_angles, log_level)
        self.joint_angles_dict = {}
        #: optional ``{leg: (fixed_coxa, scale, template_coxa)}`` (``AlignPose.leg_affines()``): when
        #: given, ``aligned_pos`` holds RAW key points and the alignment is fused into the kernels
        self.leg_affine = leg_affine
        #: scipy termination status / nfev of the last run when ``diagnostics=True`` was passed
        self.solver_status = {}
        self.solver_nfev = {}
        #: chunk statistics of the last launch (``_lib.CHUNK_STATS_FIELDS``; all zero = serial walk)
        self.frame_chunk_stats = {}
        #: per leg, where a chunked run was hard (see ``run_ik_and_fk``); empty after a serial walk
        self.frame_chunk_report = {}
        #: per leg, ``cost`` (N, 2) and ``info`` (N,) of the last ``run_refine``
        self.refine_report = {}
        #: per leg, what the last ``run_smooth`` reports of its trajectory
        self.smooth_report = {}

    def _fk_key_points(self, leg_name, segment_array):
        """Key points in the frame the solver works in: with ``leg_affine`` ``aligned_pos`` holds RAW key points and the
        fused alignment (``AlignPose.align_leg``) is applied here with the kernels' operations: row 0 = template_coxa,
        rows 1..4 = (raw - fixed_coxa) * scale + template_coxa."""
        kp = super()._fk_key_points(leg_name, segment_array)
        if self.leg_affine is None:
            return kp
        fixed, scale, template = (np.asarray(v, dtype=np.float64) for v in self.leg_affine[leg_name])
        out = np.empty_like(kp)
        out[:, 0] = template
        out[:, 1:] = (kp[:, 1:] - fixed) * scale + template
        return out

    def _leg_params(self, leg_name, initial_angles=None):
        kc = self.kinematic_chain_class
        return _lib.make_leg_params(leg_name, kc.bounds_dof, kc.body_size,
                                    self.initial_angles if initial_angles is None else initial_angles)

    # -- angle error bars (include/seqik_sensitivity.h) ---------------------------------------
    def _sensitivity_outputs(self, joint_angles, key_point_sigma, want_sens, want_flags, bound_tol):
        """``_lib.fit_sensitivity`` per group of legs with the same frame count -> {segment_name: (leg_name, dict)}."""
        out = {}
        for items, angles, pose in self._fk_batches(joint_angles, want_pose=True):
            legs = [self._leg_params(leg_name) for _, leg_name, _, _ in items]
            n = angles.shape[2]
            sigma = None
            if key_point_sigma is not None:
                sigma = np.empty((1, len(items), n, 4))
                for li, (_, leg_name, _, _) in enumerate(items):
                    s = key_point_sigma[leg_name] if isinstance(key_point_sigma, dict) else key_point_sigma
                    s = np.asarray(s, dtype=np.float64)
                    if s.shape not in ((), (4,), (n, 4)):
                        raise ValueError(f"key_point_sigma must be a scalar, (4,) or ({n}, 4), got {s.shape}")
                    sigma[0, li] = s
            res = _lib.fit_sensitivity(angles, pose, legs, kp_sigma=sigma, want_sens=want_sens, want_flags=want_flags,
                                       bound_tol=bound_tol, device=self.device)
            for li, (segment_name, leg_name, _, _) in enumerate(items):
                out[segment_name] = (leg_name, {k: v[0, li].copy() for k, v in res.items() if v is not None})
        return {name: out[name] for name, _, _ in self._leg_segments()}

    def run_angle_sensitivity(self, joint_angles: Optional[Dict[str, np.ndarray]] = None,
                              bound_tol: float = _lib.SENS_BOUND_TOL) -> Dict[str, Dict[str, np.ndarray]]:
        """How the fitted angles move when the key points they were fitted to move, for every leg, on the GPU
        (``seqik_fit_sensitivity``): ``{segment_name: dict(sens (N, 7, 4, 3), flags (N,))}`` in the order of
        ``aligned_pos``.  ``sens[t, d, k, c]`` is the derivative of the angle of ``DOFS[d]`` of frame t with respect to
        component c of aligned key point k + 1, radians per length -- the response of the four sequential solves with
        their exact Hessians, 0 for a joint that sits on its limit (within ``bound_tol`` rad) and is pushed against it.
        ``flags``: ``_lib.fit_sensitivity``.  The key points are the class's own aligned ones (with ``leg_affine``: after
        the fused alignment; for the RAW key points multiply by the alignment's scale); ``joint_angles`` defaults to the
        stored angles.  The full covariance of a frame's angles is ``S @ diag(sigma^2) @ S.T`` with ``S = sens[t].reshape(7,
        12)``."""
        return {name: res for name, (_, res) in
                self._sensitivity_outputs(joint_angles, None, True, True, bound_tol).items()}

    def angle_uncertainty(self, key_point_sigma, joint_angles: Optional[Dict[str, np.ndarray]] = None,
                          bound_tol: float = _lib.SENS_BOUND_TOL, fit: str = "sequential",
                          key_point_weight=None, smooth=None) -> Dict[str, np.ndarray]:
        """The standard deviation that key-point noise gives every fitted angle, on the GPU (``seqik_fit_sensitivity``,
        ``std``): ``{"Angle_<leg>_<dof>": (N,)}``, radians.  ``key_point_sigma``: the isotropic standard deviation of key
        points 1..4 (CTr, FTi, TiTa, claw) in the units of the aligned key points -- a scalar, a ``(4,)`` vector, an ``(N,
        4)`` array (e.g. anipose's ``<kp>_error`` columns), or a ``{leg: one of those}`` dictionary.  A held joint has
        0; a frame with a non-finite angle, key point or sigma has NaN.

        ``fit``: which fit ``joint_angles`` are the answer of.  ``"sequential"`` (default): ``run_ik_and_fk``'s four
        stage solves.  ``"refine"``: the whole-leg fit of ``run_refine`` (``seqik_refine_sensitivity``); pass
        ``run_refine``'s angles as ``joint_angles`` and the ``key_point_weight`` it was run with -- the values are that
        fit's error bars only at angles that minimise it (``run_refine_sensitivity`` returns ``grad``, which tells).
        ``"smooth"``: the trajectory fit of ``run_smooth`` (``seqik_smooth_sensitivity``); pass ``run_smooth``'s angles
        and the ``smooth`` (required: the penalty is part of the quantity) and ``key_point_weight`` it was run with.  The
        penalty couples the frames, so an angle's standard deviation collects the noise of ALL frames' key points, taken
        as independent between frames; it is as good as the stationarity ``run_smooth`` reached
        (``run_smooth_sensitivity`` returns ``grad``)."""
        if fit not in ("sequential", "refine", "smooth") or (fit == "smooth" and smooth is None):
            raise ValueError(f"fit must be 'sequential', 'refine', or 'smooth' together with smooth= (the penalty the "
                             f"trajectory was fitted with); got fit={fit!r}, smooth={smooth!r}")
        if smooth is not None and fit != "smooth":
            raise ValueError(f"smooth belongs to fit='smooth': fit={fit!r} has no penalty")
        if fit == "smooth":
            res_by_segment = self._smooth_sensitivity_outputs(joint_angles, smooth, key_point_weight, key_point_sigma, 0,
                                                              bound_tol, False, False, False)
            return {f"Angle_{leg_name}_{dof}": res["std"][:, di].copy() for leg_name, res in res_by_segment.values()
                    for di, dof in enumerate(DOFS)}
        if fit == "refine":
            res_by_segment = self._refine_sensitivity_outputs(joint_angles, key_point_weight, key_point_sigma, bound_tol,
                                                              False, False, False)
            return {f"Angle_{leg_name}_{dof}": res["std"][:, di].copy() for leg_name, res in res_by_segment.values()
                    for di, dof in enumerate(DOFS)}
        if key_point_weight is not None:
            raise ValueError("key_point_weight belongs to fit='refine' and fit='smooth': the sequential fit has no weights")
        out = {}
        for _, (leg_name, res) in self._sensitivity_outputs(joint_angles, key_point_sigma, False, False, bound_tol).items():
            for di, dof in enumerate(DOFS):
                out[f"Angle_{leg_name}_{dof}"] = res["std"][:, di].copy()
        return out

    @staticmethod
    def _key_point_sigmas(items, n, key_point_sigma):
        """``key_point_sigma`` for one batch of legs -> (1, L, n, 4), or None."""
        if key_point_sigma is None:
            return None
        sigma = np.empty((1, len(items), n, 4))
        for li, (_, leg_name, _, _) in enumerate(items):
            s = key_point_sigma[leg_name] if isinstance(key_point_sigma, dict) else key_point_sigma
            s = np.asarray(s, dtype=np.float64)
            if s.shape not in ((), (4,), (n, 4)):
                raise ValueError(f"key_point_sigma must be a scalar, (4,) or ({n}, 4), got {s.shape}")
            sigma[0, li] = s
        return sigma

    # -- error bars of the whole-leg refinement (include/seqik_refine_sensitivity.h) ------------
    def _refine_sensitivity_outputs(self, joint_angles, key_point_weight, key_point_sigma, bound_tol, want_sens, want_grad,
                                    want_flags):
        """``_lib.refine_sensitivity`` per group of legs with the same frame count -> {segment_name: (leg_name, dict)}."""
        out = {}
        for items, angles, pose in self._fk_batches(joint_angles, want_pose=True):
            legs = [self._leg_params(leg_name) for _, leg_name, _, _ in items]
            n = angles.shape[2]
            res = _lib.refine_sensitivity(angles, pose, legs, kp_weight=self._key_point_weights(items, n, key_point_weight),
                                          kp_sigma=self._key_point_sigmas(items, n, key_point_sigma), bound_tol=bound_tol,
                                          want_sens=want_sens, want_grad=want_grad, want_flags=want_flags,
                                          device=self.device)
            for li, (segment_name, leg_name, _, _) in enumerate(items):
                out[segment_name] = (leg_name, {k: v[0, li].copy() for k, v in res.items() if v is not None})
        return {name: out[name] for name, _, _ in self._leg_segments()}

    def run_refine_sensitivity(self, joint_angles: Optional[Dict[str, np.ndarray]] = None, key_point_weight=None,
                               bound_tol: float = _lib.SENS_BOUND_TOL) -> Dict[str, Dict[str, np.ndarray]]:
        """How the angles of the whole-leg fit (``run_refine``) move when the key points move, for every leg, on the GPU
        (``seqik_refine_sensitivity``): ``{segment_name: dict(sens (N, 7, 4, 3), flags (N,), grad (N,))}`` in the order
        of ``aligned_pos``.  ``sens[t, d, k, c]`` is the derivative of the angle of ``DOFS[d]`` of frame t with respect
        to component c of aligned key point k + 1, radians per length: the inverse of the fit's exact Hessian on the
        free joints applied to the weighted Jacobian.  Unlike ``run_angle_sensitivity`` it is a full matrix -- in the
        whole-leg fit every angle answers to every key point.

        THE VALUES ARE THE WHOLE-LEG FIT'S RESPONSE ONLY AT ANGLES THAT MINIMISE THAT FIT, that is ``run_refine``'s
        output: pass it as ``joint_angles`` (default: the stored angles, as everywhere) with the ``key_point_weight`` it
        was run with.  ``grad`` tells whether they do: the left side of ``run_refine``'s gradient test at these angles
        (``<= gtol``, 1e-10 by default, where the refinement stopped on it).  ``flags``: bits 0..6 joint held on a limit
        (its row is 0), bit 8 the angles are not a strict minimum (the free rows are NaN), bit 16 bad input
        (``_lib.refine_sensitivity``).  The key points are the class's own aligned ones (with ``leg_affine``: after the
        fused alignment; for the RAW key points multiply by the alignment's scale).  The full covariance of a frame's
        angles is ``S @ diag(sigma^2) @ S.T`` with ``S = sens[t].reshape(7, 12)``."""
        return {name: res for name, (_, res) in
                self._refine_sensitivity_outputs(joint_angles, key_point_weight, None, bound_tol, True, True, True).items()}

    def _refine_with_error_bars(self, angles, pose, legs, weight, sigma, bound_tol, opts):
        """``refine_legs_device`` then ``refine_sensitivity_device`` on the same stream: the refined angles do not leave
        the device in between -> the dict of ``_lib.refine_legs`` plus ``std`` (1, L, N, 7) and ``sens_flags`` (1, L, N)."""
        import torch
        S, L, N = angles.shape[:3]
        dev = torch.device("cuda", torch.cuda.current_device() if self.device < 0 else self.device)
        with torch.cuda.device(dev):
            up = lambda a: 0 if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
            d_ang, d_pose, d_w, d_sig = up(angles), up(pose), up(weight), up(sigma)
            d_out = torch.empty((S, L, N, 7), dtype=torch.float64, device=dev)
            d_cost = torch.empty((S, L, N, 2), dtype=torch.float64, device=dev)
            d_info = torch.empty((S, L, N), dtype=torch.int32, device=dev)
            d_std = torch.empty((S, L, N, 7), dtype=torch.float64, device=dev)
            d_flags = torch.empty((S, L, N), dtype=torch.int32, device=dev)
            stream = torch.cuda.current_stream().cuda_stream
            _lib.refine_legs_device(d_ang, d_pose, S, L, N, legs, d_out, d_kp_weight=d_w, d_cost=d_cost, d_info=d_info,
                                    stream=stream, **opts)
            _lib.refine_sensitivity_device(d_out, d_pose, S, L, N, legs, d_kp_weight=d_w, d_kp_sigma=d_sig, d_std=d_std,
                                           d_flags=d_flags, bound_tol=bound_tol, stream=stream)
            torch.cuda.synchronize(dev)
            return dict(angles=d_out.cpu().numpy(), cost=d_cost.cpu().numpy(), info=d_info.cpu().numpy(),
                        std=d_std.cpu().numpy(), sens_flags=d_flags.cpu().numpy())

    @staticmethod
    def _key_point_weights(items, n, key_point_weight):
        """``key_point_weight`` of ``run_refine`` / ``run_smooth`` for one batch of legs -> (1, L, n, 4), or None."""
        if key_point_weight is None:
            return None
        weight = np.empty((1, len(items), n, 4))
        for li, (_, leg_name, _, _) in enumerate(items):
            w = key_point_weight[leg_name] if isinstance(key_point_weight, dict) else key_point_weight
            w = np.asarray(w, dtype=np.float64)
            if w.shape not in ((), (4,), (n, 4)):
                raise ValueError(f"key_point_weight must be a scalar, (4,) or ({n}, 4), got {w.shape}")
            weight[0, li] = w
        return weight

    # -- whole-leg refinement (include/seqik_refine.h) ------------------------------------------
    def run_refine(self, joint_angles: Optional[Dict[str, np.ndarray]] = None, key_point_weight=None,
                   export_path: Union[Path, str] = None, key_point_sigma=None,
                   bound_tol: float = _lib.SENS_BOUND_TOL, **opts
                   ) -> Tuple[Dict[str, np.ndarray], Dict[str, np.ndarray]]:
        """The sequential fit's angles refined against all four key points at once, on the GPU (``seqik_refine_legs``).

        The sequential fit is greedy -- no stage looks back, so the error accumulates towards the claw.  This starts
        from ``joint_angles`` (default: the stored angles of the last ``run_ik_and_fk``) and, for every frame of every
        leg, minimises the summed squared distance of the reconstructed CTr, FTi, TiTa and claw from key points 1..4
        over all seven angles inside the joint limits.  FRAMES ARE REFINED INDEPENDENTLY, each from its own start: no
        frame is a warm start for the next, so where a leg has two configurations that fit, an angle may move by more
        than a radian from its start and neighbouring frames may differ by as much.

        ``key_point_weight``: the weight of key points 1..4 -- a scalar, ``(4,)``, ``(N, 4)`` or a ``{leg: one of those}``
        dictionary (default 1); a key point with weight exactly 0 is not read and may be NaN.  ``opts``: ``max_iter``,
        ``gtol``, ``ftol`` of ``_lib.refine_legs``.  The key points are the class's own aligned ones (with ``leg_affine``:
        after the fused alignment).  Returns ``(joint_angles_dict, forward_kinematics_dict)`` shaped as ``run_ik_and_fk``
        returns them, the forward kinematics computed from the refined angles (``seqik_forward_kinematics``);
        ``self.joint_angles_dict`` is NOT overwritten.  ``self.refine_report[leg]`` holds ``cost`` ``(N, 2)`` -- the sum
        of squares at the clamped start and at the result -- and ``info`` ``(N,)`` (``_lib.refine_legs``).
        ``export_path``: writes ``leg_joint_angles_refined.pkl`` and ``forward_kinematics_refined.pkl`` there.

        ``key_point_sigma`` (as ``angle_uncertainty``'s; default None: nothing changes): the error bars of the refined
        angles in the same visit to the device -- the sensitivity kernel (``seqik_refine_sensitivity_device``) reads the
        refined angles where the refinement left them.  ``self.refine_report[leg]`` then also holds ``std`` ``(N, 7)``,
        what ``angle_uncertainty(key_point_sigma, refined, fit="refine", key_point_weight=...)`` returns, and
        ``sens_flags`` ``(N,)`` (``_lib.refine_sensitivity``'s flags; ``bound_tol`` is its held-joint tolerance)."""
        unknown = set(opts) - {"max_iter", "gtol", "ftol"}
        if unknown:
            raise ValueError(f"unknown refinement options: {sorted(unknown)}")
        angles_out, fk_out, report = {}, {}, {}
        for items, angles, pose in self._fk_batches(joint_angles, want_pose=True):
            legs = [self._leg_params(leg_name) for _, leg_name, _, _ in items]
            weight = self._key_point_weights(items, angles.shape[2], key_point_weight)
            if key_point_sigma is None:
                res = _lib.refine_legs(angles, pose, legs, kp_weight=weight, device=self.device, **opts)
            else:
                sigma = self._key_point_sigmas(items, angles.shape[2], key_point_sigma)
                res = self._refine_with_error_bars(angles, pose, legs, weight, sigma, bound_tol, opts)
            fk = _lib.forward_kinematics(res["angles"], legs, kind=self._fk_kind, origin=pose[..., 0, :],
                                         device=self.device)["fk"]
            for li, (segment_name, leg_name, _, _) in enumerate(items):
                for di, dof in enumerate(DOFS):
                    angles_out[f"Angle_{leg_name}_{dof}"] = res["angles"][0, li, :, di].copy()
                fk_out[segment_name] = fk[0, li].copy()
                report[leg_name] = dict(cost=res["cost"][0, li].copy(), info=res["info"][0, li].copy())
                if key_point_sigma is not None:
                    report[leg_name].update(std=res["std"][0, li].copy(), sens_flags=res["sens_flags"][0, li].copy())
        order = [(name, leg_name) for name, leg_name, _ in self._leg_segments()]
        angles_out = {f"Angle_{leg_name}_{dof}": angles_out[f"Angle_{leg_name}_{dof}"] for _, leg_name in order
                      for dof in DOFS}
        fk_out = {name: fk_out[name] for name, _ in order}
        self.refine_report = {leg_name: report[leg_name] for _, leg_name in order}
        if export_path is not None:
            save_file(Path(export_path) / "leg_joint_angles_refined.pkl", angles_out)
            save_file(Path(export_path) / "forward_kinematics_refined.pkl", fk_out)
            self.logger.info("Refined joint angles and forward kinematics are saved at %s", export_path)
        return angles_out, fk_out

    # -- trajectory refinement (include/seqik_smooth.h) ------------------------------------------
    def run_smooth(self, joint_angles: Optional[Dict[str, np.ndarray]] = None, smooth=_lib.SMOOTH_DEFAULT,
                   key_point_weight=None, export_path: Union[Path, str] = None, key_point_sigma=None,
                   bound_tol: float = _lib.SENS_BOUND_TOL, **opts) -> Dict[str, np.ndarray]:
        """The whole-leg fit of ``run_refine`` over ALL frames of a leg at once, with a penalty on the change of every
        angle from frame to frame, on the GPU (``seqik_smooth_legs``).

        ``run_refine`` fits every frame on its own, and where a leg has two configurations that fit, neighbouring frames
        land in different ones: the per-frame fit improves and the trajectory gets worse.  This starts from
        ``joint_angles`` (default: the stored angles of the last ``run_ik_and_fk``) and minimises, per leg, the summed
        squared key-point distances of all frames plus ``smooth[j] * leg_length^2`` times the squared change of angle j
        between neighbouring frames, inside the joint limits, by one bounded Levenberg-Marquardt for the whole
        trajectory.  ``smooth``: a scalar or ``(7,)`` in ``DOFS`` order, dimensionless (0.1 removes the 2.6 rad jumps of
        the shipped recording's RF leg; 0.01 leaves most of them).  A frame with a non-finite angle or key point comes
        back as NaN and cuts the coupling between its neighbours.  It is a LOCAL method: it ends in the minimum its start
        leads to.

        ``key_point_weight``: as ``run_refine``.  ``opts``: ``max_iter`` (accepted steps, default 300), ``gtol``,
        ``ftol`` of ``_lib.smooth_legs``.  Returns the joint-angle dictionary shaped as ``run_ik_and_fk`` returns it;
        ``self.joint_angles_dict`` is NOT overwritten.  ``self.smooth_report[leg]`` holds ``cost`` ``(2,)`` -- the
        objective at the clamped start and at the result --, ``reason`` (``_lib.REFINE_STOP_*``), ``steps``,
        ``rejected``, ``frame_info`` ``(N,)`` and ``largest_change`` ``(2,)``: the largest frame-to-frame change of any
        angle before and after, radians.  ``export_path``: writes ``leg_joint_angles_smooth.pkl`` there.

        The trajectory usually stops on the cost decrease (``reason`` 1), not on the gradient test: the angles are then
        stationary only as far as ``run_smooth_sensitivity``'s ``grad`` says (both legs of the shipped recording stop with
        reason 1, at a largest ``grad`` of 3.6e-8 and 5.4e-8 where ``gtol`` is 1e-10).

        ``key_point_sigma`` (as ``angle_uncertainty``'s; default None: nothing changes): the error bars of the smoothed
        angles in the same visit to the device -- ``seqik_smooth_sensitivity_device`` is enqueued behind
        ``seqik_smooth_legs_device`` on one stream and reads the angles where the fit left them.
        ``self.smooth_report[leg]`` then also holds ``std`` ``(N, 7)``, what ``angle_uncertainty(key_point_sigma,
        smoothed, fit="smooth", smooth=..., key_point_weight=...)`` returns, and ``sens_flags`` ``(N,)``
        (``_lib.smooth_sensitivity``'s flags; ``bound_tol`` is its held-joint tolerance).  THE ERROR BARS ARE AS GOOD AS
        THE STATIONARITY THE FIT REACHED."""
        unknown = set(opts) - {"max_iter", "gtol", "ftol"}
        if unknown:
            raise ValueError(f"unknown smoothing options: {sorted(unknown)}")
        angles_out, report = {}, {}
        for items, angles, pose in self._fk_batches(joint_angles, want_pose=True):
            legs = [self._leg_params(leg_name) for _, leg_name, _, _ in items]
            weight = self._key_point_weights(items, angles.shape[2], key_point_weight)
            if key_point_sigma is None:
                res = _lib.smooth_legs(angles, pose, legs, smooth=smooth, kp_weight=weight, device=self.device, **opts)
            else:
                sigma = self._key_point_sigmas(items, angles.shape[2], key_point_sigma)
                res = self._smooth_with_error_bars(angles, pose, legs, smooth, weight, sigma, bound_tol, opts)
            for li, (_, leg_name, _, _) in enumerate(items):
                for di, dof in enumerate(DOFS):
                    angles_out[f"Angle_{leg_name}_{dof}"] = res["angles"][0, li, :, di].copy()
                change = [np.abs(np.diff(a[0, li], axis=0)) for a in (angles, res["angles"])]
                change = [float(c[np.isfinite(c)].max()) if np.isfinite(c).any() else 0.0 for c in change]
                reason, steps, rejected = (int(v) for v in res["info"][0, li])
                report[leg_name] = dict(cost=res["cost"][0, li].copy(), reason=reason, steps=steps, rejected=rejected,
                                        frame_info=res["frame_info"][0, li].copy(), largest_change=np.array(change))
                if key_point_sigma is not None:
                    report[leg_name].update(std=res["std"][0, li].copy(), sens_flags=res["sens_flags"][0, li].copy())
        order = [leg_name for _, leg_name, _ in self._leg_segments()]
        angles_out = {f"Angle_{leg_name}_{dof}": angles_out[f"Angle_{leg_name}_{dof}"] for leg_name in order for dof in DOFS}
        self.smooth_report = {leg_name: report[leg_name] for leg_name in order}
        if export_path is not None:
            save_file(Path(export_path) / "leg_joint_angles_smooth.pkl", angles_out)
            self.logger.info("Smoothed joint angles are saved at %s", export_path)
        return angles_out

    # -- error bars of the smoothed trajectory (include/seqik_smooth_sensitivity.h) ---------------
    def _smooth_with_error_bars(self, angles, pose, legs, smooth, weight, sigma, bound_tol, opts):
        """``smooth_legs_device`` then ``smooth_sensitivity_device`` on the same stream: the smoothed angles do not leave
        the device in between -> the dict of ``_lib.smooth_legs`` plus ``std`` (1, L, N, 7) and ``sens_flags`` (1, L, N)."""
        import torch
        S, L, N = angles.shape[:3]
        dev = torch.device("cuda", torch.cuda.current_device() if self.device < 0 else self.device)
        with torch.cuda.device(dev):
            up = lambda a: 0 if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
            d_ang, d_pose, d_w, d_sig = up(angles), up(pose), up(weight), up(sigma)
            d_out = torch.empty((S, L, N, 7), dtype=torch.float64, device=dev)
            d_finfo = torch.empty((S, L, N), dtype=torch.int32, device=dev)
            d_cost = torch.empty((S, L, 2), dtype=torch.float64, device=dev)
            d_info = torch.empty((S, L, 3), dtype=torch.int32, device=dev)
            d_std = torch.empty((S, L, N, 7), dtype=torch.float64, device=dev)
            d_flags = torch.empty((S, L, N), dtype=torch.int32, device=dev)
            ws_bytes = max(_lib.smooth_workspace_bytes(S, L, N), _lib.smooth_sensitivity_workspace_bytes(S, L, N, 0))
            d_ws = torch.empty((max(ws_bytes, 8),), dtype=torch.uint8, device=dev)   # one workspace, used in turn
            stream = torch.cuda.current_stream().cuda_stream
            _lib.smooth_legs_device(d_ang, d_pose, S, L, N, legs, d_out, d_ws, ws_bytes, d_kp_weight=d_w,
                                    d_frame_info=d_finfo, d_cost=d_cost, d_info=d_info, smooth=smooth, stream=stream, **opts)
            _lib.smooth_sensitivity_device(d_out, d_pose, S, L, N, legs, d_ws, ws_bytes, d_kp_weight=d_w, d_kp_sigma=d_sig,
                                           d_std=d_std, d_flags=d_flags, smooth=smooth, bound_tol=bound_tol, stream=stream)
            torch.cuda.synchronize(dev)
            return dict(angles=d_out.cpu().numpy(), frame_info=d_finfo.cpu().numpy(), cost=d_cost.cpu().numpy(),
                        info=d_info.cpu().numpy(), std=d_std.cpu().numpy(), sens_flags=d_flags.cpu().numpy())

    def _smooth_sensitivity_outputs(self, joint_angles, smooth, key_point_weight, key_point_sigma, half_width, bound_tol,
                                    want_sens, want_grad, want_flags):
        """``_lib.smooth_sensitivity`` per group of legs with the same frame count -> {segment_name: (leg_name, dict)}."""
        out = {}
        for items, angles, pose in self._fk_batches(joint_angles, want_pose=True):
            legs = [self._leg_params(leg_name) for _, leg_name, _, _ in items]
            n = angles.shape[2]
            res = _lib.smooth_sensitivity(angles, pose, legs, smooth=smooth,
                                          kp_weight=self._key_point_weights(items, n, key_point_weight),
                                          kp_sigma=self._key_point_sigmas(items, n, key_point_sigma), half_width=half_width,
                                          bound_tol=bound_tol, want_sens=want_sens, want_grad=want_grad,
                                          want_flags=want_flags, device=self.device)
            for li, (segment_name, leg_name, _, _) in enumerate(items):
                out[segment_name] = (leg_name, {k: v[0, li].copy() for k, v in res.items() if v is not None})
        return {name: out[name] for name, _, _ in self._leg_segments()}

    def run_smooth_sensitivity(self, joint_angles: Optional[Dict[str, np.ndarray]] = None, smooth=_lib.SMOOTH_DEFAULT,
                               key_point_weight=None, half_width: int = 0,
                               bound_tol: float = _lib.SENS_BOUND_TOL) -> Dict[str, Dict[str, np.ndarray]]:
        """How the angles of the trajectory fit (``run_smooth``) move when the key points move, for every leg, on the GPU
        (``seqik_smooth_sensitivity``): ``{segment_name: dict(sens (N, 2 W + 1, 7, 4, 3), flags (N,), grad (N,))}`` in the
        order of ``aligned_pos``, W = ``half_width`` (0..32).  ``sens[t, d, j, k, c]`` is the derivative of the angle of
        ``DOFS[j]`` of frame t with respect to component c of aligned key point k + 1 of frame ``t + d - W``: the penalty
        couples the frames, so an angle answers to its neighbours' key points too (the blocks fall off with ``|d - W|``;
        the centre block ``d = W`` is the frame's own).  A block whose source frame lies outside the recording or beyond a
        NaN frame is 0.

        THE VALUES ARE THE TRAJECTORY FIT'S RESPONSE ONLY AT ANGLES THAT MINIMISE THAT FIT, that is ``run_smooth``'s
        output: pass it as ``joint_angles`` with the ``smooth`` and ``key_point_weight`` it was run with.  ``grad`` (per
        frame; its maximum is the left side of ``run_smooth``'s gradient test) tells how far they do -- ``run_smooth``
        usually stops on the cost decrease, not on the gradient, and the values are as good as that stationarity.
        ``flags``: bits 0..6 joint held on a limit (its rows are 0), bit 8 the run of frames is not a strict minimum (the
        free rows are NaN), bit 16 bad input (``_lib.smooth_sensitivity``)."""
        return {name: res for name, (_, res) in
                self._smooth_sensitivity_outputs(joint_angles, smooth, key_point_weight, None, half_width, bound_tol, True,
                                                 True, True).items()}

    def _prior_angles(self, leg_name, n_frames, first_stage):
        """(N, 7) array with the columns of stages < first_stage taken from ``joint_angles_dict``
        (raises KeyError like the reference's chain factory when they are missing)."""
        angles = np.zeros((n_frames, 7))
        for stage in range(1, first_stage):
            for dof in STAGE_DOFS[stage]:
                col = np.asarray(self.joint_angles_dict[f"Angle_{leg_name}_{dof}"], dtype=np.float64)
                angles[:, DOFS.index(dof)] = col[:n_frames]
        return angles

    def calculate_ik_stage(self, end_effector_pos: np.ndarray, origin: np.ndarray, initial_angles: np.ndarray,
                           segment_name: str, **kwargs) -> np.ndarray:
        """Inverse kinematics of one stage over all frames of one leg.

        ``segment_name`` is the leg (RF, LF, ...), ``stage`` (kwarg) in 1..4.  Joint angles are
        stored in ``self.joint_angles_dict``; returns the joint positions ``(N, n_links, 3)``,
        meaningful for stage 4 only (as in the reference, :279-282)."""
        stage = kwargs.get("stage", 1)
        if segment_name not in LEG_NAMES:
            raise ValueError(f"Segment name ({segment_name}) is not valid.")
        if not 1 <= stage <= 4:
            raise ValueError(f"Stage ({stage}) should be between 1 and 4.")
        end_effector_pos = np.asarray(end_effector_pos, dtype=np.float64)
        frames_no = end_effector_pos.shape[0]
        origin = np.asarray(origin, dtype=np.float64)
        if origin.size == 3:
            origin = np.tile(origin.reshape(3), (frames_no, 1))
        n_links = len(initial_angles)
        if n_links != STAGE_LINKS[stage]:
            raise ValueError(f"Your joints vector length is {n_links} but you have {STAGE_LINKS[stage]} links")
        seeds = {segment_name: {f"stage_{k}": np.zeros(STAGE_LINKS[k]) for k in (1, 2, 3, 4)}}
        seeds[segment_name][f"stage_{stage}"] = np.asarray(initial_angles, dtype=np.float64)
        lp = self._leg_params(segment_name, seeds)
        pose = np.zeros((1, 1, frames_no, 5, 3))
        pose[0, 0, :, 0] = origin
        pose[0, 0, :, stage] = end_effector_pos
        prior = self._prior_angles(segment_name, frames_no, stage)
        out = _lib.solve_seq(pose, [lp], stage, stage, angles=prior[None, None], want_fk=(stage == 4),
                             device=self.device)
        for dof in STAGE_DOFS[stage]:
            self.joint_angles_dict[f"Angle_{segment_name}_{dof}"] = out["angles"][0, 0, :, DOFS.index(dof)].copy()
        self.logger.debug("Stage %d is completed!", stage)
        if stage == 4:
            return out["fk"][0, 0]
        return np.full((frames_no, n_links, 3), np.nan)

    def run_ik_and_fk(self, export_path: Union[Path, str] = None, **kwargs
                      ) -> Tuple[Dict[str, np.ndarray], Dict[str, np.ndarray]]:
        """Inverse and forward kinematics of every leg.

        kwargs: ``stages`` (default [1, 2, 3, 4], consecutive), ``hide_progress_bar`` (accepted,
        unused: there is no per-frame host loop), ``diagnostics`` (also collect scipy status/nfev),
        ``frame_parallel``: how the serial frame loop of the reference (:259-282, frame t warm-started from frame
        t-1, :272) is mapped to the GPU --

        * ``False``: the reference's own order -- every chain is walked frame by frame, bit-identical to the oracle
          restatement of the reference.  (Environment variable ``SEQIK_FRAME_PARALLEL=0`` makes it the default of a
          process; an explicit argument always wins.)
        * ``"auto"`` (DEFAULT since round 6, see ``default_frame_parallel``): recordings of 48 frames and more are cut into
          frame chunks that are solved concurrently, verified
          against their true predecessor and repaired on the device (``SeqikOptions.frame_chunk = -1``,
          include/seqik.h): 10-70x faster for one recording.  Every frame is still solved by the reference's algorithm,
          from a warm start within 1e-6 rad of the serial one; the result equals the serial walk to ~1e-5 rad on
          well-posed frames (the reference's own run-to-run noise is ~5e-5 rad).  The chunk geometry is a function of
          the recording's length alone, so a recording gives the same bits alone, inside ``run_ik_and_fk_many`` or in a
          larger batch.  Applies to runs of all four stages without diagnostics; others are walked serially.  The
          library guards the speculation per leg: a leg of which more than one chunk in eight fails its first
          verification (poses with several equivalent leg configurations, kinematic singularities) is walked
          serially instead (``frame_chunk_report[leg]["walked_serially"]``).
        * ``True``: the same automatic geometry and per-leg guard as ``"auto"``, but a run that cannot be chunked (stage
          subsets, diagnostics) raises instead of silently walking serially.
        * a dict with any of ``chunk``, ``halo``, ``tol``, ``rounds``: explicit chunk parameters; an explicit ``chunk`` > 0
          runs WITHOUT the guard (the guard belongs to the automatic geometry, ``SeqikOptions.frame_chunk = -1``).

        ``missing_key_points``: ``"raise"`` (default) refuses a recording with a non-finite key point (``ValueError``, as
        scipy does in the reference); ``"skip"`` solves every leg as if its frames with a non-finite key point (rows 0-4,
        rows 1-4 with ``leg_affine``) were not in the recording -- frame t warm-started from the last complete frame
        before it (include/seqik_gaps.h).  Those frames get NaN angles and NaN FK rows (``run_fk`` / ``fit_error`` on the
        returned angles give NaN rows there too), status ``_lib.STATUS_MISSING`` and nfev 0 with ``diagnostics``;
        ``self.missing_frames[leg]`` holds the (N,) bool mask.  Skip mode needs ``stages=[1, 2, 3, 4]`` and works with
        every ``frame_parallel`` setting.

        After a chunked run ``self.frame_chunk_stats`` holds the statistics of the last launch and
        ``self.frame_chunk_report[leg]`` says where the recording was hard: ``frames_per_chunk``, ``run_in_frames``,
        ``failed_first_check`` (first frames of the chunks whose run-in did not reproduce the true state -- chaotic
        episodes show up here), ``frames_repaired``, ``walked_serially``.
        Returns ``(joint_angles_dict, forward_kinematics_dict)``."""
        stages = list(kwargs.get("stages", [1, 2, 3, 4]))
        diagnostics = bool(kwargs.get("diagnostics", False))
        skip = _lib.check_missing_mode(kwargs.get("missing_key_points", "raise"))
        if skip and stages != [1, 2, 3, 4]:
            raise ValueError("missing_key_points='skip' needs stages=[1, 2, 3, 4]")
        frame_parallel = kwargs.get("frame_parallel", default_frame_parallel())
        chunk_opts = dict(frame_chunk=0)
        if frame_parallel is not False and frame_parallel is not None:
            explicit = frame_parallel is True or isinstance(frame_parallel, dict)
            if explicit and (list(stages) != [1, 2, 3, 4] or diagnostics):
                raise ValueError("frame_parallel needs stages=[1, 2, 3, 4] and diagnostics=False")
            fp = frame_parallel if isinstance(frame_parallel, dict) else {}
            unknown = set(fp) - {"chunk", "halo", "tol", "rounds"}
            if unknown:
                raise ValueError(f"unknown frame_parallel options: {sorted(unknown)}")
            chunk_opts = dict(frame_chunk=int(fp.get("chunk", -1)), frame_halo=int(fp.get("halo", 0)),
                              chunk_tol=float(fp.get("tol", 0.0)), chunk_rounds=int(fp.get("rounds", 0)))
        if max(stages) > 4 or not all(np.diff(stages) == 1):
            raise ValueError("Maximum stage number is 4 and the list should be strictly incremental.")
        first_stage, last_stage = stages[0], stages[-1]
        forward_kinematics_dict = {}
        self.frame_chunk_stats, self.frame_chunk_report = {}, {}   # describe THIS run only (empty after a serial walk)
        self.missing_frames = {}
        self.logger.info("Computing joint angles and forward kinematics...")

        segments = self._leg_segments()
        # one launch per group of legs with the same number of frames (normally a single group)
        groups = {}
        for item in segments:
            groups.setdefault(np.asarray(item[2]).shape[0], []).append(item)
        for n_frames, items in groups.items():
            legs = [self._leg_params(leg_name) for _, leg_name, _ in items]
            pose = np.stack([np.asarray(arr, dtype=np.float64)[:, :5, :] for _, _, arr in items])[None]
            prior = np.stack([self._prior_angles(leg_name, n_frames, first_stage) for _, leg_name, _ in items])[None]
            affine = None
            if self.leg_affine is not None:
                affine = [_lib.make_affine(*self.leg_affine[leg_name]) for _, leg_name, _ in items]
            out = _lib.solve_seq(pose, legs, first_stage, last_stage, angles=prior, want_fk=True,
                                 want_diag=diagnostics, device=self.device, affine=affine,
                                 want_chunk_flags=chunk_opts["frame_chunk"] != 0 and not skip,
                                 missing="skip" if skip else "raise", **chunk_opts)
            if skip:
                rows = pose[0][:, :, 1:] if affine is not None else pose[0]
                for li, (_, leg_name, _) in enumerate(items):
                    self.missing_frames[leg_name] = ~np.isfinite(rows[li]).all(axis=(1, 2))
            self.frame_chunk_stats = out["chunk_stats"]
            self.frame_chunk_report.update(chunk_report(out, [leg_name for _, leg_name, _ in items], n_frames)[0])
            if out["chunk_stats"].get("chunks"):
                self.logger.info("%d frames x %d legs solved in %d verified frame chunks (frame_parallel='auto'; "
                                 "frame_parallel=False walks every chain frame by frame, as the reference does)",
                                 n_frames, len(items), out["chunk_stats"]["chunks"])
            for li, (segment_name, leg_name, _) in enumerate(items):
                for stage in stages:
                    for dof in STAGE_DOFS[stage]:
                        self.joint_angles_dict[f"Angle_{leg_name}_{dof}"] = out["angles"][0, li, :, DOFS.index(dof)].copy()
                if last_stage == 4:
                    forward_kinematics_dict[segment_name] = out["fk"][0, li].copy()
                else:  # the reference returns an uninitialised array here
                    forward_kinematics_dict[segment_name] = np.full((n_frames, STAGE_LINKS[last_stage], 3), np.nan)
                if diagnostics:
                    self.solver_status[leg_name] = out["status"][0, li].copy()
                    self.solver_nfev[leg_name] = out["nfev"][0, li].copy()
        # keep the reference's insertion order of the FK dict (dict order of aligned_pos)
        forward_kinematics_dict = {name: forward_kinematics_dict[name] for name, _, _ in segments}
        self.logger.debug("Joint angles and forward kinematics are computed.")
        self._export(export_path, forward_kinematics_dict)
        return self.joint_angles_dict, forward_kinematics_dict


class LegInvKinGeneric(LegInvKinBase):
    """Generic inverse kinematics: one 9-link chain per leg that only follows the claw
    (reference ``seqikpy/leg_inverse_kinematics.py:406-613``).

    The problem has 7 unknowns and 3 equations; which of the infinitely many solutions the
    reference reports is decided by LAPACK round-off inside scipy, so this class
    matches the reference in the claw position and respects the joint bounds, but the individual
    angles are *a* solution, not necessarily the reference's.

    >>> gen_ik = LegInvKinGeneric(aligned_pos, KinematicChainGeneric(BOUNDS, ["RF", "LF"]), INITIAL_ANGLES)
    >>> leg_joint_angles, forward_kinematics = gen_ik.run_ik_and_fk(export_path=DATA_PATH)
    """

    def __init__(self, aligned_pos: Dict[str, np.ndarray], kinematic_chain_class: KinematicChainGeneric,
                 initial_angles: Optional[Dict[str, np.ndarray]] = None,
                 log_level: Literal["DEBUG", "INFO", "WARNING", "ERROR"] = "INFO") -> None:
        super().__init__(aligned_pos, kinematic_chain_class, initial_angles, log_level)
        self.joint_angles_dict = {}

    _fk_kind = "generic"

    def _fk_key_points(self, leg_name, segment_array):
        arr = np.asarray(segment_array, dtype=np.float64)
        # the claw (last key point) is the end effector (:587), as in run_ik_and_fk
        return arr[:, [0, 1, 2, 3, -1], :] if arr.shape[1] >= 5 else arr

    def _leg_params(self, leg_name, seed9):
        kc = self.kinematic_chain_class
        seeds = {leg_name: {f"stage_{k}": np.zeros(STAGE_LINKS[k]) for k in (1, 2, 3)}}
        seeds[leg_name]["stage_4"] = np.asarray(seed9, dtype=np.float64)
        return _lib.make_leg_params(leg_name, kc.bounds_dof, kc.body_size, seeds)

    def run_angle_sensitivity(self, joint_angles=None, bound_tol=None):
        """Not defined for the generic chain: raises ``ValueError`` (see ``LegInvKinSeq.run_angle_sensitivity``)."""
        raise ValueError("the generic chain has no angle sensitivity: it fits seven angles to the three coordinates of the "
                         "claw, so the angles it reports are not a function of the key points (use LegInvKinSeq)")

    def angle_uncertainty(self, key_point_sigma, joint_angles=None, bound_tol=None, fit="sequential", key_point_weight=None,
                          smooth=None):
        """Not defined for the generic chain: raises ``ValueError`` (see ``LegInvKinSeq.angle_uncertainty``)."""
        return self.run_angle_sensitivity(joint_angles)

    def run_smooth_sensitivity(self, joint_angles=None, smooth=_lib.SMOOTH_DEFAULT, key_point_weight=None, half_width=0,
                               bound_tol=None):
        """Not defined for the generic chain: raises ``ValueError`` (see ``LegInvKinSeq.run_smooth_sensitivity``)."""
        return self.run_angle_sensitivity(joint_angles)

    def run_refine_sensitivity(self, joint_angles=None, key_point_weight=None, bound_tol=None):
        """Not defined for the generic chain: raises ``ValueError`` (see ``LegInvKinSeq.run_refine_sensitivity``)."""
        return self.run_angle_sensitivity(joint_angles)

    def run_refine(self, joint_angles=None, key_point_weight=None, export_path=None, **opts):
        """Not built for the generic chain: raises ``NotImplementedError`` (see ``LegInvKinSeq.run_refine``)."""
        raise NotImplementedError("the whole-leg refinement is built for the sequential chain only: the generic chain "
                                  "already fits all seven angles at once, to the claw alone (use LegInvKinSeq)")

    def run_smooth(self, joint_angles=None, smooth=_lib.SMOOTH_DEFAULT, key_point_weight=None, export_path=None,
                   key_point_sigma=None, bound_tol=None, **opts):
        """Not built for the generic chain: raises ``NotImplementedError`` (see ``LegInvKinSeq.run_smooth``)."""
        raise NotImplementedError("the trajectory refinement is built for the sequential chain only (use LegInvKinSeq)")

    def _store(self, leg_name, angles):
        # key order of the reference: the chain's link order, Base and Claw skipped (:533-539)
        for dof in ["ThC_roll", "ThC_yaw", "ThC_pitch", "CTr_pitch", "CTr_roll", "FTi_pitch", "TiTa_pitch"]:
            self.joint_angles_dict[f"Angle_{leg_name}_{dof}"] = angles[:, DOFS.index(dof)].copy()

    def calculate_ik_stage(self, end_effector_pos: np.ndarray, origin: np.ndarray, initial_angles: np.ndarray,
                           segment_name: str, **kwargs) -> np.ndarray:
        """Inverse kinematics of one leg over all frames; returns the joint positions ``(N, 9, 3)``."""
        if segment_name not in LEG_NAMES:
            raise ValueError(f"Segment name ({segment_name}) is not valid.")
        end_effector_pos = np.asarray(end_effector_pos, dtype=np.float64)
        frames_no = end_effector_pos.shape[0]
        origin = np.asarray(origin, dtype=np.float64)
        if origin.size == 3:
            origin = np.tile(origin.reshape(3), (frames_no, 1))
        if len(initial_angles) != 9:
            raise ValueError(f"Your joints vector length is {len(initial_angles)} but you have 9 links")
        pose = np.zeros((1, 1, frames_no, 5, 3))
        pose[0, 0, :, 0] = origin
        pose[0, 0, :, 4] = end_effector_pos
        out = _lib.solve_generic(pose, [self._leg_params(segment_name, initial_angles)], device=self.device)
        self._store(segment_name, out["angles"][0, 0])
        return out["fk"][0, 0]

    def run_ik_and_fk(self, export_path: Union[Path, str] = None, **kwargs
                      ) -> Tuple[Dict[str, np.ndarray], Dict[str, np.ndarray]]:
        """Inverse and forward kinematics of every leg with the generic chain.

        ``missing_key_points``: ``"raise"`` (default) or ``"skip"``, as for ``LegInvKinSeq.run_ik_and_fk``; here a frame is
        missing when its origin (key point 0) or its claw (the last key point) holds a non-finite coordinate.
        ``self.missing_frames[leg]`` holds the (N,) bool mask after a run."""
        skip = _lib.check_missing_mode(kwargs.get("missing_key_points", "raise"))
        self.missing_frames = {}
        forward_kinematics_dict = {}
        self.logger.info("Computing joint angles and forward kinematics...")
        segments = self._leg_segments()
        groups = {}
        for item in segments:
            groups.setdefault(np.asarray(item[2]).shape[0], []).append(item)
        for n_frames, items in groups.items():
            legs = [self._leg_params(leg, self.initial_angles[leg]["stage_4"]) for _, leg, _ in items]
            # the claw (last key point) is the end effector (:587)
            pose = np.stack([np.asarray(arr, dtype=np.float64)[:, [0, 1, 2, 3, -1], :] if np.asarray(arr).shape[1] >= 5
                             else np.asarray(arr, dtype=np.float64) for _, _, arr in items])[None]
            out = _lib.solve_generic(pose, legs, device=self.device, missing="skip" if skip else "raise")
            if skip:
                for li, (_, leg_name, _) in enumerate(items):
                    self.missing_frames[leg_name] = ~np.isfinite(pose[0, li][:, [0, 4]]).all(axis=(1, 2))
            for li, (segment_name, leg_name, _) in enumerate(items):
                self._store(leg_name, out["angles"][0, li])
                forward_kinematics_dict[segment_name] = out["fk"][0, li].copy()
        forward_kinematics_dict = {name: forward_kinematics_dict[name] for name, _, _ in segments}
        self.logger.debug("Joint angles and forward kinematics are computed.")
        self._export(export_path, forward_kinematics_dict)
        return self.joint_angles_dict, forward_kinematics_dict
