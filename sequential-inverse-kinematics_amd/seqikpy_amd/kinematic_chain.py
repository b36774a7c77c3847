"""Kinematic chains of the sequential leg IK -- host-side mirror of the reference's
``seqikpy/kinematic_chain.py`` (``KinematicChainBase`` :27-74, ``KinematicChainSeq`` :77-421,
``KinematicChainGeneric`` :424-532).

The reference builds an ``ikpy.chain.Chain`` per stage (and, for stages 2-4, per frame).
Here a chain is a plain description -- link names, axes, translations, bounds -- that the
HIP library turns into per-(leg, stage) constants once; nothing symbolic, nothing per frame.
The public surface is kept: class names, constructor arguments, ``body_size`` /
``bounds_dof`` attributes, ``create_leg_chain(leg_name, angles=, stage=, t=)`` and the
``ValueError`` conditions.  Returned chains carry the part of IKPy's ``Chain`` / ``Link`` interface the
reference's callers use: ``.name``, ``.links[i].name`` / ``.bounds`` / ``.get_link_frame_matrix(theta)``,
``.active_links_mask``, ``.forward_kinematics(joints, full_kinematics=)`` (host numpy: one frame is not worth a
launch) and ``.inverse_kinematics(target_position=, initial_position=)`` (one single-frame launch of the HIP solver);
``.forward_kinematics_many(joints)`` is the batched form, on the GPU for factory-made chains
(``include/seqik_frames.h``).
"""
from abc import ABC, abstractmethod
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from .data import DOFS, NMF_TEMPLATE, SEGMENTS
from .utils import calculate_body_size

LEG_NAMES = ["RF", "LF", "RM", "LM", "RH", "LH"]

X_AXIS = (1, 0, 0)
Y_AXIS = (0, 1, 0)
Z_AXIS = (0, 0, 1)

#: joints stored by each stage (leg_inverse_kinematics.py:285-320)
STAGE_DOFS = {1: ["ThC_yaw", "ThC_pitch"], 2: ["ThC_roll", "CTr_pitch"], 3: ["CTr_roll", "FTi_pitch"],
              4: ["TiTa_pitch"]}
STAGE_LINKS = {1: 4, 2: 6, 3: 8, 4: 9}
#: link order of the whole-leg chains (``_lib.link_frames``): base, seven joints, claw
WHOLE_LEG_LINKS = {"seq": ["ThC_yaw", "ThC_pitch", "ThC_roll", "CTr_pitch", "CTr_roll", "FTi_pitch", "TiTa_pitch"],
                   "generic": ["ThC_roll", "ThC_yaw", "ThC_pitch", "CTr_pitch", "CTr_roll", "FTi_pitch", "TiTa_pitch"]}


def _rot(axis, a):
    """IKPy's axis rotation: the un-normalised Rodrigues form (a zero axis gives cos(a) . I)."""
    c, s = np.cos(a), np.sin(a)
    x, y, z = axis
    return np.array([[x * x + (1 - x * x) * c, x * y * (1 - c) - z * s, x * z * (1 - c) + y * s],
                     [x * y * (1 - c) + z * s, y * y + (1 - y * y) * c, y * z * (1 - c) - x * s],
                     [x * z * (1 - c) - y * s, y * z * (1 - c) + x * s, z * z + (1 - z * z) * c]])


def _joints_error(n_joints, n_links):
    return ValueError(f"Your joints vector length is {n_joints} but you have {n_links} links")


def _strictly_feasible_start(links, x0):
    """scipy shifts start entries that sit on a bound inwards by 1e-10 * max(1, |bound|)."""
    res = x0.copy()
    lo = np.array([l.bounds[0] for l in links])
    hi = np.array([l.bounds[1] for l in links])
    with np.errstate(invalid="ignore"):  # the base link is unbounded (-inf, inf)
        near_lo = np.isfinite(lo) & (res - lo <= np.minimum(hi - res, 1e-10 * np.maximum(1, np.abs(lo))))
        near_hi = np.isfinite(hi) & (hi - res <= np.minimum(res - lo, 1e-10 * np.maximum(1, np.abs(hi))))
        res[near_lo] = (lo + 1e-10 * np.maximum(1, np.abs(lo)))[near_lo]
        res[near_hi] = (hi - 1e-10 * np.maximum(1, np.abs(hi)))[near_hi]
    return res


class Link:
    """One link of a chain: ``T(origin_translation) . RPY(origin_orientation) . R(rotation, theta)``."""

    def __init__(self, name: str, origin_translation=(0, 0, 0), origin_orientation=(0, 0, 0),
                 rotation: Optional[Sequence[float]] = None, joint_type: str = "revolute",
                 bounds=(-np.inf, np.inf)):
        self.name = name
        self.origin_translation = np.asarray(origin_translation, dtype=np.float64)
        self.origin_orientation = np.asarray(origin_orientation, dtype=np.float64)
        self.rotation = None if rotation is None else np.asarray(rotation, dtype=np.float64)
        self.joint_type = joint_type
        self.bounds = (float(bounds[0]), float(bounds[1]))

    @property
    def has_rotation(self) -> bool:
        return self.joint_type == "revolute" and self.rotation is not None

    def get_link_frame_matrix(self, theta) -> np.ndarray:
        """4 x 4 frame of this link at joint variable ``theta`` (ignored by fixed links and the base link)."""
        m = np.eye(4)
        m[:3, 3] = self.origin_translation
        r, p, y = self.origin_orientation
        m[:3, :3] = _rot((0, 0, 1), y) @ _rot((0, 1, 0), p) @ _rot((1, 0, 0), r)
        if self.has_rotation:
            h = np.eye(4)
            h[:3, :3] = _rot(tuple(self.rotation), theta)
            m = m @ h
        return m

    def __repr__(self):
        return f"Link(name={self.name!r}, joint_type={self.joint_type!r}, bounds={self.bounds})"


def OriginLink() -> Link:
    return Link("Base link", joint_type="fixed")


class Chain:
    """Ordered list of links with the methods of ``ikpy.chain.Chain`` the reference's callers use.  ``spec`` records how
    the HIP library should solve it; ``device`` is the HIP device ordinal of its launches (-1 = the calling thread's
    current device)."""

    def __init__(self, name: str, links: List[Link], spec: Optional[dict] = None):
        self.name = name
        self.links = links
        self.spec = spec or {}
        self.device = -1

    def __len__(self):
        return len(self.links)

    def __repr__(self):
        return f"Chain(name={self.name!r}, links={[l.name for l in self.links]})"

    @property
    def active_links_mask(self) -> np.ndarray:
        """IKPy's default: every link active (the reference never passes a mask)."""
        return np.ones(len(self.links), dtype=bool)

    # -- forward kinematics ------------------------------------------------------------
    def forward_kinematics(self, joints, full_kinematics: bool = False):
        """The 4 x 4 frame of the last link at the joint vector ``joints`` (one entry per link), or with
        ``full_kinematics`` the list of the frames of all links.  Host numpy; works on any chain."""
        if len(joints) != len(self.links):
            raise _joints_error(len(joints), len(self.links))
        frame = np.eye(4)
        frames = []
        for link, theta in zip(self.links, joints):
            frame = frame @ link.get_link_frame_matrix(theta)
            if full_kinematics:
                frames.append(frame)
        return frames if full_kinematics else frame

    def _whole_leg_angles(self, joints):
        """(angles (N, 7) in DOFS order, indices of this chain's links among the nine of the whole-leg chain) when
        ``_lib.link_frames`` computes this chain's frames, else None: the chain must come from a factory and the base
        and claw variables must be 0 (the library never moves them)."""
        kind, factory = self.spec.get("kind"), self.spec.get("factory")
        if kind not in WHOLE_LEG_LINKS or factory is None:
            return None
        leg = self.spec["leg"]
        whole = ["Base link"] + [f"{leg}_{dof}" for dof in WHOLE_LEG_LINKS[kind]] + [f"{leg}_Claw"]
        names = [l.name for l in self.links]
        if any(n not in whole for n in names) or joints[:, 0].any():
            return None
        if names[-1] == whole[-1] and joints[:, -1].any():
            return None
        angles = np.zeros((joints.shape[0], 7))
        prior = self.spec.get("prior_angles")
        if prior is not None:
            angles[:] = prior  # the fixed links; the joints of later stages are 0 there
        for i, link in enumerate(self.links):
            dof = link.name[len(leg) + 1:]
            if link.has_rotation and dof in DOFS:
                angles[:, DOFS.index(dof)] = joints[:, i]
        return angles, [whole.index(n) for n in names]

    def forward_kinematics_many(self, joints) -> np.ndarray:
        """``forward_kinematics(q, full_kinematics=True)`` for N joint vectors at once: (N, len(links)) ->
        (N, len(links), 4, 4).  Chains made by ``KinematicChainSeq`` / ``KinematicChainGeneric`` go through the GPU
        (``_lib.link_frames``): a stage chain is the whole-leg chain with the later joints at 0 and a subset of its links.
        A chain assembled by hand, or a non-zero base or claw variable, is walked on the host; the two routes agree to
        1e-12."""
        joints = np.asarray(joints, dtype=np.float64)
        if joints.ndim != 2 or joints.shape[1] != len(self.links):
            raise _joints_error(joints.shape[-1] if joints.ndim else 0, len(self.links))
        route = self._whole_leg_angles(joints) if joints.shape[0] else None
        if route is None:
            out = np.empty((joints.shape[0], len(self.links), 4, 4))
            for t in range(joints.shape[0]):
                out[t] = self.forward_kinematics(joints[t], full_kinematics=True)
            return out
        angles, pick = route
        lp = _lib.SeqikLegParams()
        for i, seg in enumerate(SEGMENTS):
            lp.seg[i] = float(self.spec["factory"].body_size[f"{self.spec['leg']}_{seg}"])
        frames = _lib.link_frames(angles[None, None], [lp], kind=self.spec["kind"], device=self.device)["frames"]
        return np.ascontiguousarray(frames[0, 0][:, pick])

    # -- inverse kinematics ------------------------------------------------------------
    def inverse_kinematics(self, target_position=None, initial_position=None, **kwargs) -> np.ndarray:
        """Joint variables (one per link) that bring the end effector closest to ``target_position`` (default: the
        origin), started from ``initial_position`` (default: zeros): one single-frame launch of the HIP solver -- one
        stage of ``seqik_solve_seq`` for a stage chain, ``seqik_solve_generic`` for the generic chain (base and claw keep
        their start values, made strictly feasible as scipy does).  The batched entry points are the fast path; this
        exists for callers that hold the chain object.  ``device=`` overrides ``self.device`` for the call.  Needs a
        chain made by ``KinematicChainSeq`` / ``KinematicChainGeneric``; IKPy's other keyword arguments (orientation
        targets and the like) are refused by name."""
        device = kwargs.pop("device", None)
        if kwargs:
            raise TypeError(f"inverse_kinematics() got unsupported keyword arguments: {sorted(kwargs)}")
        device = self.device if device is None else device
        spec = self.spec
        kind = spec.get("kind")
        if kind not in ("seq", "generic"):
            raise ValueError("calculate_ik needs a chain made by KinematicChainSeq / KinematicChainGeneric")
        leg, factory = spec["leg"], spec["factory"]
        stage = spec["stage"] if kind == "seq" else 4
        n = STAGE_LINKS[stage]
        x0 = np.zeros(n) if initial_position is None else np.asarray(initial_position, dtype=np.float64)
        if x0.shape != (n,):
            raise _joints_error(x0.size, n)
        target = np.zeros(3) if target_position is None else np.asarray(target_position, dtype=np.float64)
        stages = (1, 2, 3, 4) if kind == "seq" else (1, 2, 3)
        seeds = {leg: {f"stage_{k}": np.zeros(STAGE_LINKS[k]) for k in stages}}
        seeds[leg][f"stage_{stage}"] = x0
        lp = _lib.make_leg_params(leg, factory.bounds_dof, factory.body_size, seeds)
        pose = np.zeros((1, 1, 1, 5, 3))
        pose[0, 0, 0, stage] = target
        if kind == "seq":
            angles = np.zeros((1, 1, 1, 7))
            if spec["prior_angles"] is not None:
                angles[0, 0, 0] = spec["prior_angles"]
            out = _lib.solve_seq(pose, [lp], stage, stage, angles=angles, want_fk=False, device=device)
            solved = STAGE_DOFS[stage]
        else:
            out = _lib.solve_generic(pose, [lp], want_fk=False, device=device)
            solved = DOFS
        res = _strictly_feasible_start(self.links, x0)
        names = [l.name for l in self.links]
        for dof in solved:
            res[names.index(f"{leg}_{dof}")] = out["angles"][0, 0, 0, DOFS.index(dof)]
        return res


class KinematicChainBase(ABC):
    """Abstract class to create kinematic chains for the legs.

    Parameters
    ----------
    bounds_dof : Dict[str, tuple]
        Bounds of the joint degrees of freedom, ``"<leg>_<dof>" -> (lb, ub)``.
    legs_list : List[str]
        Legs for which chains are created.
    body_size : Dict[str, float], optional
        Segment sizes; computed from ``NMF_TEMPLATE`` when ``None``.
    """

    def __init__(self, bounds_dof: Dict[str, np.ndarray], legs_list: List[str],
                 body_size: Dict[str, float] = None) -> None:
        self.body_size = calculate_body_size(NMF_TEMPLATE, legs_list) if body_size is None else body_size
        self.bounds_dof = bounds_dof
        self.legs_list = list(legs_list)

    def __call__(self):
        print("Base kinematic chain is called.")

    @abstractmethod
    def create_leg_chain(self, leg_name: str, **kwargs) -> Chain:
        raise NotImplementedError


def _angle(angles, key, t):
    return float(np.asarray(angles[key])[t])


class KinematicChainSeq(KinematicChainBase):
    """Sequential kinematic chain: one chain per stage (yaw-pitch-roll order)."""

    def __call__(self):
        print("Sequential kinematic chain is called.")

    def create_leg_chain(self, leg_name: str, **kwargs) -> Chain:
        angles = kwargs.get("angles", None)
        stage = kwargs.get("stage", 1)
        t = kwargs.get("t", 0)
        if leg_name not in LEG_NAMES:
            raise ValueError(f"Unknown leg name ({leg_name}) is provided!")
        if not 1 <= stage <= 4:
            raise ValueError(f"Unknown stage number ({stage}) number is provided!")
        if stage == 1:
            return self.create_leg_chain_stage_1(leg_name)
        if stage == 2:
            return self.create_leg_chain_stage_2(leg_name, angles=angles, t=t)
        if stage == 3:
            return self.create_leg_chain_stage_3(leg_name, angles=angles, t=t)
        return self.create_leg_chain_stage_4(leg_name, angles=angles, t=t)

    # -- helpers ---------------------------------------------------------------------
    def _b(self, leg, dof):
        return self.bounds_dof[f"{leg}_{dof}"]

    def _rev(self, leg, dof, axis, segment=None):
        tz = 0.0 if segment is None else -self.body_size[f"{leg}_{segment}"]
        return Link(f"{leg}_{dof}", (0, 0, tz), (0, 0, 0), axis, "revolute", self._b(leg, dof))

    def _fix(self, leg, dof, axis, angles, t, segment=None):
        tz = 0.0 if segment is None else -self.body_size[f"{leg}_{segment}"]
        a = _angle(angles, f"Angle_{leg}_{dof}", t)
        rpy = {X_AXIS: (a, 0, 0), Y_AXIS: (0, a, 0), Z_AXIS: (0, 0, a)}[axis]
        return Link(f"{leg}_{dof}", (0, 0, tz), rpy, None, "fixed", self._b(leg, dof))

    def _spec(self, leg, stage, angles, t):
        prior = None
        if stage > 1:
            prior = np.zeros(7)
            dofs = ["ThC_yaw", "ThC_pitch", "ThC_roll", "CTr_pitch", "CTr_roll", "FTi_pitch"][: 2 * (stage - 1)]
            for i, dof in enumerate(dofs):
                prior[i] = _angle(angles, f"Angle_{leg}_{dof}", t)
        return dict(kind="seq", leg=leg, stage=stage, prior_angles=prior, factory=self)

    # -- stages ----------------------------------------------------------------------
    def create_leg_chain_stage_1(self, leg_name: str) -> Chain:
        """Thorax/coxa yaw and pitch; contains the coxa only."""
        links = [
            OriginLink(),
            self._rev(leg_name, "ThC_yaw", X_AXIS),
            self._rev(leg_name, "ThC_pitch", Y_AXIS),
            self._rev(leg_name, "CTr_pitch", Y_AXIS, "Coxa"),
        ]
        return Chain("chain_stage_1", links, self._spec(leg_name, 1, None, 0))

    def create_leg_chain_stage_2(self, leg_name: str, angles: Dict[str, np.ndarray], t: int) -> Chain:
        """Thorax/coxa roll and coxa/trochanter pitch; coxa + femur."""
        links = [
            OriginLink(),
            self._fix(leg_name, "ThC_yaw", X_AXIS, angles, t),
            self._fix(leg_name, "ThC_pitch", Y_AXIS, angles, t),
            self._rev(leg_name, "ThC_roll", Z_AXIS),
            self._rev(leg_name, "CTr_pitch", Y_AXIS, "Coxa"),
            self._rev(leg_name, "FTi_pitch", Y_AXIS, "Femur"),
        ]
        return Chain("chain_stage_2", links, self._spec(leg_name, 2, angles, t))

    def create_leg_chain_stage_3(self, leg_name: str, angles: Dict[str, np.ndarray], t: int) -> Chain:
        """Coxa/trochanter roll and femur/tibia pitch; coxa + femur + tibia."""
        links = [
            OriginLink(),
            self._fix(leg_name, "ThC_yaw", X_AXIS, angles, t),
            self._fix(leg_name, "ThC_pitch", Y_AXIS, angles, t),
            self._fix(leg_name, "ThC_roll", Z_AXIS, angles, t),
            self._fix(leg_name, "CTr_pitch", Y_AXIS, angles, t, "Coxa"),
            self._rev(leg_name, "CTr_roll", Z_AXIS),
            self._rev(leg_name, "FTi_pitch", Y_AXIS, "Femur"),
            self._rev(leg_name, "TiTa_pitch", Y_AXIS, "Tibia"),
        ]
        return Chain("chain_stage_3", links, self._spec(leg_name, 3, angles, t))

    def create_leg_chain_stage_4(self, leg_name: str, angles: Dict[str, np.ndarray], t: int) -> Chain:
        """Tibia/tarsus pitch; the entire leg."""
        links = [
            OriginLink(),
            self._fix(leg_name, "ThC_yaw", X_AXIS, angles, t),
            self._fix(leg_name, "ThC_pitch", Y_AXIS, angles, t),
            self._fix(leg_name, "ThC_roll", Z_AXIS, angles, t),
            self._fix(leg_name, "CTr_pitch", Y_AXIS, angles, t, "Coxa"),
            self._fix(leg_name, "CTr_roll", Z_AXIS, angles, t),
            self._fix(leg_name, "FTi_pitch", Y_AXIS, angles, t, "Femur"),
            self._rev(leg_name, "TiTa_pitch", Y_AXIS, "Tibia"),
            Link(f"{leg_name}_Claw", (0, 0, -self.body_size[f"{leg_name}_Tarsus"]), (0, 0, 0), (0, 0, 0),
                 "revolute", (-np.pi, np.pi)),
        ]
        return Chain("chain_stage_4", links, self._spec(leg_name, 4, angles, t))


class KinematicChainGeneric(KinematicChainBase):
    """Generic kinematic chain: one 9-link chain for the entire leg."""

    def __call__(self):
        print("Generic kinematic chain is called.")

    def create_leg_chain(self, leg_name: str, **kwargs) -> Chain:
        if leg_name not in LEG_NAMES:
            raise ValueError(f"Unknown leg name ({leg_name}) is provided!")
        b = self.bounds_dof
        size = self.body_size

        def rev(dof, axis, segment=None):
            tz = 0.0 if segment is None else -size[f"{leg_name}_{segment}"]
            return Link(f"{leg_name}_{dof}", (0, 0, tz), (0, 0, 0), axis, "revolute", b[f"{leg_name}_{dof}"])

        links = [
            OriginLink(),
            rev("ThC_roll", Z_AXIS),
            rev("ThC_yaw", X_AXIS),
            rev("ThC_pitch", Y_AXIS),
            rev("CTr_pitch", Y_AXIS, "Coxa"),
            rev("CTr_roll", Z_AXIS),
            rev("FTi_pitch", Y_AXIS, "Femur"),
            rev("TiTa_pitch", Y_AXIS, "Tibia"),
            Link(f"{leg_name}_Claw", (0, 0, -size[f"{leg_name}_Tarsus"]), (0, 0, 0), (0, 0, 0), "revolute",
                 (-np.pi, np.pi)),
        ]
        return Chain("chain", links, dict(kind="generic", leg=leg_name, factory=self))
