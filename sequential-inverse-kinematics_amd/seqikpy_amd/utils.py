"""Host helpers on either side of the leg-IK path: body sizes, the pickle formats, and the converters between the
pose / angle containers the reference's callers hold (DeepFly3D dictionaries) and the ``(N, key points, 3)`` /
``(N, dofs)`` arrays the solvers take and give, and the resampling of the resulting joint-angle series -- the
data-format part of the reference's ``seqikpy/utils.py`` (:89-123, :235-245, :293-362).  Not here: the stimulus /
video / DeepLabCut helpers of that file (not part of the path), its duplicates of AlignPose's private reductions, and
``from_anipose_to_array`` / ``df_to_nparray`` (:248-290), which assign a ``(3, N)`` block into an ``(N, 3)`` slot and so
only run for N == 3 -- nothing in the reference calls them."""
import pickle
from typing import Dict, List

import numpy as np

_ALL_LEGS = ["RF", "LF", "RM", "LM", "RH", "LH"]


def calculate_body_size(body_template: Dict[str, np.ndarray], legs_list: List[str] = None) -> Dict[str, float]:
    """Segment lengths from template joint positions (reference: ``seqikpy/utils.py:89-123``).

    ``body_size["<leg>_<segment>"]`` is the distance between consecutive template joints,
    ``body_size["<leg>"]`` the sum over the four segments.
    """
    legs_list = list(_ALL_LEGS) if legs_list is None else legs_list
    if set(legs_list).difference(_ALL_LEGS):
        raise NameError(
            f"""
            legs_list could only contain ["RF", "LF", "RM", "LM", "RH", "LH"],
            currently, it contains {legs_list}
            """
        )
    joints = ["Coxa", "Femur", "Tibia", "Tarsus", "Claw"]
    body_size = {}
    for i, segment in enumerate(joints[:-1]):
        for leg in legs_list:
            body_size[f"{leg}_{segment}"] = np.linalg.norm(
                body_template[f"{leg}_{segment}"] - body_template[f"{leg}_{joints[i + 1]}"]
            )
    for leg in legs_list:
        body_size[leg] = (body_size[f"{leg}_Coxa"] + body_size[f"{leg}_Femur"]
                          + body_size[f"{leg}_Tibia"] + body_size[f"{leg}_Tarsus"])
    if "R_Antenna_base" in body_template:
        body_size["Antenna"] = np.linalg.norm(body_template["R_Antenna_base"] - body_template["R_Antenna_edge"])
        body_size["Antenna_mid_thorax"] = np.linalg.norm(body_template["R_Antenna_base"] - body_template["Thorax_mid"])
    return body_size


def save_file(out_fname, data):
    """Pickle ``data`` (same on-disk format as the reference, ``seqikpy/utils.py:235-238``)."""
    with open(out_fname, "wb") as f:
        pickle.dump(data, f)


def load_file(output_fname):
    with open(output_fname, "rb") as f:
        return pickle.load(f)


def dict_to_nparray_pose(pose_dict, claw_is_end_effector: bool):
    """DeepFly3DPostProcessing leg dictionary (``{"Coxa": {"raw_pos_aligned": (N, 3)}, ...}``) ->
    ``(N, 4 or 5, 3)`` key-point array (reference ``seqikpy/utils.py:293-310``)."""
    key_points = ["Coxa", "Femur", "Tibia", "Tarsus"] + (["Claw"] if claw_is_end_effector else [])
    n = np.asarray(pose_dict["Coxa"]["raw_pos_aligned"]).shape[0]
    out = np.empty((n, len(key_points), 3))
    for i, kp in enumerate(key_points):
        out[:, i, :] = np.array(pose_dict[kp]["raw_pos_aligned"])
    return out


def dict_to_nparray_angle(angle_dict, leg, claw_is_end_effector):
    """DeepFly3DPostProcessing angle dictionary (``{"RF_leg": {"ThC_roll": (N,), ...}}``) -> ``(N, 7 or 6)`` in THAT
    format's column order -- roll, yaw, pitch, then CTr pitch / roll, FTi, (TiTa) (``seqikpy/utils.py:313-329``)."""
    dofs = ["ThC_roll", "ThC_yaw", "ThC_pitch", "CTr_pitch", "CTr_roll", "FTi_pitch"] + \
        (["TiTa_pitch"] if claw_is_end_effector else [])
    return np.stack([np.asarray(angle_dict[f"{leg}_leg"][d], dtype=np.float64) for d in dofs], axis=1)


def _reference_grid_check(n_frames, original_ts):
    """The reference builds its knots with ``np.arange(0, N * original_ts, original_ts)``; rounding can make that grid one
    element longer than the series (3 frames at 0.1 s, 1000 at 1/30 s), and scipy then refuses the pair."""
    n_knots = len(np.arange(0, n_frames * original_ts, original_ts))
    if n_knots != n_frames:
        raise ValueError(f"x and y arrays must be equal in length along interpolation axis: np.arange(0, "
                         f"{n_frames} * {original_ts!r}, {original_ts!r}) holds {n_knots} knots for {n_frames} samples")


def _is_plain_value(der):
    """``der=0`` as an int: the interpolant's value alone, the code path without derivatives."""
    return isinstance(der, (int, np.integer)) and not isinstance(der, (bool, np.bool_)) and der == 0


def _resample_series_on_gpu(stacked, orders, original_ts, new_ts, missing, max_gap):
    """Series of one length, stacked (C, N), each a chain of width 1 -> one (C, n_out) array per order; ``orders`` None:
    the value alone through ``_lib.resample_pchip``, else ``_lib.resample_pchip_der``."""
    from . import _lib
    y = stacked[:, :, None]
    if orders is None:
        res = (_lib.resample_pchip(y, original_ts, new_ts, missing=missing, max_gap=max_gap),)
    else:
        res = _lib.resample_pchip_der(y, original_ts, new_ts, der=orders, missing=missing, max_gap=max_gap)
    return [r[:, :, 0] for r in res]


def interpolate_signal(signal, original_ts, new_ts, on_gpu=False, missing="error", max_gap=None, der=0):
    """Resamples one series from time step ``original_ts`` to ``new_ts`` with a shape-preserving cubic (PCHIP) over
    ``[0, N * original_ts)`` (``seqikpy/utils.py:332-349``).  As there: if the interpolation fails, infinities and the
    last sample are zeroed IN the caller's array and it is tried once more.

    ``on_gpu=True`` runs the same interpolant on the GPU (``_lib.resample_pchip``, include/seqik_resample.h) and never
    modifies ``signal``: where the reference raises (non-finite values, fewer than 2 samples, a knot grid that
    ``np.arange`` makes longer than the series) it raises ``ValueError`` before anything is launched.
    ``missing="bridge"`` (GPU only) resamples over the finite samples alone and so fills the NaN frames of
    ``missing_key_points="skip"``; ``max_gap``: longest run of missing frames that is filled (None: any).

    ``der``: the derivative order of the interpolant to return -- 0 (default: the value, the code path as it was), 1
    (velocity, per unit of ``original_ts``) or 2 (acceleration) -- or a sequence of orders without repeats, which
    returns a list with one array per order.  The host path hands ``der`` to ``pchip_interpolate``; ``on_gpu=True``
    computes it with ``_lib.resample_pchip_der`` (include/seqik_resample_der.h), NaN exactly where the value is NaN."""
    plain = _is_plain_value(der)
    orders = None
    if not plain:
        from . import _lib
        orders = _lib._resample_orders(der)     # scipy alone would take any order: both paths accept the same ones
    if on_gpu:
        y = np.asarray(signal, dtype=np.float64)
        if y.ndim != 1:
            raise ValueError(f"signal must be one series (N,), got shape {y.shape}")
        if y.shape[0] < 2:
            raise ValueError("`x` must contain at least 2 elements.")
        _reference_grid_check(y.shape[0], original_ts)
        res = [r[0].copy() for r in _resample_series_on_gpu(y[None], orders, original_ts, new_ts, missing, max_gap)]
        return res if np.iterable(der) else res[0]
    if missing != "error" or max_gap is not None:
        raise ValueError("missing / max_gap need on_gpu=True (the host path is the reference's own)")
    from scipy.interpolate import pchip_interpolate
    total = signal.shape[0] * original_ts
    x_old, x_new = np.arange(0, total, original_ts), np.arange(0, total, new_ts)
    if not plain:
        if np.iterable(der):
            return [np.array(r) for r in pchip_interpolate(x_old, signal, x_new, der=list(orders))]
        return np.array(pchip_interpolate(x_old, signal, x_new, der=orders[0]))
    try:
        return np.array(pchip_interpolate(x_old, signal, x_new))
    except BaseException:  # noqa: B036 -- the reference's own breadth
        signal[np.isinf(signal)] = 0
        signal[-1] = 0
        return np.array(pchip_interpolate(x_old, signal, x_new))


def interpolate_joint_angles(joint_angles_dict, **kwargs):
    """``interpolate_signal`` over every series of a joint-angle dictionary (``run_ik_and_fk``'s first result);
    ``original_ts`` / ``new_ts`` as keyword arguments (``seqikpy/utils.py:352-360``).  With ``on_gpu=True`` ALL series go
    to the GPU in one call per series length (each series a chain of width 1) and the reference's dictionary comes
    back; ``missing`` / ``max_gap`` / ``der`` as for ``interpolate_signal`` (a sequence ``der`` gives every entry a list)."""
    if not kwargs.get("on_gpu", False):
        return {dof: interpolate_signal(signal=series, **kwargs) for dof, series in joint_angles_dict.items()}
    from . import _lib
    opts = dict(kwargs)
    opts.pop("on_gpu")
    original_ts, new_ts = opts.pop("original_ts"), opts.pop("new_ts")
    missing, max_gap, der = opts.pop("missing", "error"), opts.pop("max_gap", None), opts.pop("der", 0)
    orders = None if _is_plain_value(der) else _lib._resample_orders(der)
    if opts:
        raise TypeError(f"interpolate_signal() got an unexpected keyword argument {sorted(opts)[0]!r}")
    groups = {}
    for dof, series in joint_angles_dict.items():
        y = np.asarray(series, dtype=np.float64)
        if y.ndim != 1:
            raise ValueError(f"{dof}: expected one series (N,), got shape {y.shape}")
        if y.shape[0] < 2:
            raise ValueError("`x` must contain at least 2 elements.")
        _reference_grid_check(y.shape[0], original_ts)
        groups.setdefault(y.shape[0], []).append((dof, y))
    out = {}
    for items in groups.values():
        res = _resample_series_on_gpu(np.stack([y for _, y in items]), orders, original_ts, new_ts, missing, max_gap)
        for k, (dof, _) in enumerate(items):
            per_order = [r[k].copy() for r in res]
            out[dof] = per_order if np.iterable(der) else per_order[0]
    return {dof: out[dof] for dof in joint_angles_dict}
