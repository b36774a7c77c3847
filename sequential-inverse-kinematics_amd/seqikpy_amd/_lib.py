"""ctypes binding of ``libseqik_hip.so`` (C ABI: ``include/seqik.h``).

There is no CPU implementation behind this module: if the HIP library is missing, or no
GPU is visible when a solve is requested, the call raises.  ``build()`` compiles the
library in-tree with hipcc for gfx950 (cross-compiles without a GPU).
"""
import ctypes
import os
import subprocess
import threading

import numpy as np

from .data import DOFS, SEGMENTS

_PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(_PKG), "csrc")
# installed (pyproject.toml / setup.py): the built library inside the package wins whenever it exists; the source tree is
# recognised by a file of THIS project next to the package -- a stray top-level csrc/ in site-packages (several native packages
# install one) must not switch an installed package into tree mode (round-5 advice)
_NATIVE = os.path.join(_PKG, "_native")
_IN_TREE = not os.path.isfile(os.path.join(_NATIVE, "libseqik_hip.so")) and os.path.isfile(os.path.join(CSRC, "seqik_hip.hip"))
_LIB_DIR = CSRC if _IN_TREE else _NATIVE
LIB_PATH = os.environ.get("SEQIK_LIB", os.path.join(_LIB_DIR, "libseqik_hip.so"))  # SEQIK_LIB: A/B builds
COMPILE_UNITS = ["seqik_hip.hip", "seqik_runtime.hip", "seqik_head.hip", "seqik_stream.hip", "seqik_align.hip",
                 "seqik_peer.hip", "seqik_fk.hip", "seqik_gaps.hip", "seqik_resample.hip", "seqik_frames.hip",
                 "seqik_head_align.hip", "seqik_jacobian.hip", "seqik_sensitivity.hip", "seqik_refine.hip",
                 "seqik_smooth.hip", "seqik_refine_sens.hip", "seqik_smooth_sens.hip"]
CSRC_HEADERS = ["seqik_core.hpp", "seqik_consts.hpp", "seqik_head.hpp", "seqik_generic.hpp", "seqik_device_scope.hpp",
                "seqik_runtime.hpp", "seqik_fk.hpp", "seqik_gaps.hpp", "seqik_resample.hpp", "seqik_frames.hpp",
                "seqik_head_align.hpp", "seqik_jacobian.hpp", "seqik_leg_map.hpp", "seqik_head_launch.hpp",
                "seqik_order_stats.hpp", "seqik_sensitivity.hpp", "seqik_refine.hpp", "seqik_leg_chain.hpp",
                "seqik_smooth.hpp", "seqik_refine_sens.hpp", "seqik_smooth_sens.hpp"]
SOURCES = COMPILE_UNITS + CSRC_HEADERS   # what a build depends on
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17"]

SEQIK_OK = 0
ERR_HIP, ERR_X0, ERR_BOUNDS, ERR_ARG, ERR_STAGE = -1, -2, -3, -4, -5

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_u8p = ctypes.POINTER(ctypes.c_uint8)


class SeqikLegParams(ctypes.Structure):
    """Mirror of ``struct SeqikLegParams`` (include/seqik.h)."""
    _fields_ = [("seg", ctypes.c_double * 4),
                ("bounds", (ctypes.c_double * 2) * 7),
                ("seeds", ctypes.c_double * 27)]


class SeqikOptions(ctypes.Structure):
    """Mirror of ``struct SeqikOptions`` (include/seqik.h; unchanged since ABI 3)."""
    _fields_ = [("device", ctypes.c_int32), ("block_size", ctypes.c_int32),
                ("stage_events", ctypes.POINTER(ctypes.c_void_p)), ("reserved", ctypes.c_int32 * 4),
                ("frame_chunk", ctypes.c_int32), ("frame_halo", ctypes.c_int32), ("chunk_tol", ctypes.c_double),
                ("chunk_rounds", ctypes.c_int32), ("frame_lead", ctypes.c_int32),
                ("chunk_stats", ctypes.POINTER(ctypes.c_int32)),
                ("chunk_flags", ctypes.POINTER(ctypes.c_uint8)), ("chunk_states", ctypes.POINTER(ctypes.c_double)),
                ("chunk_resume", ctypes.c_int32), ("pad2_", ctypes.c_int32)]


ABI_VERSION = 7
N_CHUNK_STATS = 16
CHUNK_STATS_FIELDS = ("chunks", "frames_per_chunk", "run_in_frames", "repaired_round_1", "repaired_round_2",
                      "repaired_later_rounds", "repaired_by_sweep", "inconsistent_at_first_check",
                      "chains_walked_serially", "chunks_of_those_chains")
CHUNK_FLAG_FAILED_FIRST, CHUNK_FLAG_REPAIRED, CHUNK_FLAG_SWEPT, CHUNK_FLAG_SERIAL = 1, 2, 4, 8
CHUNK_FLAG_LEFT_BLOCKED = 0x80   # input of a lockstep round (chunk_resume = 4), see include/seqik.h


def chunk_stats_dict(stats):
    """int32[16] of ``SeqikOptions.chunk_stats`` -> dict (all zero: the call ran serially; ``chains_walked_serially``:
    chains the automatic mode's per-chain guard handed to the serial walk because more than one of their chunks in eight
    failed the first verification)."""
    return {k: int(v) for k, v in zip(CHUNK_STATS_FIELDS, stats)}


def selftest_div_sqrt(a, b):
    """(a / b, sqrt(a)) as the kernels compute them on the device (``seqik_selftest_div_sqrt``)."""
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    b = np.ascontiguousarray(b, dtype=np.float64).ravel()
    if a.shape != b.shape:
        raise ValueError("a and b must have the same number of elements")
    q, r = np.empty_like(a), np.empty_like(a)
    _call("seqik_selftest_div_sqrt", _data(a), _data(b), _data(q), _data(r), a.size)
    return q, r


def selftest_sqrt_pos(a):
    """sqrt(a) as the kernels compute it for the Coleman-Li distances (``sqrt_pos_``: no zero / infinity selects)."""
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    r = np.empty_like(a)
    _call("seqik_selftest_sqrt_pos", _data(a), _data(r), a.size)
    return r


def check_faults(stream=None):
    """``seqik_check_faults`` / ``seqik_check_faults_stream``: raises ``SeqikLibraryError`` when a kernel launched through
    the asynchronous device entry points reported a fault (the stage pipeline's watchdog) since the last check.  Call it
    after synchronising.  ``stream=None``: every stream of the process (single-threaded callers); ``stream=<hipStream_t as
    int>`` (0 = the default stream): the launches made on that stream of the current device only -- what a host thread
    that shares the process with other threads' GPUs / streams uses (ABI 6)."""
    if stream is None:
        _call("seqik_check_faults")
    else:
        _call("seqik_check_faults_stream", _stream_ptr(stream))


def frame_chunk_plan(n_frames, frame_chunk=-1, frame_halo=0, frame_lead=0):
    """``seqik_frame_chunk_plan``: (frames per chunk, run-in frames, chunks per chain) a call over recordings of
    ``n_frames`` frames would use -- (0, 0, 0) when it would be walked serially.  No GPU needed."""
    opt = SeqikOptions(frame_chunk=int(frame_chunk), frame_halo=int(frame_halo), frame_lead=int(frame_lead))
    c, h, k = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0)
    _call("seqik_frame_chunk_plan", int(n_frames), ctypes.byref(opt), ctypes.byref(c), ctypes.byref(h), ctypes.byref(k))
    return int(c.value), int(h.value), int(k.value)


class SeqikLayout(ctypes.Structure):
    """Mirror of ``struct SeqikLayout``: element strides of the device buffers."""
    _fields_ = [("pose_chain", ctypes.c_int64), ("pose_row", ctypes.c_int64), ("pose_frame", ctypes.c_int64),
                ("ang_chain", ctypes.c_int64), ("ang_dof", ctypes.c_int64), ("ang_frame", ctypes.c_int64)]


def planar_layout(n_frames: int) -> SeqikLayout:
    """pose [chain][5][frame][3], angles [chain][7][frame]: every key-point row / joint a time series."""
    return SeqikLayout(15 * n_frames, 3 * n_frames, 3, 7 * n_frames, n_frames, 1)


class SeqikAffine(ctypes.Structure):
    """Mirror of ``struct SeqikAffine``: fused AlignPose.align_leg of one leg."""
    _fields_ = [("fixed_coxa", ctypes.c_double * 3), ("scale", ctypes.c_double),
                ("template_coxa", ctypes.c_double * 3)]


def make_affine(fixed_coxa, scale, template_coxa) -> SeqikAffine:
    a = SeqikAffine()
    for i in range(3):
        a.fixed_coxa[i] = float(fixed_coxa[i])
        a.template_coxa[i] = float(template_coxa[i])
    a.scale = float(scale)
    return a


class SeqikHeadAffine(ctypes.Structure):
    """Mirror of ``struct SeqikHeadAffine`` (include/seqik_head_align.h): fused AlignPose.align_head of one side."""
    _fields_ = [("origin", ctypes.c_double * 3), ("scale_base", ctypes.c_double), ("scale_tip", ctypes.c_double),
                ("template_base", ctypes.c_double * 3)]


class SeqikRefineOptions(ctypes.Structure):
    """Mirror of ``struct SeqikRefineOptions`` (include/seqik_refine.h)."""
    _fields_ = [("max_iter", ctypes.c_int32), ("gtol", ctypes.c_double), ("ftol", ctypes.c_double)]


class SeqikSmoothOptions(ctypes.Structure):
    """Mirror of ``struct SeqikSmoothOptions`` (include/seqik_smooth.h)."""
    _fields_ = [("smooth", ctypes.c_double * 7), ("max_iter", ctypes.c_int32), ("gtol", ctypes.c_double),
                ("ftol", ctypes.c_double)]


def make_head_affine(origin, scale_base, scale_tip, template_base) -> SeqikHeadAffine:
    a = SeqikHeadAffine()
    for i in range(3):
        a.origin[i] = float(origin[i])
        a.template_base[i] = float(template_base[i])
    a.scale_base, a.scale_tip = float(scale_base), float(scale_tip)
    return a


# The C ABI as ctypes sees it, one line per entry point of each header under include/: (name, return type, parameter
# types...).  ``load()`` applies it; tests/test_capi_symbols.py holds it against the prototypes.  Device pointers, streams
# and handles are ``void *`` here whatever the header's pointee type, so that wrappers and tests can pass plain ints.
_int, _i32, _i64, _f64, _size = ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_size_t
_vp, _vpp, _cp, _i64p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64)
_legs, _opt, _lay = ctypes.POINTER(SeqikLegParams), ctypes.POINTER(SeqikOptions), ctypes.POINTER(SeqikLayout)
_aff, _haff = ctypes.POINTER(SeqikAffine), ctypes.POINTER(SeqikHeadAffine)
_ropt = ctypes.POINTER(SeqikRefineOptions)
SIGNATURES = {
    "seqik.h": (
        ("seqik_abi_version", _int),
        ("seqik_device_count", _int),
        ("seqik_last_error", _cp),
        ("seqik_device_attributes", _int, _i32, _ip, _ip, _i64p),
        ("seqik_release_workspaces", _int),
        ("seqik_validate_legs", _int, _legs, _i32, _i32, _i32),
        ("seqik_solve_seq", _int, _dp, _i64, _i32, _i64, _legs, _i32, _i32, _dp, _dp, _ip, _ip, _dp, _aff, _opt),
        ("seqik_selftest_div_sqrt", _int, _dp, _dp, _dp, _dp, _i64),
        ("seqik_selftest_sqrt_pos", _int, _dp, _dp, _i64),
        ("seqik_check_faults", _int),
        ("seqik_check_faults_stream", _int, _vp),
        ("seqik_frame_chunk_plan", _int, _i64, _opt, _ip, _ip, _i64p),
        ("seqik_solve_seq_device", _int, _vp, _i64, _i32, _i64, _legs, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _lay, _aff, _opt, _vp),
        ("seqik_validate_legs_generic", _int, _legs, _i32),
        ("seqik_solve_generic", _int, _dp, _i64, _i32, _i64, _legs, _dp, _dp, _ip, _ip, _dp, _aff, _opt),
        ("seqik_solve_generic_device", _int, _vp, _i64, _i32, _i64, _legs, _vp, _vp, _vp, _vp, _vp, _lay, _aff, _opt, _vp),
        ("seqik_head_angles", _int, _dp, _dp, _i64, _dp, _i64, _f64, _f64, _i32, _dp, _opt),
        ("seqik_head_angles_device", _int, _vp, _vp, _i64, _vp, _i64, _f64, _f64, _i32, _vp, _vp),
        ("seqik_head_angles_ex", _int, _dp, _dp, _i64, _i32, _dp, _i64, _f64, _f64, _i32, _dp, _dp, _opt),
        ("seqik_head_angles_ex_device", _int, _vp, _vp, _i64, _i32, _vp, _i64, _f64, _f64, _i32, _vp, _vp, _vp),
        ("seqik_signed_angles", _int, _dp, _i64, _dp, _i64, _dp, _i64, _dp, _opt),
        ("seqik_peer_alloc", _int, _vpp, _size),
        ("seqik_peer_free", _int, _vp),
        ("seqik_peer_export", _int, _vp, _cp),
        ("seqik_peer_open", _int, _cp, _vpp),
        ("seqik_peer_close", _int, _vp),
        ("seqik_peer_copy", _int, _vp, _vp, _size, _vp),
        ("seqik_host_alloc", _vp, _size),
        ("seqik_host_free", None, _vp),
        ("seqik_host_register", _int, _vp, _size),
        ("seqik_host_unregister", _int, _vp),
        ("seqik_stream_open", _int, _vpp, _i32, _legs, _aff, _i64, _i64, _lay, _i32, _i32, _i32, _i32, _opt),
        ("seqik_stream_submit", _int, _vp, _vp, _i64, _vp, _vp),
        ("seqik_stream_wait", _int, _vp),
        ("seqik_stream_reset_carry", _int, _vp),
        ("seqik_stream_set_carry", _int, _vp, _vp, _i64, _i32),
        ("seqik_stream_close", _int, _vp),
        ("seqik_align_stats_open", _int, _vpp, _i32, _i64, _opt),
        ("seqik_align_stats_add", _int, _vp, _vp, _i32, _i64, _i64, _lay, _vp),
        ("seqik_align_stats_finish", _int, _vp, _i64p, _i32, _dp, _vp),
        ("seqik_align_stats_reset", _int, _vp),
        ("seqik_align_stats_close", _int, _vp)),
    "seqik_fk.h": (
        ("seqik_forward_kinematics", _int, _dp, _i64, _i32, _i64, _legs, _i32, _dp, _dp, _dp, _dp, _i32),
        ("seqik_forward_kinematics_device", _int, _vp, _i64, _i32, _i64, _legs, _i32, _vp, _vp, _vp, _vp, _vp)),
    "seqik_frames.h": (
        ("seqik_link_frames", _int, _dp, _i64, _i32, _i64, _legs, _i32, _dp, _dp, _i32),
        ("seqik_link_frames_device", _int, _vp, _i64, _i32, _i64, _legs, _i32, _vp, _vp, _vp)),
    "seqik_gaps.h": (
        ("seqik_gaps_compact_device", _int, _vp, _i64, _i32, _i64, _i32, _legs, _vp, _vp, _vp, _vp),
        ("seqik_gaps_expand_device", _int, _vp, _i64, _i32, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp),
        ("seqik_solve_seq_gaps", _int, _dp, _i64, _i32, _i64, _legs, _i32, _i32, _dp, _dp, _ip, _ip, _dp, _aff, _opt, _ip),
        ("seqik_solve_generic_gaps", _int, _dp, _i64, _i32, _i64, _legs, _dp, _dp, _ip, _ip, _dp, _aff, _opt, _ip)),
    "seqik_resample.h": (
        ("seqik_resample_count", _i64, _i64, _f64, _f64),
        ("seqik_resample_workspace_bytes", _size, _i64, _i64, _i32),
        ("seqik_resample_pchip", _int, _dp, _i64, _i64, _i32, _f64, _f64, _i32, _i32, _dp, _i64, _i32),
        ("seqik_resample_pchip_device", _int, _vp, _i64, _i64, _i32, _f64, _f64, _i32, _i32, _vp, _i64, _vp, _vp)),
    "seqik_head_align.h": (
        ("seqik_head_align_stats_open", _int, _vpp, _i64, _opt),
        ("seqik_head_align_stats_select", _int, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _f64, _i64p, _i64p),
        ("seqik_head_align_stats_pick", _int, _vp, _i64p, _i64p, _i32, _dp),
        ("seqik_head_align_stats_close", _int, _vp),
        ("seqik_head_angles_raw", _int, _dp, _dp, _i64, _i32, _dp, _i64, _f64, _f64, _i32, _dp, _haff, _dp, _dp, _dp, _opt),
        ("seqik_head_angles_raw_device", _int, _vp, _vp, _i64, _i32, _vp, _i64, _f64, _f64, _i32, _vp, _haff, _vp, _vp, _vp, _vp)),
}

# Entry points added behind ABI 7 without a change of it, in headers of their own: the same row shape, bound by ``load()``
# in the same loop (``SIGNATURES`` stays the set of headers ABI 7 was cut with).
EXTENSION_SIGNATURES = {
    "seqik_resample_der.h": (
        ("seqik_resample_der", _int, _dp, _i64, _i64, _i32, _f64, _f64, _i32, _i32, _dp, _dp, _dp, _i64, _i32),
        ("seqik_resample_der_device", _int, _vp, _i64, _i64, _i32, _f64, _f64, _i32, _i32, _vp, _vp, _vp, _i64, _vp, _vp)),
}

# The same for skip mode on streams (include/seqik_stream_gaps.h): a third table, so that the two above stay the sets
# their tests pin.
STREAM_GAPS_SIGNATURES = {
    "seqik_stream_gaps.h": (
        ("seqik_stream_open_skip", _int, _vpp, _i32, _legs, _aff, _i64, _i64, _lay, _i32, _i32, _i32, _i32, _opt),
        ("seqik_stream_seed_state", _int, _legs, _i32, _i32, _dp),
        ("seqik_stream_get_carry", _int, _vp, _dp, _i64)),
}

# The same for the leg Jacobians (include/seqik_jacobian.h): a fourth table.
JACOBIAN_SIGNATURES = {
    "seqik_jacobian.h": (
        ("seqik_leg_jacobians", _int, _dp, _i64, _i32, _i64, _legs, _i32, _dp, _dp, _dp, _dp, _i32),
        ("seqik_leg_jacobians_device", _int, _vp, _i64, _i32, _i64, _legs, _i32, _vp, _vp, _vp, _vp, _vp)),
}

# The same for the key-point sensitivity of the sequential fit (include/seqik_sensitivity.h): a fifth table.
SENSITIVITY_SIGNATURES = {
    "seqik_sensitivity.h": (
        ("seqik_fit_sensitivity", _int, _dp, _dp, _i64, _i32, _i64, _legs, _i32, _dp, _f64, _dp, _dp, _ip, _i32),
        ("seqik_fit_sensitivity_device", _int, _vp, _vp, _i64, _i32, _i64, _legs, _i32, _vp, _f64, _vp, _vp, _vp, _vp)),
}

# The same for the whole-leg refinement (include/seqik_refine.h): a sixth table.
REFINE_SIGNATURES = {
    "seqik_refine.h": (
        ("seqik_refine_legs", _int, _dp, _dp, _i64, _i32, _i64, _legs, _i32, _dp, _ropt, _dp, _dp, _ip, _i32),
        ("seqik_refine_legs_device", _int, _vp, _vp, _i64, _i32, _i64, _legs, _i32, _vp, _ropt, _vp, _vp, _vp, _vp)),
}

# The same for the trajectory refinement (include/seqik_smooth.h): a seventh table.
_sopt = ctypes.POINTER(SeqikSmoothOptions)
SMOOTH_SIGNATURES = {
    "seqik_smooth.h": (
        ("seqik_smooth_workspace_bytes", _i64, _i64, _i32, _i64),
        ("seqik_smooth_legs", _int, _dp, _dp, _i64, _i32, _i64, _legs, _i32, _dp, _sopt, _dp, _ip, _dp, _ip, _i32),
        ("seqik_smooth_legs_device", _int, _vp, _vp, _i64, _i32, _i64, _legs, _i32, _vp, _sopt, _vp, _vp, _vp, _vp, _vp,
         _i64, _vp)),
}

# The same for the error bars of the whole-leg refinement (include/seqik_refine_sensitivity.h): an eighth table.
REFINE_SENS_SIGNATURES = {
    "seqik_refine_sensitivity.h": (
        ("seqik_refine_sensitivity", _int, _dp, _dp, _i64, _i32, _i64, _legs, _i32, _dp, _dp, _f64, _dp, _dp, _dp, _ip, _i32),
        ("seqik_refine_sensitivity_device", _int, _vp, _vp, _i64, _i32, _i64, _legs, _i32, _vp, _vp, _f64, _vp, _vp, _vp, _vp,
         _vp)),
}

# The same for the error bars of the smoothed trajectory (include/seqik_smooth_sensitivity.h): a ninth table.
SMOOTH_SENS_SIGNATURES = {
    "seqik_smooth_sensitivity.h": (
        ("seqik_smooth_sensitivity_workspace_bytes", _i64, _i64, _i32, _i64, _i32),
        ("seqik_smooth_sensitivity", _int, _dp, _dp, _i64, _i32, _i64, _legs, _i32, _dp, _dp, _dp, _f64, _i32, _dp, _dp, _dp,
         _ip, _i32),
        ("seqik_smooth_sensitivity_device", _int, _vp, _vp, _i64, _i32, _i64, _legs, _i32, _vp, _vp, _dp, _f64, _i32, _vp,
         _vp, _vp, _vp, _vp, _i64, _vp)),
}


class SeqikLibraryError(RuntimeError):
    pass


_lock = threading.Lock()
_lib = None


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


KERNEL_SOURCES = ["seqik_core.hpp", "seqik_consts.hpp", "seqik_hip.hip"]   # what the solver kernels are compiled from
LATENCY_SOURCES = KERNEL_SOURCES + ["seqik_generic.hpp"]   # ... and the generic-chain kernel (profiles/r04_latency_floor.json)


def _code_only(text: str) -> str:
    """C++ source without comments and with white space collapsed (what the compiler sees, roughly)."""
    import re
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return " ".join(text.split())


def csrc_sha256(files=None, read=None) -> str:
    """sha256 over the CODE of the solver kernels' sources (``KERNEL_SOURCES`` order; comments and white space do not
    count): ties a committed PMC summary (profiles/traffic_rNN.json, written by scripts/summarize_profile.py) to the build
    it was measured on.  ``read(name) -> str``: another source of the files (e.g. an older commit)."""
    import hashlib
    h = hashlib.sha256()
    for name in (files or KERNEL_SOURCES):
        if read is not None:
            text = read(name)
        else:
            with open(os.path.join(CSRC, name), "r") as f:
                text = f.read()
        h.update(_code_only(text).encode())
    return h.hexdigest()


def _older_than_sources(path) -> bool:
    return (not os.path.exists(path) or
            any(os.path.getmtime(os.path.join(CSRC, s)) > os.path.getmtime(path) for s in SOURCES))


def is_stale() -> bool:
    # installed package: the library was compiled when the distribution was built
    return _IN_TREE and _older_than_sources(LIB_PATH)


def _compile(out_path, extra_flags, needed) -> str:
    """``COMPILE_UNITS`` -> ``out_path`` with ``HIPCC_FLAGS`` + ``extra_flags`` (gfx950), when ``needed``."""
    if needed:
        cmd = [_hipcc()] + HIPCC_FLAGS + extra_flags + ["-o", out_path] + [os.path.join(CSRC, u) for u in COMPILE_UNITS]
        subprocess.check_call(cmd, cwd=CSRC)
    return out_path


def build(force: bool = False) -> str:
    """Compiles ``csrc/seqik_hip.hip`` -> ``csrc/libseqik_hip.so`` (gfx950)."""
    return _compile(LIB_PATH, [], force or is_stale())


WATCHDOG_LIB_PATH = os.path.join(CSRC, "libseqik_hip_watchdog.so")


def build_watchdog_variant(force: bool = False) -> str:
    """DIAGNOSTIC build for tests/test_gpu_parity.py::test_pipeline_watchdog_is_reported: the same sources with the stage
    pipeline's watchdog limit set to ONE pass (``-DSEQIK_PIPE_SPIN_LIMIT=1``), so that the fault path -- NaN in the
    chain, fault word, ``SEQIK_ERR_HIP`` from the entry points -- can be exercised.  Never loaded by the package itself
    (only through ``SEQIK_LIB`` in a child process of that test)."""
    return _compile(WATCHDOG_LIB_PATH, ["-DSEQIK_PIPE_SPIN_LIMIT=1"], force or _older_than_sources(WATCHDOG_LIB_PATH))


def load():
    """Loads the HIP library; raises ``SeqikLibraryError`` if it has not been built."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise SeqikLibraryError(
                f"{LIB_PATH} not found: the HIP extension is not built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'`). "
                "seqikpy_amd has no CPU fallback.")
        # PyTorch-ROCm wheels bundle their own libamdhip64.so.7.  Two HIP runtimes in one
        # process cannot both own the GPU, so when torch is installed let it load first: the
        # dynamic linker then binds this library to the already-loaded runtime (same SONAME)
        # and torch tensors / streams / RCCL can be shared with it.
        if os.environ.get("SEQIK_NO_TORCH_PRELOAD", "0") != "1":
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        L = ctypes.CDLL(LIB_PATH)
        if L.seqik_abi_version() != ABI_VERSION:
            raise SeqikLibraryError(f"{LIB_PATH} has ABI {L.seqik_abi_version()}, this package needs {ABI_VERSION}: "
                                    "rebuild it (`python -c 'import __graft_entry__ as g; g.build()'`)")
        for signatures in (list(SIGNATURES.values()) + list(EXTENSION_SIGNATURES.values()) +
                           list(STREAM_GAPS_SIGNATURES.values()) + list(JACOBIAN_SIGNATURES.values()) +
                           list(SENSITIVITY_SIGNATURES.values()) + list(REFINE_SIGNATURES.values()) +
                           list(SMOOTH_SIGNATURES.values()) + list(REFINE_SENS_SIGNATURES.values()) +
                           list(SMOOTH_SENS_SIGNATURES.values())):
            for name, restype, *argtypes in signatures:
                fn = getattr(L, name)
                fn.restype, fn.argtypes = restype, argtypes
        _lib = L
        return _lib


def _raise(rc: int):
    msg = load().seqik_last_error().decode("utf-8", "replace")
    if rc in (ERR_X0, ERR_BOUNDS, ERR_STAGE):
        raise ValueError(msg)
    if rc == ERR_ARG:
        raise ValueError(f"seqik: bad argument: {msg}")
    raise SeqikLibraryError(f"seqik: HIP error: {msg}")


def _call(name, *args):
    """Calls the status-returning entry point ``name``; anything but ``SEQIK_OK`` raises (``_raise``)."""
    rc = getattr(_lib or load(), name)(*args)
    if rc != SEQIK_OK:
        _raise(rc)


def _data(a, pointer_type=_dp):
    """``a.ctypes.data_as(pointer_type)`` of a numpy array; None = NULL."""
    return a.ctypes.data_as(pointer_type) if a is not None else None


def _ptr(x, name="buffer", shape=None, dtype="float64"):
    """A raw device pointer (int) or a tensor's ``data_ptr()``; 0 / None = NULL.  A tensor is checked against what the
    kernel will read or write through the pointer: a contiguous GPU tensor of ``dtype`` with ``shape``'s element count
    (``shape=None``: the layout is not dense, the count is not checked)."""
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        if str(x.dtype) != f"torch.{dtype}":
            raise ValueError(f"{name}: expected a {dtype} tensor, got {x.dtype}")
        if shape is not None and x.numel() != int(np.prod(shape)):
            raise ValueError(f"{name}: expected {int(np.prod(shape))} elements {tuple(shape)}, got {x.numel()} "
                             f"{tuple(x.shape)}")
        if not x.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous tensor")
        if not x.is_cuda:
            raise ValueError(f"{name}: expected a GPU tensor, got one on {x.device}")
        return ctypes.c_void_p(x.data_ptr() or None)
    return ctypes.c_void_p(int(x) or None)


def _stream_ptr(stream):
    """A hipStream_t as int or a torch stream; 0 / None = the default stream."""
    if stream is None:
        return None
    s = stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)
    return ctypes.c_void_p(s or None)


EXPORTED_SYMBOLS = [sig[0] for sig in SIGNATURES["seqik.h"]]

#: entry points of include/seqik_fk.h (forward kinematics from joint angles), kept apart from the ABI-7 set of seqik.h
FK_EXPORTED_SYMBOLS = [sig[0] for sig in SIGNATURES["seqik_fk.h"]]
FK_KINDS = {"seq": 0, "generic": 1}


def _fk_kind(kind) -> int:
    if isinstance(kind, str):
        if kind not in FK_KINDS:
            raise ValueError(f"kind must be one of {sorted(FK_KINDS)}, got {kind!r}")
        return FK_KINDS[kind]
    return int(kind)


def _angles_batch(angles, legs, kind):
    """The checks the host wrappers of the angle maps share -> (angles, (S, L, N), kind as int, the leading arguments)."""
    angles = np.ascontiguousarray(angles, dtype=np.float64)
    if angles.ndim != 4 or angles.shape[3] != 7:
        raise ValueError(f"angles must have shape (S, L, N, 7), got {angles.shape}")
    if len(legs) != angles.shape[1]:
        raise ValueError("one SeqikLegParams per leg expected")
    k = _fk_kind(kind)
    return angles, angles.shape[:3], k, (_data(angles), *angles.shape[:3], (SeqikLegParams * len(legs))(*legs), k)


def _angle_map_head(d_angles, n_seq, n_legs, n_frames, legs, kind):
    """The leading arguments of the angle maps' ``*_device`` wrappers -> ((S, L, N), (angles, S, L, N, legs, kind))."""
    lf = (n_seq, n_legs, n_frames)
    return lf, (_ptr(d_angles, "angles", lf + (7,)), *map(int, lf), (SeqikLegParams * n_legs)(*legs), _fk_kind(kind))


def _origin_batch(origin, slf):
    """``origin`` broadcast to a contiguous (S, L, N, 3) array; None stays None."""
    if origin is None:
        return None
    return np.ascontiguousarray(np.broadcast_to(np.asarray(origin, dtype=np.float64), tuple(slf) + (3,)))


def forward_kinematics(angles, legs, kind="seq", pose=None, origin=None, want_dist=False, device=-1):
    """``seqik_forward_kinematics`` on host arrays: joint angles (S, L, N, 7) in ``DOFS`` order -> dict(fk (S, L, N, 9, 3),
    dist (S, L, N, 4) or None), the rows the solvers write (``solve_seq`` / ``solve_generic``).

    ``kind``: ``"seq"`` (KinematicChainSeq) or ``"generic"`` (KinematicChainGeneric) -- the chain that produced the angles.
    The origin of each leg-frame is key point 0 of ``pose`` (S, L, N, 5, 3), or ``origin`` (anything that broadcasts to
    (S, L, N, 3); the fused alignment's origin is ``template_coxa``), or 0 when neither is given (leg-local positions).
    ``want_dist`` (needs ``pose``): distances of FK rows 4, 6, 7, 8 from key points 1..4.  An angle that is not finite or lies beyond
    ``SEQIK_ANGLE_MAX`` (2^30 rad, include/seqik_fk.h) makes that leg-frame's rows (and distances) NaN.  Fed a solver's angles and origin, the result equals the solver's FK bit for bit."""
    angles, (S, L, N), k, head = _angles_batch(angles, legs, kind)
    if pose is not None and origin is not None:
        raise ValueError("pass pose or origin, not both")
    if want_dist and pose is None:
        raise ValueError("want_dist needs pose (the key points to measure against)")
    if pose is not None:
        pose = np.ascontiguousarray(pose, dtype=np.float64)
        if pose.shape != (S, L, N, 5, 3):
            raise ValueError(f"pose must have shape {(S, L, N, 5, 3)}, got {pose.shape}")
    origin = _origin_batch(origin, (S, L, N))
    fk = np.full((S, L, N, 9, 3), np.nan)
    dist = np.full((S, L, N, 4), np.nan) if want_dist else None
    _call("seqik_forward_kinematics", *head, _data(pose), _data(origin), _data(fk), _data(dist), int(device))
    return dict(fk=fk, dist=dist)


def forward_kinematics_device(d_angles, n_seq, n_legs, n_frames, legs, d_fk, kind="seq", d_pose=0, d_origin=0, d_dist=0,
                              stream=0):
    """``seqik_forward_kinematics_device``: raw device pointers (ints) or torch tensors in the dense layouts of
    ``forward_kinematics``, asynchronous on ``stream`` (a hipStream_t as int, or a torch stream; 0 = the default stream)
    of the current device."""
    lf, head = _angle_map_head(d_angles, n_seq, n_legs, n_frames, legs, kind)
    _call("seqik_forward_kinematics_device", *head, _ptr(d_pose, "pose", lf + (5, 3)), _ptr(d_origin, "origin", lf + (3,)),
          _ptr(d_fk, "fk", lf + (9, 3)), _ptr(d_dist, "dist", lf + (4,)), _stream_ptr(stream))


#: entry points of include/seqik_frames.h (link frames from joint angles), kept apart from the ABI-7 set of seqik.h
FRAMES_EXPORTED_SYMBOLS = [sig[0] for sig in SIGNATURES["seqik_frames.h"]]


def link_frames(angles, legs, kind="seq", origin=None, device=-1, rows3=False):
    """``seqik_link_frames`` on host arrays: joint angles (S, L, N, 7) in ``DOFS`` order -> dict(frames (S, L, N, 9, 4, 4)),
    the 4 x 4 frame of each of the nine links of the whole-leg chain in the chain's base frame -- what IKPy's
    ``Chain.forward_kinematics(q, full_kinematics=True)`` returns, for every leg-frame of the batch.

    ``kind``: ``"seq"`` (links base, ThC_yaw, ThC_pitch, ThC_roll, CTr_pitch, CTr_roll, FTi_pitch, TiTa_pitch, Claw) or
    ``"generic"`` (base, ThC_roll, ThC_yaw, ThC_pitch, ...).  ``origin``: anything that broadcasts to (S, L, N, 3), added to
    the translation column only; absent = leg-local frames.  The translation columns equal ``forward_kinematics``' rows
    for the same angles, kind and origin bit for bit.  ``rows3=True`` returns the (S, L, N, 9, 3, 4) array as the library
    wrote it (the fourth row, 0 0 0 1, is filled in on the host otherwise).  An angle that is not finite or lies beyond
    ``SEQIK_ANGLE_MAX`` (2^30 rad) makes that leg-frame's frames NaN (with ``rows3=False`` the fourth row too)."""
    angles, (S, L, N), k, head = _angles_batch(angles, legs, kind)
    origin = _origin_batch(origin, (S, L, N))
    rows = np.full((S, L, N, 9, 3, 4), np.nan)
    _call("seqik_link_frames", *head, _data(origin), _data(rows), int(device))
    if rows3:
        return dict(frames=rows)
    frames = np.empty((S, L, N, 9, 4, 4))
    frames[..., :3, :] = rows
    frames[..., 3, :] = (0.0, 0.0, 0.0, 1.0)
    frames[..., 3, :][np.isnan(rows[..., 0, 0])] = np.nan
    return dict(frames=frames)


def link_frames_device(d_angles, n_seq, n_legs, n_frames, legs, d_frames, kind="seq", d_origin=0, stream=None):
    """``seqik_link_frames_device``: raw device pointers (ints) or torch tensors in the dense layouts of
    ``include/seqik_frames.h`` (``d_frames``: (S, L, N, 9, 3, 4) doubles), asynchronous on ``stream`` (a hipStream_t as
    int, or a torch stream; None / 0 = the default stream) of the current device."""
    lf, head = _angle_map_head(d_angles, n_seq, n_legs, n_frames, legs, kind)
    _call("seqik_link_frames_device", *head, _ptr(d_origin, "origin", lf + (3,)), _ptr(d_frames, "frames", lf + (9, 3, 4)),
          _stream_ptr(stream))


#: entry points of include/seqik_jacobian.h (leg Jacobians, conditioning, key-point velocities), additive to ABI 7
JACOBIAN_EXPORTED_SYMBOLS = [sig[0] for sig in JACOBIAN_SIGNATURES["seqik_jacobian.h"]]


def _sigma_view(sigma, kind):
    """The library's (..., 8) conditioning record as documented: (..., 4, 2) for the sequential chain, (..., 3) for the
    generic chain (its other five values are NaN and carry no meaning)."""
    if sigma is None:
        return None
    return sigma.reshape(sigma.shape[:-1] + (4, 2)) if kind == 0 else np.ascontiguousarray(sigma[..., :3])


def leg_jacobians(angles, legs, kind="seq", qdot=None, want_jac=True, want_sigma=True, device=-1):
    """``seqik_leg_jacobians`` on host arrays: joint angles (S, L, N, 7) in ``DOFS`` order -> dict(jac (S, L, N, 4, 3, 7) or
    None, sigma or None, vel (S, L, N, 4, 3) or None).

    ``jac[..., k, :, d]`` is the derivative of key point k + 1 (FK rows 4, 6, 7, 8: coxa, femur and tibia end, claw) with
    respect to the angle of DOF d -- ``DOFS`` order for both kinds -- in the leg's own frame (it does not depend on the
    origin).  ``sigma`` (``want_sigma``): for ``kind="seq"`` (S, L, N, 4, 2), per stage (sigma_max, sigma_min) of the
    block that stage's solve sees (key point s by the stage's own DOFs); for ``"generic"`` (S, L, N, 3), the singular
    values of the claw's 3 x 7 block, descending.  ``vel`` (when ``qdot`` (S, L, N, 7), joint rates, is given): ``jac @
    qdot``, the key-point velocities.  At least one of the three must be asked for.  An angle that is not finite or lies
    beyond ``SEQIK_ANGLE_MAX`` makes that leg-frame's values NaN; a non-finite rate its velocities only."""
    angles, (S, L, N), k, head = _angles_batch(angles, legs, kind)
    if qdot is not None:
        qdot = np.ascontiguousarray(qdot, dtype=np.float64)
        if qdot.shape != angles.shape:
            raise ValueError(f"qdot must have the shape of angles {angles.shape}, got {qdot.shape}")
    jac = np.full((S, L, N, 4, 3, 7), np.nan) if want_jac else None
    sigma = np.full((S, L, N, 8), np.nan) if want_sigma else None
    vel = np.full((S, L, N, 4, 3), np.nan) if qdot is not None else None
    _call("seqik_leg_jacobians", *head, _data(qdot), _data(jac), _data(sigma), _data(vel), int(device))
    return dict(jac=jac, sigma=_sigma_view(sigma, k), vel=vel)


def leg_jacobians_device(d_angles, n_seq, n_legs, n_frames, legs, kind="seq", d_qdot=0, d_jac=0, d_sigma=0, d_vel=0,
                         stream=None):
    """``seqik_leg_jacobians_device``: raw device pointers (ints) or torch tensors in the dense layouts of
    ``include/seqik_jacobian.h`` (``d_jac`` (S, L, N, 4, 3, 7), ``d_sigma`` (S, L, N, 8), ``d_vel`` (S, L, N, 4, 3)
    doubles; 0 / None: not computed, not written; at least one), asynchronous on ``stream`` (a hipStream_t as int, or a
    torch stream; None / 0 = the default stream) of the current device."""
    lf, head = _angle_map_head(d_angles, n_seq, n_legs, n_frames, legs, kind)
    _call("seqik_leg_jacobians_device", *head, _ptr(d_qdot, "qdot", lf + (7,)), _ptr(d_jac, "jac", lf + (4, 3, 7)),
          _ptr(d_sigma, "sigma", lf + (8,)), _ptr(d_vel, "vel", lf + (4, 3)), _stream_ptr(stream))


#: entry points of include/seqik_sensitivity.h (key-point sensitivity of the sequential fit), additive to ABI 7
SENSITIVITY_EXPORTED_SYMBOLS = [sig[0] for sig in SENSITIVITY_SIGNATURES["seqik_sensitivity.h"]]
SENS_BOUND_TOL = 1e-6        # SEQIK_SENS_BOUND_TOL
SENS_FLAG_BAD_INPUT = 1 << 16


def sens_flag_held(dof: int) -> int:
    """The flag bit of ``fit_sensitivity`` that says DOF ``dof`` (``DOFS`` order) sits on a limit and is held there."""
    return 1 << dof


def sens_flag_not_pd(stage: int) -> int:
    """The flag bit of ``fit_sensitivity`` that says stage ``stage`` (1..4) is not at a strict minimum."""
    return 1 << (7 + stage)


def _sigma_batch(kp_sigma, slf):
    """``kp_sigma`` (a scalar, (4,) or anything else that broadcasts) as a contiguous (S, L, N, 4) array; None stays None."""
    if kp_sigma is None:
        return None
    return np.ascontiguousarray(np.broadcast_to(np.asarray(kp_sigma, dtype=np.float64), tuple(slf) + (4,)))


def fit_sensitivity(angles, pose, legs, kp_sigma=None, want_sens=True, want_flags=True, bound_tol=SENS_BOUND_TOL,
                    device=-1):
    """``seqik_fit_sensitivity`` on host arrays: the solved angles (S, L, N, 7) of the sequential chain and the aligned key
    points (S, L, N, 5, 3) they were fitted to -> dict(sens (S, L, N, 7, 4, 3) or None, std (S, L, N, 7) or None, flags
    (S, L, N) int32 or None).

    ``sens[..., d, k, c]`` is the derivative of the fitted angle of ``DOFS[d]`` with respect to component c of aligned key
    point k + 1: the response of the four sequential solves with their exact Hessians (not the pseudo-inverse of the
    Jacobian), 0 for a joint that sits on a limit of ``legs[l].bounds`` (within ``bound_tol`` rad; <= 0: never) and is
    pushed against it.  ``std`` (when ``kp_sigma`` -- a scalar, (4,), or anything that broadcasts to (S, L, N, 4):
    the isotropic standard deviation of key points 1..4 -- is given): the standard deviation that noise gives every angle.
    ``flags``: bits 0..6 DOF held (``sens_flag_held``), bits 8..11 stage not at a strict minimum (its rows are NaN;
    ``sens_flag_not_pd``), bit 16 non-finite input (the leg-frame's values are NaN).  At least one of the three must be
    asked for.  ``legs`` carry the segment lengths and the bounds."""
    angles, (S, L, N), _, head = _angles_batch(angles, legs, 0)
    pose = np.ascontiguousarray(pose, dtype=np.float64)
    if pose.shape != (S, L, N, 5, 3):
        raise ValueError(f"pose must have shape {(S, L, N, 5, 3)}, got {pose.shape}")
    try:
        sigma = _sigma_batch(kp_sigma, (S, L, N))
    except ValueError:
        raise ValueError(f"kp_sigma must broadcast to {(S, L, N, 4)}, got {np.shape(kp_sigma)}") from None
    sens = np.full((S, L, N, 7, 4, 3), np.nan) if want_sens else None
    std = np.full((S, L, N, 7), np.nan) if sigma is not None else None
    flags = np.zeros((S, L, N), dtype=np.int32) if want_flags else None
    _call("seqik_fit_sensitivity", head[0], _data(pose), *head[1:], _data(sigma), float(bound_tol), _data(sens), _data(std),
          _data(flags, _ip), int(device))
    return dict(sens=sens, std=std, flags=flags)


def fit_sensitivity_device(d_angles, d_pose, n_seq, n_legs, n_frames, legs, d_kp_sigma=0, d_sens=0, d_std=0, d_flags=0,
                           bound_tol=SENS_BOUND_TOL, stream=None):
    """``seqik_fit_sensitivity_device``: raw device pointers (ints) or torch tensors in the dense layouts of
    ``include/seqik_sensitivity.h`` (``d_pose`` (S, L, N, 5, 3), ``d_kp_sigma`` (S, L, N, 4), ``d_sens`` (S, L, N, 7, 4, 3),
    ``d_std`` (S, L, N, 7) doubles, ``d_flags`` (S, L, N) int32; 0 / None: not computed, not written; at least one
    output), asynchronous on ``stream`` (a hipStream_t as int, or a torch stream; None / 0 = the default stream) of the
    current device."""
    lf, head = _angle_map_head(d_angles, n_seq, n_legs, n_frames, legs, 0)
    _call("seqik_fit_sensitivity_device", head[0], _ptr(d_pose, "pose", lf + (5, 3)), *head[1:],
          _ptr(d_kp_sigma, "kp_sigma", lf + (4,)), float(bound_tol), _ptr(d_sens, "sens", lf + (7, 4, 3)),
          _ptr(d_std, "std", lf + (7,)), _ptr(d_flags, "flags", lf, dtype="int32"), _stream_ptr(stream))


#: entry points of include/seqik_refine.h (whole-leg refinement of the sequential fit), additive to ABI 7
REFINE_EXPORTED_SYMBOLS = [sig[0] for sig in REFINE_SIGNATURES["seqik_refine.h"]]
REFINE_MAX_ITER, REFINE_GTOL, REFINE_FTOL = 200, 1e-10, 1e-14   # SEQIK_REFINE_MAX_ITER / _GTOL / _FTOL
REFINE_STOP_GRADIENT, REFINE_STOP_DECREASE, REFINE_STOP_DAMPING, REFINE_STOP_MAX_ITER = 0, 1, 2, 4
REFINE_BAD_INPUT = 1 << 24


def refine_stop_reason(info):
    """Why the lanes of ``refine_legs`` stopped (``REFINE_STOP_*``), from ``info``."""
    return (np.asarray(info) >> 8) & 7


def refine_iterations(info):
    """The accepted iterations of the lanes of ``refine_legs``, from ``info``."""
    return (np.asarray(info) >> 16) & 255


def _refine_options(max_iter, gtol, ftol):
    return ctypes.byref(SeqikRefineOptions(int(max_iter), float(gtol), float(ftol)))


def refine_legs(angles, pose, legs, kp_weight=None, max_iter=REFINE_MAX_ITER, gtol=REFINE_GTOL, ftol=REFINE_FTOL,
                want_cost=True, want_info=True, device=None):
    """``seqik_refine_legs`` on host arrays: angles (S, L, N, 7) of the sequential chain -- normally the sequential fit's
    -- and the aligned key points (S, L, N, 5, 3) -> dict(angles (S, L, N, 7), cost (S, L, N, 2) or None, info (S, L, N)
    int32 or None).

    Every leg-frame is refined on its own: from its start, clamped into ``legs[l].bounds``, a bounded Levenberg-Marquardt
    minimises the weighted squared distance of the chain's four key points from key points 1..4 over all seven angles at
    once.  ``kp_weight``: a scalar, (4,) or anything that broadcasts to (S, L, N, 4) (None: 1); a key point with weight
    exactly 0 is not read and may be NaN.  ``cost[..., 0]`` is the weighted sum of squares at the clamped start,
    ``cost[..., 1]`` at the result (never larger).  ``info``: bits 0..6 DOF held on a limit, ``refine_stop_reason``,
    ``refine_iterations``, bit 24 (``REFINE_BAD_INPUT``) non-finite input: that leg-frame's angles and costs are NaN.
    ``max_iter`` (1..255), ``gtol``, ``ftol``: include/seqik_refine.h.  ``device=None``: the current device."""
    angles, (S, L, N), _, head = _angles_batch(angles, legs, 0)
    pose = np.ascontiguousarray(pose, dtype=np.float64)
    if pose.shape != (S, L, N, 5, 3):
        raise ValueError(f"pose must have shape {(S, L, N, 5, 3)}, got {pose.shape}")
    try:
        weight = _sigma_batch(kp_weight, (S, L, N))
    except ValueError:
        raise ValueError(f"kp_weight must broadcast to {(S, L, N, 4)}, got {np.shape(kp_weight)}") from None
    out = np.full((S, L, N, 7), np.nan)
    cost = np.full((S, L, N, 2), np.nan) if want_cost else None
    info = np.zeros((S, L, N), dtype=np.int32) if want_info else None
    _call("seqik_refine_legs", head[0], _data(pose), *head[1:], _data(weight), _refine_options(max_iter, gtol, ftol),
          _data(out), _data(cost), _data(info, _ip), -1 if device is None else int(device))
    return dict(angles=out, cost=cost, info=info)


def refine_legs_device(d_angles, d_pose, n_seq, n_legs, n_frames, legs, d_angles_out, d_kp_weight=0, d_cost=0, d_info=0,
                       max_iter=REFINE_MAX_ITER, gtol=REFINE_GTOL, ftol=REFINE_FTOL, stream=None):
    """``seqik_refine_legs_device``: raw device pointers (ints) or torch tensors in the dense layouts of
    ``include/seqik_refine.h`` (``d_pose`` (S, L, N, 5, 3), ``d_kp_weight`` (S, L, N, 4), ``d_angles_out`` (S, L, N, 7) --
    it may be ``d_angles`` --, ``d_cost`` (S, L, N, 2) doubles, ``d_info`` (S, L, N) int32; 0 / None: all weights 1, not
    written), asynchronous on ``stream`` (a hipStream_t as int, or a torch stream; None / 0 = the default stream) of the
    current device."""
    lf, head = _angle_map_head(d_angles, n_seq, n_legs, n_frames, legs, 0)
    _call("seqik_refine_legs_device", head[0], _ptr(d_pose, "pose", lf + (5, 3)), *head[1:],
          _ptr(d_kp_weight, "kp_weight", lf + (4,)), _refine_options(max_iter, gtol, ftol),
          _ptr(d_angles_out, "angles_out", lf + (7,)), _ptr(d_cost, "cost", lf + (2,)),
          _ptr(d_info, "info", lf, dtype="int32"), _stream_ptr(stream))


#: entry points of include/seqik_refine_sensitivity.h (error bars of the whole-leg refinement), additive to ABI 7
REFINE_SENS_EXPORTED_SYMBOLS = [sig[0] for sig in REFINE_SENS_SIGNATURES["seqik_refine_sensitivity.h"]]
REFINE_SENS_FLAG_NOT_PD = 1 << 8
REFINE_SENS_FLAG_BAD_INPUT = 1 << 16


def refine_sensitivity(angles, pose, legs, kp_weight=None, kp_sigma=None, bound_tol=SENS_BOUND_TOL, want_sens=True,
                       want_std=None, want_grad=True, want_flags=True, device=None):
    """``seqik_refine_sensitivity`` on host arrays: angles (S, L, N, 7) that minimise the whole-leg fit -- the output of
    ``refine_legs`` -- and the aligned key points (S, L, N, 5, 3) they were fitted to -> dict(sens (S, L, N, 7, 4, 3),
    std (S, L, N, 7), grad (S, L, N), flags (S, L, N) int32; None for what is not asked for).

    ``sens[..., d, k, c]`` is the derivative of the refined angle of ``DOFS[d]`` with respect to component c of aligned
    key point k + 1: the inverse of the exact Hessian of the whole-leg fit on the free joints applied to the weighted
    Jacobian (not the pseudo-inverse of the Jacobian, and not ``fit_sensitivity``'s block-triangular response of the
    four sequential solves); 0 for a joint that sits on a limit of ``legs[l].bounds`` (within ``bound_tol`` rad; 0:
    never) and is pushed against it.  THE VALUES ARE THE FIT'S RESPONSE ONLY AT ANGLES THAT MINIMISE IT: ``grad`` -- the
    left side of the gradient test of ``refine_legs`` at these angles -- tells whether they do.  ``kp_weight``: the
    weights the fit was made with (as ``refine_legs``; a key point with weight exactly 0 is not read and its columns
    are 0).  ``std`` (``want_std``; default: whenever ``kp_sigma`` -- a scalar, (4,), or anything that broadcasts to (S,
    L, N, 4) -- is given): the standard deviation that key-point noise gives every angle.  ``flags``: bits 0..6 DOF held
    (``sens_flag_held``), bit 8 (``REFINE_SENS_FLAG_NOT_PD``) the angles are not a strict minimum (the rows of the free
    joints are NaN), bit 16 bad input (the leg-frame's values are NaN).  At least one of the four must be asked for.
    ``device=None``: the current device."""
    angles, (S, L, N), _, head = _angles_batch(angles, legs, 0)
    pose = np.ascontiguousarray(pose, dtype=np.float64)
    if pose.shape != (S, L, N, 5, 3):
        raise ValueError(f"pose must have shape {(S, L, N, 5, 3)}, got {pose.shape}")
    try:
        weight = _sigma_batch(kp_weight, (S, L, N))
    except ValueError:
        raise ValueError(f"kp_weight must broadcast to {(S, L, N, 4)}, got {np.shape(kp_weight)}") from None
    try:
        sigma = _sigma_batch(kp_sigma, (S, L, N))
    except ValueError:
        raise ValueError(f"kp_sigma must broadcast to {(S, L, N, 4)}, got {np.shape(kp_sigma)}") from None
    if want_std is None:
        want_std = sigma is not None
    if want_std and sigma is None:
        raise ValueError("std needs kp_sigma")
    sens = np.full((S, L, N, 7, 4, 3), np.nan) if want_sens else None
    std = np.full((S, L, N, 7), np.nan) if want_std else None
    grad = np.full((S, L, N), np.nan) if want_grad else None
    flags = np.zeros((S, L, N), dtype=np.int32) if want_flags else None
    _call("seqik_refine_sensitivity", head[0], _data(pose), *head[1:], _data(weight), _data(sigma if want_std else None),
          float(bound_tol), _data(sens), _data(std), _data(grad), _data(flags, _ip), -1 if device is None else int(device))
    return dict(sens=sens, std=std, grad=grad, flags=flags)


def refine_sensitivity_device(d_angles, d_pose, n_seq, n_legs, n_frames, legs, d_kp_weight=0, d_kp_sigma=0, d_sens=0,
                              d_std=0, d_grad=0, d_flags=0, bound_tol=SENS_BOUND_TOL, stream=None):
    """``seqik_refine_sensitivity_device``: raw device pointers (ints) or torch tensors in the dense layouts of
    ``include/seqik_refine_sensitivity.h`` (``d_pose`` (S, L, N, 5, 3), ``d_kp_weight`` and ``d_kp_sigma`` (S, L, N, 4),
    ``d_sens`` (S, L, N, 7, 4, 3), ``d_std`` (S, L, N, 7), ``d_grad`` (S, L, N) doubles, ``d_flags`` (S, L, N) int32; 0 /
    None: all weights 1, not computed, not written; at least one output), asynchronous on ``stream`` (a hipStream_t as
    int, or a torch stream; None / 0 = the default stream) of the current device.  ``d_angles`` may be the output buffer
    of ``refine_legs_device`` enqueued before it on the same stream."""
    lf, head = _angle_map_head(d_angles, n_seq, n_legs, n_frames, legs, 0)
    _call("seqik_refine_sensitivity_device", head[0], _ptr(d_pose, "pose", lf + (5, 3)), *head[1:],
          _ptr(d_kp_weight, "kp_weight", lf + (4,)), _ptr(d_kp_sigma, "kp_sigma", lf + (4,)), float(bound_tol),
          _ptr(d_sens, "sens", lf + (7, 4, 3)), _ptr(d_std, "std", lf + (7,)), _ptr(d_grad, "grad", lf),
          _ptr(d_flags, "flags", lf, dtype="int32"), _stream_ptr(stream))


#: entry points of include/seqik_gaps.h (skip mode for missing key points), kept apart from the ABI-7 set of seqik.h
GAPS_EXPORTED_SYMBOLS = [sig[0] for sig in SIGNATURES["seqik_gaps.h"]]
#: status of a missing leg-frame in skip mode (``SEQIK_STATUS_MISSING``; scipy's statuses are -1..4)
STATUS_MISSING = -100
GAPS_SEQ, GAPS_GENERIC, GAPS_AFFINE = 0, 1, 2
MISSING_MODES = ("raise", "skip")


def check_missing_mode(missing) -> bool:
    """True for ``"skip"``, False for ``"raise"``; anything else is a ``ValueError``."""
    if missing not in MISSING_MODES:
        raise ValueError(f"missing key points: expected one of {MISSING_MODES}, got {missing!r}")
    return missing == "skip"


def _gaps_flags(kind, affine) -> int:
    return (GAPS_GENERIC if _fk_kind(kind) == 1 else GAPS_SEQ) | (GAPS_AFFINE if affine else 0)


def gaps_compact_device(d_pose, n_seq, n_legs, n_frames, legs, d_cpose, d_map, d_n_valid, kind="seq", affine=False,
                        stream=0):
    """``seqik_gaps_compact_device``: pose (S, L, N, 5, 3) float64 -> the compacted and padded pose (same shape), the
    frame map (S, L, N) int32 (compact slot, -1 = missing) and n_valid (S, L) int32.  Raw device pointers (ints) or torch
    tensors; asynchronous on ``stream`` (a hipStream_t as int, or a torch stream).  ``kind`` ("seq" / "generic") and
    ``affine`` (the solve will use the fused alignment) decide which key points count (include/seqik_gaps.h)."""
    lf, ch = (n_seq, n_legs, n_frames), (n_seq, n_legs)
    _call("seqik_gaps_compact_device", _ptr(d_pose, "pose", lf + (5, 3)), int(n_seq), int(n_legs), int(n_frames),
          _gaps_flags(kind, affine), (SeqikLegParams * n_legs)(*legs), _ptr(d_cpose, "cpose", lf + (5, 3)),
          _ptr(d_map, "map", lf, "int32"), _ptr(d_n_valid, "n_valid", ch, "int32"), _stream_ptr(stream))


def gaps_expand_device(d_map, n_seq, n_legs, n_frames, d_cangles, d_angles, d_cfk=0, d_fk=0, d_cstatus=0, d_status=0,
                       d_cnfev=0, d_nfev=0, kind="seq", stream=0):
    """``seqik_gaps_expand_device``: compact angles / fk / status / nfev back to original frame order; NaN,
    ``STATUS_MISSING`` and 0 at the missing frames.  fk, status and nfev are optional pairs."""
    lf = (n_seq, n_legs, n_frames)
    sw = (1,) if _fk_kind(kind) == 1 else (4,)
    _call("seqik_gaps_expand_device", _ptr(d_map, "map", lf, "int32"), int(n_seq), int(n_legs), int(n_frames),
          _gaps_flags(kind, False), _ptr(d_cangles, "cangles", lf + (7,)), _ptr(d_cfk, "cfk", lf + (9, 3)),
          _ptr(d_cstatus, "cstatus", lf + sw, "int32"), _ptr(d_cnfev, "cnfev", lf + sw, "int32"),
          _ptr(d_angles, "angles", lf + (7,)), _ptr(d_fk, "fk", lf + (9, 3)), _ptr(d_status, "status", lf + sw, "int32"),
          _ptr(d_nfev, "nfev", lf + sw, "int32"), _stream_ptr(stream))


def solve_seq_gaps_device(d_pose, n_seq, n_legs, n_frames, legs, d_angles, d_cpose, d_map, d_n_valid, d_cangles,
                          d_fk=0, d_cfk=0, d_status=0, d_cstatus=0, d_nfev=0, d_cnfev=0, affine=None, d_init=0, stream=0,
                          **solve_options):
    """Skip mode on device buffers: compact -> ``solve_seq_device`` -> expand, enqueued on ``stream`` from caller-provided
    buffers (raw pointers or torch tensors): the compacted pose, map and n_valid of ``gaps_compact_device`` and compact
    angles / fk / status / nfev of the solver's shapes.  ``solve_options``: the frame-chunk and launch options of
    ``solve_seq_device``.  Equals ``solve_seq(..., missing="skip")`` bit for bit."""
    def raw(x, name, shape, dtype="float64"):
        p = _ptr(x, name, shape, dtype)
        return p.value or 0 if p is not None else 0
    lf = (n_seq, n_legs, n_frames)
    def given(x):
        return x is not None and (hasattr(x, "data_ptr") or int(x) != 0)
    for a, b, name in ((d_fk, d_cfk, "fk"), (d_status, d_cstatus, "status"), (d_nfev, d_cnfev, "nfev")):
        if given(a) != given(b):
            raise ValueError(f"{name} and c{name} are a pair: give both or neither")
    # every buffer is checked here, before anything is enqueued
    c_ptrs = (raw(d_cpose, "cpose", lf + (5, 3)), raw(d_cangles, "cangles", lf + (7,)), raw(d_cfk, "cfk", lf + (9, 3)),
              raw(d_cstatus, "cstatus", lf + (4,), "int32"), raw(d_cnfev, "cnfev", lf + (4,), "int32"),
              raw(d_init, "init", (n_seq, n_legs, 7)))
    for x, name, shape, dt in ((d_pose, "pose", lf + (5, 3), "float64"), (d_angles, "angles", lf + (7,), "float64"),
                               (d_map, "map", lf, "int32"), (d_n_valid, "n_valid", (n_seq, n_legs), "int32"),
                               (d_fk, "fk", lf + (9, 3), "float64"), (d_status, "status", lf + (4,), "int32"),
                               (d_nfev, "nfev", lf + (4,), "int32")):
        raw(x, name, shape, dt)
    if not raw(d_pose, "pose", lf + (5, 3)) or not raw(d_angles, "angles", lf + (7,)) or not c_ptrs[0] or not c_ptrs[1]:
        raise ValueError("pose, angles, cpose and cangles must be given")
    s = _stream_ptr(stream)
    s = s.value or 0 if s is not None else 0
    gaps_compact_device(d_pose, n_seq, n_legs, n_frames, legs, d_cpose, d_map, d_n_valid, kind="seq",
                        affine=affine is not None, stream=s)
    solve_seq_device(c_ptrs[0], n_seq, n_legs, n_frames, legs, c_ptrs[1], c_ptrs[2], c_ptrs[3], c_ptrs[4], stream=s,
                     affine=affine, d_init=c_ptrs[5], **solve_options)
    gaps_expand_device(d_map, n_seq, n_legs, n_frames, d_cangles, d_angles, d_cfk, d_fk, d_cstatus, d_status, d_cnfev,
                       d_nfev, kind="seq", stream=s)


#: entry points of include/seqik_stream_gaps.h (skip mode on streams), additive to ABI 7
STREAM_GAPS_EXPORTED_SYMBOLS = [sig[0] for sig in STREAM_GAPS_SIGNATURES["seqik_stream_gaps.h"]]


def stream_seed_state(legs, generic=False) -> np.ndarray:
    """``seqik_stream_seed_state``: (L, 7) joint angles in ``DOFS`` order, the ``init_angles`` that are bit-equivalent to
    none -- the start values of every stage's active joints (``seeds[[1, 2, 7, 8, 15, 16, 25]]``), for the generic chain
    those of its seven joints.  What a carried skip stream starts from (``SeqikStream.get_carry``).  No GPU needed."""
    n = len(legs)
    state = np.zeros((n, 7))
    _call("seqik_stream_seed_state", (SeqikLegParams * n)(*legs), n, 1 if generic else 0, _data(state))
    return state


#: entry points of include/seqik_resample.h (PCHIP resampling of joint angles), kept apart from the ABI-7 set of seqik.h
RESAMPLE_EXPORTED_SYMBOLS = [sig[0] for sig in SIGNATURES["seqik_resample.h"]]
RESAMPLE_BRIDGE = 1
RESAMPLE_MODES = ("error", "bridge")
RESAMPLE_MAX_WIDTH = 16


def resample_count(n_frames, original_ts, new_ts) -> int:
    """``seqik_resample_count``: samples per chain, ``len(np.arange(0, n_frames * original_ts, new_ts))``.  No GPU
    needed.  ``ValueError`` for fewer than 2 frames or time steps that are not finite and positive."""
    n = load().seqik_resample_count(int(n_frames), float(original_ts), float(new_ts))
    if n < 0:
        _raise(int(n))
    return int(n)


def _resample_flags(missing, max_gap):
    if missing not in RESAMPLE_MODES:
        raise ValueError(f"missing: expected one of {RESAMPLE_MODES}, got {missing!r}")
    if max_gap is not None and missing != "bridge":
        raise ValueError("max_gap needs missing='bridge'")
    if max_gap is not None and (int(max_gap) != max_gap or max_gap < 0 or max_gap > 2**31 - 1):
        raise ValueError(f"max_gap must be None (unlimited) or an integer in 0 .. 2^31 - 1, got {max_gap!r}")
    return (RESAMPLE_BRIDGE if missing == "bridge" else 0), (-1 if max_gap is None else int(max_gap))


def _resample_host_args(y, original_ts, new_ts, missing, max_gap):
    """What ``resample_pchip`` and ``resample_pchip_der`` check and hand on: the contiguous float64 ``y`` (..., N, W), the
    shape of one output plane, and the arguments of the C call in front of and behind the output pointers."""
    flags, gap = _resample_flags(missing, max_gap)
    y = np.ascontiguousarray(y, dtype=np.float64)
    if y.ndim < 2:
        raise ValueError(f"y must have shape (..., N, W), got {y.shape}")
    N, W = y.shape[-2:]
    if not 1 <= W <= RESAMPLE_MAX_WIDTH:
        raise ValueError(f"the record width must lie in 1..{RESAMPLE_MAX_WIDTH}, got {W}")
    if N < 2:
        raise ValueError("The number of knots must be at least 2 (scipy: `x` must contain at least 2 elements)")
    if not flags and not np.isfinite(y).all():
        raise ValueError("`y` must contain only finite values (missing='bridge' resamples over the finite records)")
    n_out = resample_count(N, original_ts, new_ts)
    C = int(np.prod(y.shape[:-2], dtype=np.int64))
    return y.shape[:-2] + (n_out, W), (_data(y), C, N, W, float(original_ts), float(new_ts), flags, gap), n_out


def resample_pchip(y, original_ts, new_ts, missing="error", max_gap=None, device=-1):
    """``seqik_resample_pchip`` on a host array: records ``(..., N, W)`` float64 (W in 1..16) at time step
    ``original_ts`` -> ``(..., n_out, W)`` at ``new_ts`` with scipy's PCHIP (``pchip_interpolate``), every leading index a
    chain of its own.  Knot j sits at ``j * original_ts``, sample i at ``i * new_ts``, ``n_out = resample_count(...)``;
    the samples behind the last knot continue the last cubic, as scipy does.

    ``missing``: ``"error"`` (default) refuses non-finite input with ``ValueError``, as scipy does; ``"bridge"`` treats a
    record with a non-finite value as a missing knot and resamples every chain over its valid knots alone
    (``pchip_interpolate(x[valid], y[valid], u)``): NaN in front of the first valid knot, from one ``original_ts`` behind
    the last one, and throughout a chain with fewer than two valid knots.  ``max_gap`` (bridge mode): samples strictly
    inside an interval that spans more than ``max_gap`` missing knots stay NaN; None = no limit."""
    shape, front, n_out = _resample_host_args(y, original_ts, new_ts, missing, max_gap)
    out = np.full(shape, np.nan)
    _call("seqik_resample_pchip", *front, _data(out), n_out, int(device))
    return out


def resample_workspace_bytes(n_chains, n_frames, missing="error") -> int:
    """``seqik_resample_workspace_bytes``: size of the workspace ``resample_pchip_device`` needs (8 B per knot in bridge
    mode, else 0)."""
    return int(load().seqik_resample_workspace_bytes(int(n_chains), int(n_frames), _resample_flags(missing, None)[0]))


def _resample_device_call(name, d_y, n_chains, n_frames, width, original_ts, new_ts, planes, missing, max_gap,
                          d_workspace, stream):
    """``name`` (one of the two ``_device`` entry points) with ``planes``: (argument name, pointer or tensor) per output."""
    flags, gap = _resample_flags(missing, max_gap)
    n_out = resample_count(n_frames, original_ts, new_ts)
    ws = _ptr(d_workspace, "workspace", (2, n_chains, n_frames), "int32")
    _call(name, _ptr(d_y, "y", (n_chains, n_frames, width)), int(n_chains), int(n_frames), int(width), float(original_ts),
          float(new_ts), flags, gap, *[_ptr(d, what, (n_chains, n_out, width)) for what, d in planes], n_out, ws,
          _stream_ptr(stream))
    return n_out


def resample_pchip_device(d_y, n_chains, n_frames, width, original_ts, new_ts, d_out, missing="error", max_gap=None,
                          d_workspace=0, stream=0):
    """``seqik_resample_pchip_device``: ``d_y`` (C, N, W) -> ``d_out`` (C, n_out, W) float64, raw device pointers (ints) or
    torch tensors, asynchronous on ``stream`` (a hipStream_t as int, or a torch stream).  Nothing is checked per frame:
    in the default mode a non-finite knot makes the samples whose stencil touches it NaN.  ``d_workspace`` (bridge mode):
    ``resample_workspace_bytes`` bytes; as a tensor, int32 of ``2 * C * N`` elements (prev, then next).  Returns n_out."""
    return _resample_device_call("seqik_resample_pchip_device", d_y, n_chains, n_frames, width, original_ts, new_ts,
                                 [("out", d_out)], missing, max_gap, d_workspace, stream)


#: entry points of include/seqik_resample_der.h (derivatives of the PCHIP interpolant), additive to ABI 7
RESAMPLE_DER_EXPORTED_SYMBOLS = [sig[0] for sig in EXTENSION_SIGNATURES["seqik_resample_der.h"]]
RESAMPLE_DER_ORDERS = (0, 1, 2)


def _resample_orders(der):
    """``der`` (an int or a sequence of ints) -> tuple of orders in 0..2 without repeats, or ``ValueError``."""
    if isinstance(der, (bool, np.bool_)) or isinstance(der, (str, bytes)):
        raise ValueError(f"der: expected orders out of {RESAMPLE_DER_ORDERS}, got {der!r}")
    orders = (der,) if isinstance(der, (int, np.integer)) else tuple(der) if np.iterable(der) else None
    if not orders or any(isinstance(o, (bool, np.bool_)) or not isinstance(o, (int, np.integer))
                         or o not in RESAMPLE_DER_ORDERS for o in orders):
        raise ValueError(f"der: expected one or more orders out of {RESAMPLE_DER_ORDERS}, got {der!r}")
    if len(set(orders)) != len(orders):
        raise ValueError(f"der: an order is given twice in {der!r}")
    return tuple(int(o) for o in orders)


def resample_pchip_der(y, original_ts, new_ts, der=(0, 1), missing="error", max_gap=None, device=-1):
    """``seqik_resample_der`` on a host array: the derivatives of the interpolant ``resample_pchip`` evaluates, what
    ``scipy.interpolate.pchip_interpolate(x, y, u, der=...)`` returns.  ``y``, the time steps, ``missing`` and ``max_gap``
    are ``resample_pchip``'s, with the same checks; ``der``: the orders wanted out of 0 (the value, ``resample_pchip``'s
    bits), 1 and 2, without repeats.  Returns a tuple of ``(..., n_out, W)`` arrays in the order of ``der``, in units of
    ``y`` per unit of ``original_ts`` (squared for order 2).  Every order is NaN exactly where the value is."""
    orders = _resample_orders(der)
    shape, front, n_out = _resample_host_args(y, original_ts, new_ts, missing, max_gap)
    planes = [np.full(shape, np.nan) if k in orders else None for k in RESAMPLE_DER_ORDERS]
    _call("seqik_resample_der", *front, *[_data(plane) for plane in planes], n_out, int(device))
    return tuple(planes[k] for k in orders)


def resample_der_device(d_y, n_chains, n_frames, width, original_ts, new_ts, d_value=0, d_d1=0, d_d2=0, missing="error",
                        max_gap=None, d_workspace=0, stream=0):
    """``seqik_resample_der_device``: ``d_y`` (C, N, W) -> those of ``d_value``, ``d_d1``, ``d_d2`` (C, n_out, W) float64
    that are given (0 / None: not computed, not written; at least one), raw device pointers (ints) or torch tensors,
    asynchronous on ``stream``.  ``d_workspace`` and what is (not) checked: ``resample_pchip_device``.  Returns n_out."""
    return _resample_device_call("seqik_resample_der_device", d_y, n_chains, n_frames, width, original_ts, new_ts,
                                 [("value", d_value), ("d1", d_d1), ("d2", d_d2)], missing, max_gap, d_workspace, stream)


#: entry points of include/seqik_head_align.h (antenna alignment on the GPU), kept apart from the ABI-7 set of seqik.h
HEAD_ALIGN_EXPORTED_SYMBOLS = [sig[0] for sig in SIGNATURES["seqik_head_align.h"]]
#: what the antenna-alignment kernels are compiled from (``csrc_sha256(HEAD_ALIGN_SOURCES)`` ties
#: profiles/head_align.json to a build; ``KERNEL_SOURCES`` stays the solver's own set)
HEAD_ALIGN_SOURCES = ["seqik_head.hpp", "seqik_head_align.hpp", "seqik_order_stats.hpp", "seqik_head_align.hip"]
HEAD_STAT_THRESHOLD = 5e-5


def _head_arrays(r_head, l_head, min_points=1, points="key points >= {}"):
    r_head = np.ascontiguousarray(r_head, dtype=np.float64)
    l_head = np.ascontiguousarray(l_head, dtype=np.float64)
    if r_head.ndim != 3 or r_head.shape[2] != 3 or r_head.shape[1] < min_points or l_head.shape != r_head.shape:
        raise ValueError(f"R_head / L_head must have the same shape (N, {points.format(min_points)}, 3)")
    return r_head, l_head


def _head_inputs(r_head, l_head, neck, compute_ant, head_roll, **shape_text):
    """What ``head_angles`` and ``head_angles_raw`` prepare alike -> (r_head, l_head, N, K, neck, neck stride, head_roll
    (N,) or None, zeroed angles (7 or 3, N))."""
    r_head, l_head = _head_arrays(r_head, l_head, **shape_text)
    n, k = r_head.shape[:2]
    if compute_ant and k < 2:
        # what the reference's get_ant_vector runs into (head_inverse_kinematics.py:159-161)
        raise IndexError(f"index 1 is out of bounds for axis 1 with size {k}: the antenna angles need the antenna base "
                         "and tip; call compute_head_angles(compute_ant_angles=False)")
    neck = np.ascontiguousarray(neck, dtype=np.float64).reshape(-1, 3)
    if neck.shape[0] not in (1, n):
        raise ValueError("Neck must hold one point or one point per frame")
    stride = 3 if (neck.shape[0] == n and n > 1) else 0
    if head_roll is not None and compute_ant:
        head_roll = np.ascontiguousarray(np.broadcast_to(np.asarray(head_roll, dtype=np.float64).reshape(-1), (n,)))
    else:
        head_roll = None
    return r_head, l_head, n, k, neck, stride, head_roll, np.zeros((7 if compute_ant else 3, n))


def head_align_stats(r_head, l_head, thorax, ranks_for, threshold=HEAD_STAT_THRESHOLD, device=-1):
    """``seqik_head_align_stats_*`` on host arrays: the order statistics AlignPose.align_head reduces, from RAW key
    points.  ``r_head`` / ``l_head`` (N, K >= 2, 3), ``thorax`` (N, P, 3) (points 0 and last are read), N >= 3.

    ``ranks_for(n) -> sequence of ranks`` is called once per side with that side's number of stationary frames and once
    with N (the ranks depend on sizes that are only known after the selection).  Returns dict(n_stat (2,) int64 for R, L;
    n_nonfinite; order): ``order`` (2, 5, n_ranks) holds per side the order statistics of base x, y, z and the
    base-to-thorax distance over the stationary frames and of the antenna length over all frames -- or None when the
    input held non-finite values or a side selected no frame (nothing is sorted then)."""
    r_head, l_head = _head_arrays(r_head, l_head, 2)
    n = r_head.shape[0]
    thorax = np.ascontiguousarray(thorax, dtype=np.float64)
    if thorax.ndim != 3 or thorax.shape[0] != n or thorax.shape[1] < 1 or thorax.shape[2] != 3:
        raise ValueError(f"Thorax must have shape ({n}, key points, 3), got {thorax.shape}")
    if n < 3:
        raise ValueError(f"the stationary-frame test needs at least 3 frames, got {n}")
    h = ctypes.c_void_p()
    _call("seqik_head_align_stats_open", ctypes.byref(h), n, ctypes.byref(SeqikOptions(device=device)))
    try:
        n_stat = np.zeros(2, dtype=np.int64)
        bad = ctypes.c_int64(0)
        _call("seqik_head_align_stats_select", h, r_head.ctypes.data, l_head.ctypes.data, thorax.ctypes.data, 0, n,
              r_head.shape[1], thorax.shape[1], float(threshold), _data(n_stat, _i64p), ctypes.byref(bad))
        out = dict(n_stat=n_stat, n_nonfinite=int(bad.value), order=None)
        if bad.value or not n_stat.all():
            return out
        ranks_stat = np.ascontiguousarray([list(ranks_for(int(k))) for k in n_stat], dtype=np.int64)
        ranks_all = np.ascontiguousarray(list(ranks_for(n)), dtype=np.int64)
        if ranks_stat.ndim != 2 or ranks_stat.shape[1] != ranks_all.shape[0]:
            raise ValueError("ranks_for must return the same number of ranks for every size")
        order = np.zeros((2, 5, ranks_all.shape[0]))
        _call("seqik_head_align_stats_pick", h, _data(ranks_stat, _i64p), _data(ranks_all, _i64p), ranks_all.shape[0],
              _data(order))
        out["order"] = order
        return out
    finally:
        load().seqik_head_align_stats_close(h)


def _head_affine_pair(affine):
    """(R, L) -> ``SeqikHeadAffine[2]``; each a ``SeqikHeadAffine`` or the tuple ``AlignPose.head_affine`` returns."""
    if isinstance(affine, dict):
        affine = (affine["R"], affine["L"])
    if len(affine) != 2:
        raise ValueError("two head affines expected: R, then L")
    return (SeqikHeadAffine * 2)(*[a if isinstance(a, SeqikHeadAffine) else make_head_affine(*a) for a in affine])


def head_angles_raw(r_head, l_head, neck, rest_head_pitch, rest_antenna_pitch, affine, compute_ant=True, device=-1,
                    head_roll=None, want_aligned=False):
    """``seqik_head_angles_raw`` on host arrays: ``head_angles`` on RAW key points, with the map of
    ``AlignPose.align_head`` (``affine``: ``{"R": ..., "L": ...}`` or an (R, L) pair of ``AlignPose.head_affine`` tuples /
    ``SeqikHeadAffine``) applied in the kernel's prologue.  Returns the (7 or 3, N) angles -- the bits ``head_angles``
    gives on the host-aligned points -- or, with ``want_aligned``, ``(angles, r_aligned, l_aligned)`` with the aligned
    key points (N, min(K, 2), 3)."""
    r_head, l_head, n, k, neck, stride, head_roll, out = _head_inputs(r_head, l_head, neck, compute_ant, head_roll)
    r_al = np.zeros((n, min(k, 2), 3)) if want_aligned else None
    l_al = np.zeros((n, min(k, 2), 3)) if want_aligned else None
    _call("seqik_head_angles_raw", _data(r_head), _data(l_head), n, k, _data(neck), stride, float(rest_head_pitch),
          float(rest_antenna_pitch), 1 if compute_ant else 0, _data(head_roll), _head_affine_pair(affine), _data(out),
          _data(r_al), _data(l_al), ctypes.byref(SeqikOptions(device=device)))
    return (out, r_al, l_al) if want_aligned else out


def head_angles_raw_device(d_r_head, d_l_head, n_frames, n_points, d_neck, neck_stride, rest_head_pitch,
                           rest_antenna_pitch, affine, d_angles, compute_ant=True, d_head_roll=0, d_r_aligned=0,
                           d_l_aligned=0, stream=0):
    """``seqik_head_angles_raw_device``: raw device pointers (ints) or torch tensors -- RAW records (N, K, 3), neck (3,) or
    (N, 3) by ``neck_stride`` 0 / 3, angles (7, N), optional aligned records (N, min(K, 2), 3) -- asynchronous on ``stream``
    (a hipStream_t as int, or a torch stream) of the current device."""
    n, k = int(n_frames), int(n_points)
    al = (n, min(k, 2), 3)
    _call("seqik_head_angles_raw_device", _ptr(d_r_head, "r_head", (n, k, 3)), _ptr(d_l_head, "l_head", (n, k, 3)), n, k,
          _ptr(d_neck, "neck", (n if neck_stride else 1, 3)), int(neck_stride), float(rest_head_pitch),
          float(rest_antenna_pitch), 1 if compute_ant else 0, _ptr(d_head_roll, "head_roll", (n,)),
          _head_affine_pair(affine), _ptr(d_angles, "angles", (7, n)), _ptr(d_r_aligned, "r_aligned", al),
          _ptr(d_l_aligned, "l_aligned", al), _stream_ptr(stream))


class AlignStats:
    """``seqik_align_stats_*``: order statistics of the seven per-leg series AlignPose reduces (coxa x, y, z and
    the four segment lengths), computed on the GPU.  ``add`` takes host arrays ``(S, L, N, 5, 3)`` (or a raw
    device pointer with ``on_device=True``); ``finish(ranks)`` returns ``(L, 7, len(ranks))``."""

    def __init__(self, n_legs, capacity_frames, device=-1):
        self.n_legs = int(n_legs)
        self._h = ctypes.c_void_p()
        try:
            _call("seqik_align_stats_open", ctypes.byref(self._h), self.n_legs, int(capacity_frames),
                  ctypes.byref(SeqikOptions(device=device)))
        except Exception:
            self._h = ctypes.c_void_p()
            raise

    def add(self, pose, n_seq=None, n_frames=None, layout=None, on_device=False, stream=0):
        """Appends ``n_seq x n_frames`` frames of every leg.  A host slab is copied to the GPU as one piece of
        ``n_seq * n_legs`` chain strides, so its ``layout`` must keep every key point of a chain inside the chain's
        stride: ``pose_chain``, ``pose_row``, ``pose_frame`` > 0 and
        ``4*pose_row + (n_frames-1)*pose_frame + 3 <= pose_chain`` (the rule of ``seqik_stream_open``; ``planar_layout``
        satisfies it), and the array must hold ``pose_chain * n_seq * n_legs`` doubles: ``ValueError`` otherwise.  For
        device memory the caller owns the extent (``pose_chain`` may exceed what a chain needs; 0 only for one chain)."""
        if (on_device or layout is not None) and (n_seq is None or n_frames is None):
            raise ValueError("n_seq and n_frames are required with a layout or device memory")
        if on_device:  # a raw device pointer or a tensor (its element count is checked in the dense layout only)
            ptr = _ptr(pose, "pose", None if layout is not None else (n_seq, self.n_legs, n_frames, 5, 3))
        else:
            pose = np.ascontiguousarray(pose, dtype=np.float64)
            if layout is None:
                if pose.ndim != 5 or pose.shape[1] != self.n_legs or pose.shape[3:] != (5, 3):
                    raise ValueError(f"pose must have shape (S, {self.n_legs}, N, 5, 3), got {pose.shape}")
                n_seq, n_frames = pose.shape[0], pose.shape[2]
            elif pose.size < layout.pose_chain * int(n_seq) * self.n_legs:
                raise ValueError(f"pose holds {pose.size} doubles, the layout addresses "
                                 f"{layout.pose_chain * int(n_seq) * self.n_legs} (pose_chain * n_seq * n_legs)")
            ptr = pose.ctypes.data
        _call("seqik_align_stats_add", self._h, ptr, 1 if on_device else 0, int(n_seq), int(n_frames),
              ctypes.byref(layout) if layout is not None else None, _stream_ptr(stream))

    def finish(self, ranks, stream=0):
        ranks = np.ascontiguousarray(ranks, dtype=np.int64)
        out = np.zeros((self.n_legs, 7, len(ranks)))
        _call("seqik_align_stats_finish", self._h, _data(ranks, _i64p), len(ranks), _data(out), _stream_ptr(stream))
        return out

    def reset(self):
        load().seqik_align_stats_reset(self._h)

    def close(self):
        if self._h:
            load().seqik_align_stats_close(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


PEER_HANDLE_BYTES = 64


class PeerBuffer:
    """Device memory that other processes can map (``seqik_peer_alloc`` / ``_export``) or the mapping of another
    process's buffer (``PeerBuffer.open(handle, nbytes)``).  ``tensor(shape)`` views it as a float64 torch tensor."""

    def __init__(self, nbytes, _mapped_ptr=None):
        self.nbytes = int(nbytes)
        self.mapped = _mapped_ptr is not None
        if self.mapped:
            self.ptr = _mapped_ptr
        else:
            p = ctypes.c_void_p()
            _call("seqik_peer_alloc", ctypes.byref(p), self.nbytes)
            self.ptr = p.value

    @classmethod
    def open(cls, handle: bytes, nbytes):
        assert len(handle) == PEER_HANDLE_BYTES
        p = ctypes.c_void_p()
        _call("seqik_peer_open", handle, ctypes.byref(p))
        return cls(nbytes, _mapped_ptr=p.value)

    def handle(self) -> bytes:
        buf = ctypes.create_string_buffer(PEER_HANDLE_BYTES)
        _call("seqik_peer_export", self.ptr, buf)
        return buf.raw

    @property
    def __cuda_array_interface__(self):
        return {"shape": (self.nbytes // 8,), "typestr": "<f8", "data": (self.ptr, False), "version": 2}

    def tensor(self, shape):
        import torch
        return torch.as_tensor(self, device="cuda").view(shape)

    def close(self):
        if self.ptr:
            ptr, self.ptr = self.ptr, None
            _call("seqik_peer_close" if self.mapped else "seqik_peer_free", ptr)


def peer_copy(dst_ptr, src_ptr, nbytes, stream=0):
    """``seqik_peer_copy``: asynchronous device-to-device copy of ``nbytes`` on ``stream`` (raw pointers or float64
    tensors; a hipStream_t as int or a torch stream)."""
    _call("seqik_peer_copy", _ptr(dst_ptr, "dst"), _ptr(src_ptr, "src"), nbytes, _stream_ptr(stream))


def release_workspaces():
    """Frees the per-stream stage hand-off workspaces the library keeps between calls (drains the device)."""
    _call("seqik_release_workspaces")


def device_attributes(device=0):
    """(compute units, peak clock in kHz, HBM bytes) of a GPU."""
    cu, khz, mem = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0)
    _call("seqik_device_attributes", device, ctypes.byref(cu), ctypes.byref(khz), ctypes.byref(mem))
    return cu.value, khz.value, mem.value


def solve_generic(pose, legs, want_fk=True, want_diag=False, device=-1, block_size=0, affine=None, init_angles=None,
                  lanes_per_wave=0, lane_groups=True, chain_queue=0, missing="raise"):
    """``seqik_solve_generic`` on host arrays: pose (S, L, N, 5, 3) -> dict(angles (S, L, N, 7),
    fk (S, L, N, 9, 3) or None, status / nfev (S, L, N) or None).  ``chain_queue`` (``SeqikOptions.reserved[1]``): batches
    of full wavefronts on persistent wavefronts whose lanes pull chains from a per-leg counter -- 0 = automatic (at least
    four chains per lane of the GPU), 1 = never, 2 = whenever full wavefronts are used; same bits either way.
    ``missing``: ``"raise"`` or ``"skip"`` as for ``solve_seq`` (``seqik_solve_generic_gaps``; rows 0 and 4 count, row 4
    only with ``affine``); skip mode adds ``n_valid`` (S, L)."""
    skip = check_missing_mode(missing)
    pose, (S, L, N) = _pose_batch(pose, legs, skip)
    out = dict(angles=np.zeros((S, L, N, 7)), fk=np.full((S, L, N, 9, 3), np.nan) if want_fk else None,
               status=np.full((S, L, N), -1, dtype=np.int32) if want_diag else None,
               nfev=np.zeros((S, L, N), dtype=np.int32) if want_diag else None)
    # reserved[3] = 3 (measurements): thin waves without the split over groups of 8 lanes
    opt = SeqikOptions(device=device, block_size=block_size,
                       reserved=(lanes_per_wave, chain_queue, 0, 0 if lane_groups else 3))
    return _solve_host("seqik_solve_generic", skip, pose, legs, (), out, init_angles, affine, opt)


def head_angles(r_head, l_head, neck, rest_head_pitch, rest_antenna_pitch, compute_ant=True, device=-1, head_roll=None):
    """``seqik_head_angles_ex`` on host arrays: (N, K, 3), (N, K, 3), neck (3,) or (N, 3) -> (7 or 3, N).

    K = key points per side: point 0 gives the head angles, point 1 (the antenna tip) the antenna angles; K = 1 is
    allowed without them.  ``head_roll`` (N,): derotate the antenna vectors by this roll instead of the frame's own."""
    r_head, l_head, n, k, neck, stride, head_roll, out = _head_inputs(r_head, l_head, neck, compute_ant, head_roll,
                                                                      points="key points")
    _call("seqik_head_angles_ex", _data(r_head), _data(l_head), n, k, _data(neck), stride, float(rest_head_pitch),
          float(rest_antenna_pitch), 1 if compute_ant else 0, _data(head_roll), _data(out),
          ctypes.byref(SeqikOptions(device=device)))
    return out


def signed_angles(v1, v2, rot_axis, device=-1):
    """``seqik_signed_angles``: the reference's ``angle_between_segments`` for (N, 3) arrays (either side may be one
    vector, used for every row) -> (N,)."""
    v1 = np.ascontiguousarray(np.asarray(v1, dtype=np.float64).reshape(-1, 3))
    v2 = np.ascontiguousarray(np.asarray(v2, dtype=np.float64).reshape(-1, 3))
    axis = np.ascontiguousarray(np.asarray(rot_axis, dtype=np.float64).reshape(3))
    n = max(v1.shape[0], v2.shape[0])
    if v1.shape[0] not in (1, n) or v2.shape[0] not in (1, n):
        raise ValueError(f"operands could not be broadcast together with shapes {v1.shape} {v2.shape}")
    out = np.zeros(n)
    _call("seqik_signed_angles", _data(v1), 3 if v1.shape[0] == n and n > 1 else 0, _data(v2),
          3 if v2.shape[0] == n and n > 1 else 0, _data(axis), n, _data(out), ctypes.byref(SeqikOptions(device=device)))
    return out


def make_leg_params(leg, bounds_dof, body_size, initial_angles) -> SeqikLegParams:
    """Packs the reference's dict-shaped chain description of one leg into the ABI struct."""
    lp = SeqikLegParams()
    for i, seg in enumerate(SEGMENTS):
        lp.seg[i] = float(body_size[f"{leg}_{seg}"])
    for i, dof in enumerate(DOFS):
        lb, ub = bounds_dof[f"{leg}_{dof}"]
        lp.bounds[i][0] = float(lb)
        lp.bounds[i][1] = float(ub)
    seeds = np.concatenate([np.asarray(initial_angles[leg][f"stage_{k}"], dtype=np.float64).ravel()
                            for k in (1, 2, 3, 4)])
    if seeds.shape != (27,):
        raise ValueError(f"initial_angles[{leg!r}] must hold 4, 6, 8 and 9 values for stage_1..stage_4")
    for i in range(27):
        lp.seeds[i] = float(seeds[i])
    return lp


def leg_params_from_arrays(seg, bounds, seeds) -> SeqikLegParams:
    lp = SeqikLegParams()
    for i in range(4):
        lp.seg[i] = float(seg[i])
    for i in range(7):
        lp.bounds[i][0] = float(bounds[i][0])
        lp.bounds[i][1] = float(bounds[i][1])
    for i in range(27):
        lp.seeds[i] = float(seeds[i])
    return lp


def validate_legs(legs, first_stage=1, last_stage=4):
    _call("seqik_validate_legs", (SeqikLegParams * len(legs))(*legs), len(legs), first_stage, last_stage)


def _check_finite(pose):
    """scipy refuses non-finite residuals at the start point (``ValueError: Residuals are not finite in
    the initial point.``); a NaN key point would do exactly that in the reference's frame loop."""
    if not np.isfinite(pose).all():
        raise ValueError("Residuals are not finite in the initial point.")


def _affine_array(affine, n_legs):
    if affine is None:
        return None
    if len(affine) != n_legs:
        raise ValueError("one SeqikAffine per leg expected")
    return (SeqikAffine * n_legs)(*affine)


def _pose_batch(pose, legs, skip):
    """The checks ``solve_seq`` and ``solve_generic`` share -> (pose as a contiguous float64 array, (S, L, N))."""
    pose = np.ascontiguousarray(pose, dtype=np.float64)
    if pose.ndim != 5 or pose.shape[3:] != (5, 3):
        raise ValueError(f"pose must have shape (S, L, N, 5, 3), got {pose.shape}")
    if len(legs) != pose.shape[1]:
        raise ValueError("one SeqikLegParams per leg expected")
    if not skip:
        _check_finite(pose)
    return pose, pose.shape[:3]


def _solve_host(name, skip, pose, legs, stages, out, init_angles, affine, opt):
    """Runs the host solver ``name`` -- in skip mode its ``_gaps`` twin, which also fills ``out["n_valid"]`` (S, L) -- into
    the arrays of ``out`` (angles, and fk / status / nfev or None) and returns ``out``."""
    S, L, N = pose.shape[:3]
    if init_angles is not None:
        init_angles = np.ascontiguousarray(init_angles, dtype=np.float64)
        if init_angles.shape != (S, L, 7):
            raise ValueError(f"init_angles must have shape {(S, L, 7)}")
    args = (_data(pose), S, L, N, (SeqikLegParams * L)(*legs), *stages, _data(out["angles"]), _data(out["fk"]),
            _data(out["status"], _ip), _data(out["nfev"], _ip), _data(init_angles), _affine_array(affine, L),
            ctypes.byref(opt))
    if skip:
        out["n_valid"] = np.zeros((S, L), dtype=np.int32)
        _call(name + "_gaps", *args, _data(out["n_valid"], _ip))
    else:
        _call(name, *args)
    return out


def _solve_options(block_size, lanes_per_wave, staged, interleave_legs, pipeline, frame_chunk, frame_halo, chunk_tol,
                   chunk_rounds) -> SeqikOptions:
    """``SeqikOptions`` with the launch and frame-chunk options ``solve_seq`` and ``solve_seq_device`` share."""
    opt = SeqikOptions()
    opt.block_size = block_size
    opt.reserved[0], opt.reserved[1], opt.reserved[2], opt.reserved[3] = lanes_per_wave, staged, interleave_legs, pipeline
    opt.frame_chunk, opt.frame_halo, opt.chunk_tol, opt.chunk_rounds = frame_chunk, frame_halo, chunk_tol, chunk_rounds
    return opt


def solve_seq(pose, legs, first_stage=1, last_stage=4, angles=None, want_fk=True, want_diag=False,
              device=-1, block_size=0, affine=None, init_angles=None, lanes_per_wave=0, staged=0, interleave_legs=0,
              frame_chunk=0, frame_halo=0, chunk_tol=0.0, chunk_rounds=0, pipeline=0, want_chunk_flags=False,
              missing="raise"):
    """``seqik_solve_seq`` on host arrays.

    pose: (S, L, N, 5, 3) float64; legs: list of L ``SeqikLegParams``; angles: optional
    (S, L, N, 7) with earlier-stage columns filled when ``first_stage > 1``.
    ``affine``: optional list of L ``SeqikAffine`` -- ``pose`` then holds RAW key points and the
    alignment is fused into the kernels.  ``lanes_per_wave``: chains per wavefront (0 = automatic; 128, 192, ... 4096 = the chain
    queue of the single-launch kernel, see ``SeqikOptions.reserved[0]``); ``staged=1``: one launch per stage instead of the single fused launch.
    ``frame_chunk`` (0 = serial walk, bit-exact; -1 = automatic; > 0 = frames per chunk), ``frame_halo``,
    ``chunk_tol``, ``chunk_rounds``: frame chunks, see ``SeqikOptions`` in include/seqik.h -- one long recording
    solved in concurrently running pieces, equal to the serial walk to about ``chunk_tol`` (default 1e-6 rad).
    ``pipeline``: stage pipeline (``SeqikOptions.reserved[3]``): 0 = automatic (few chains), 1 = never, 2 = always.
    ``device``: HIP device ordinal, -1 = the calling thread's current device.
    ``want_chunk_flags``: also return the per-chunk report ``chunk_flags`` (S, L, K) uint8 (``CHUNK_FLAG_*`` bits: failed
    the first verification / repaired / swept / chain walked serially); None when the call was not chunked.
    ``missing``: ``"raise"`` (default) refuses non-finite key points as the reference does; ``"skip"`` solves every chain
    as if its leg-frames with a non-finite key point were not in the recording (``seqik_solve_seq_gaps``,
    include/seqik_gaps.h): those get NaN angles and FK, status ``STATUS_MISSING`` and nfev 0, the others equal the solve
    of the compacted recording bit for bit.  Skip mode needs all four stages and no ``want_chunk_flags``; it adds
    ``n_valid`` (S, L) int32 to the result.
    Returns dict(angles, fk or None, status or None, nfev or None, chunk_stats, chunk_flags).
    """
    skip = check_missing_mode(missing)
    pose, (S, L, N) = _pose_batch(pose, legs, skip)
    if skip and (first_stage, last_stage) != (1, 4):
        raise ValueError("missing='skip' needs all four stages (first_stage=1, last_stage=4)")
    if skip and want_chunk_flags:
        raise ValueError("missing='skip' does not report chunk_flags")
    if angles is None:
        angles = np.zeros((S, L, N, 7), dtype=np.float64)
    else:
        angles = np.array(angles, dtype=np.float64, order="C", copy=True)
        if angles.shape != (S, L, N, 7):
            raise ValueError(f"angles must have shape {(S, L, N, 7)}")
    out = dict(angles=angles, fk=np.full((S, L, N, 9, 3), np.nan) if (want_fk and last_stage == 4) else None,
               status=np.full((S, L, N, 4), -1, dtype=np.int32) if want_diag else None,
               nfev=np.zeros((S, L, N, 4), dtype=np.int32) if want_diag else None)
    stats = np.zeros(N_CHUNK_STATS, dtype=np.int32)
    opt = _solve_options(block_size, lanes_per_wave, staged, interleave_legs, pipeline, frame_chunk, frame_halo, chunk_tol,
                         chunk_rounds)
    opt.device, opt.chunk_stats = device, _data(stats, _ip)
    flags = None
    if want_chunk_flags and frame_chunk != 0 and first_stage == 1 and last_stage == 4 and not want_diag:
        k = frame_chunk_plan(N, frame_chunk, frame_halo)[2]
        if k > 0:
            flags = np.zeros((S, L, k), dtype=np.uint8)
            opt.chunk_flags = _data(flags, _u8p)
    _solve_host("seqik_solve_seq", skip, pose, legs, (first_stage, last_stage), out, init_angles, affine, opt)
    out.update(chunk_stats=chunk_stats_dict(stats), chunk_flags=flags)
    return out


def solve_seq_device(d_pose, n_seq, n_legs, n_frames, legs, d_angles, d_fk=0, d_status=0, d_nfev=0,
                     first_stage=1, last_stage=4, stream=0, block_size=0, layout=None, affine=None, d_init=0,
                     stage_events=None, lanes_per_wave=0, staged=0, interleave_legs=0,
                     frame_chunk=0, frame_halo=0, chunk_tol=0.0, chunk_rounds=0, d_chunk_stats=0, pipeline=0,
                     frame_lead=0, d_chunk_flags=0, d_chunk_states=0, chunk_resume=0):
    """``seqik_solve_seq_device``: raw device pointers (ints) or torch tensors, asynchronous on ``stream`` (a hipStream_t
    as int, or a torch stream).
    ``layout``: a ``SeqikLayout`` (``planar_layout(n_frames)``) or None for the dense layout (in which a tensor's element
    count is checked as well).
    ``stage_events``: optional 5 raw hipEvent_t handles (e.g. ``torch.cuda.Event(...).cuda_event`` after a
    first ``record()``), recorded in front of each stage kernel and behind the last one."""
    opt = _solve_options(block_size, lanes_per_wave, staged, interleave_legs, pipeline, frame_chunk, frame_halo, chunk_tol,
                         chunk_rounds)
    opt.frame_lead, opt.chunk_resume = int(frame_lead), int(chunk_resume)
    stats = _ptr(d_chunk_stats, "chunk_stats", (N_CHUNK_STATS,), "int32")   # device int32[16]
    if stats:
        opt.chunk_stats = ctypes.cast(stats, _ip)
    flags = _ptr(d_chunk_flags, "chunk_flags", None, "uint8")   # device uint8 [n_seq][n_legs][K]
    if flags:
        opt.chunk_flags = ctypes.cast(flags, _u8p)
    states = _ptr(d_chunk_states, "chunk_states")   # device float64 [n_seq][n_legs][K][7]
    if states:
        opt.chunk_states = ctypes.cast(states, _dp)
    if stage_events is not None:
        ev = (ctypes.c_void_p * 5)(*[int(e) for e in stage_events])
        opt.stage_events = ctypes.cast(ev, ctypes.POINTER(ctypes.c_void_p))
    lf = (n_seq, n_legs, n_frames)

    def shape(*tail):   # a tensor's element count is known in the dense layout only
        return lf + tail if layout is None else None
    _call("seqik_solve_seq_device", _ptr(d_pose, "pose", shape(5, 3)), n_seq, n_legs, n_frames,
          (SeqikLegParams * n_legs)(*legs), first_stage, last_stage, _ptr(d_angles, "angles", shape(7)),
          _ptr(d_fk, "fk", shape(9, 3)), _ptr(d_status, "status", shape(4), "int32"),
          _ptr(d_nfev, "nfev", shape(4), "int32"), _ptr(d_init, "init", (n_seq, n_legs, 7)),
          ctypes.byref(layout) if layout is not None else None, _affine_array(affine, n_legs), ctypes.byref(opt),
          _stream_ptr(stream))


#: entry points of include/seqik_smooth.h (trajectory refinement: the whole-leg fit with smoothness across frames),
#: additive to ABI 7
SMOOTH_EXPORTED_SYMBOLS = [sig[0] for sig in SMOOTH_SIGNATURES["seqik_smooth.h"]]
SMOOTH_DEFAULT, SMOOTH_MAX_ITER = 0.1, 300   # SEQIK_SMOOTH_DEFAULT / SEQIK_SMOOTH_MAX_ITER


def _smooth_options(smooth, max_iter, gtol, ftol):
    s = np.asarray(smooth, dtype=np.float64)
    if s.shape not in ((), (7,)):
        raise ValueError(f"smooth must be a scalar or (7,), got {s.shape}")
    return ctypes.byref(SeqikSmoothOptions((ctypes.c_double * 7)(*np.broadcast_to(s, (7,))), int(max_iter), float(gtol),
                                           float(ftol)))


def smooth_workspace_bytes(n_seq, n_legs, n_frames):
    """``seqik_smooth_workspace_bytes``: the device workspace ``smooth_legs_device`` needs for these sizes."""
    n = (_lib or load()).seqik_smooth_workspace_bytes(int(n_seq), int(n_legs), int(n_frames))
    if n < 0:
        _raise(ERR_ARG)
    return n


def smooth_legs(angles, pose, legs, smooth=SMOOTH_DEFAULT, kp_weight=None, max_iter=SMOOTH_MAX_ITER, gtol=REFINE_GTOL,
                ftol=REFINE_FTOL, device=None):
    """``seqik_smooth_legs`` on host arrays: angles (S, L, N, 7) of the sequential chain -- normally the sequential fit's
    -- and the aligned key points (S, L, N, 5, 3) -> dict(angles (S, L, N, 7), frame_info (S, L, N) int32, cost (S, L,
    2), info (S, L, 3) int32).

    Every (sequence, leg) pair is ONE trajectory: a bounded Levenberg-Marquardt minimises, over all frames at once, the
    data term of ``refine_legs`` plus ``smooth[j] * len^2`` times the squared change of angle j between neighbouring
    frames (``smooth``: a scalar or (7,), dimensionless; ``len``: the leg length), inside ``legs[l].bounds``.  A frame
    with non-finite input (``frame_info`` bit 24, ``REFINE_BAD_INPUT``) gets NaN angles, takes no part and cuts the
    coupling there.  ``frame_info`` bits 0..6: DOF held on a limit.  ``cost[..., 0]`` is the objective at the clamped
    start, ``cost[..., 1]`` at the result (never larger).  ``info[..., 0]``: why the trajectory stopped
    (``REFINE_STOP_*``), ``info[..., 1]`` its accepted steps, ``info[..., 2]`` its rejected trials.  ``kp_weight``,
    ``gtol``, ``ftol``: as ``refine_legs``; ``max_iter`` 1..1000.  ``device=None``: the current device."""
    angles, (S, L, N), _, head = _angles_batch(angles, legs, 0)
    pose = np.ascontiguousarray(pose, dtype=np.float64)
    if pose.shape != (S, L, N, 5, 3):
        raise ValueError(f"pose must have shape {(S, L, N, 5, 3)}, got {pose.shape}")
    weight = None
    if kp_weight is not None:
        try:
            weight = np.ascontiguousarray(np.broadcast_to(np.asarray(kp_weight, dtype=np.float64), (S, L, N, 4)))
        except ValueError:
            raise ValueError(f"kp_weight must broadcast to {(S, L, N, 4)}") from None
    out = np.full((S, L, N, 7), np.nan)
    finfo = np.zeros((S, L, N), dtype=np.int32)
    cost = np.full((S, L, 2), np.nan)
    info = np.zeros((S, L, 3), dtype=np.int32)
    _call("seqik_smooth_legs", head[0], _data(pose), *head[1:], _data(weight), _smooth_options(smooth, max_iter, gtol, ftol),
          _data(out), _data(finfo, _ip), _data(cost), _data(info, _ip), -1 if device is None else int(device))
    return dict(angles=out, frame_info=finfo, cost=cost, info=info)


def smooth_legs_device(d_angles, d_pose, n_seq, n_legs, n_frames, legs, d_angles_out, d_workspace, workspace_bytes,
                       d_kp_weight=0, d_frame_info=0, d_cost=0, d_info=0, smooth=SMOOTH_DEFAULT, max_iter=SMOOTH_MAX_ITER,
                       gtol=REFINE_GTOL, ftol=REFINE_FTOL, stream=None):
    """``seqik_smooth_legs_device``: raw device pointers (ints) or torch tensors in the dense layouts of
    ``include/seqik_smooth.h`` (``d_angles_out`` may be ``d_angles``; ``d_frame_info`` (S, L, N) int32, ``d_cost`` (S, L,
    2) doubles, ``d_info`` (S, L, 3) int32; 0 / None: all weights 1, not written) and a workspace of
    ``smooth_workspace_bytes`` bytes (a pointer, or a uint8 tensor), on ``stream`` of the current device.  UNLIKE THE OTHER
    ``*_device`` WRAPPERS THIS ONE SYNCHRONISES THE STREAM, once per trial round; it returns with the last launch enqueued."""
    lf, head = _angle_map_head(d_angles, n_seq, n_legs, n_frames, legs, 0)
    tl = lf[:2]
    _call("seqik_smooth_legs_device", head[0], _ptr(d_pose, "pose", lf + (5, 3)), *head[1:],
          _ptr(d_kp_weight, "kp_weight", lf + (4,)), _smooth_options(smooth, max_iter, gtol, ftol),
          _ptr(d_angles_out, "angles_out", lf + (7,)), _ptr(d_frame_info, "frame_info", lf, dtype="int32"),
          _ptr(d_cost, "cost", tl + (2,)), _ptr(d_info, "info", tl + (3,), dtype="int32"),
          _ptr(d_workspace, "workspace", None, dtype="uint8"), int(workspace_bytes), _stream_ptr(stream))


#: entry points of include/seqik_smooth_sensitivity.h (error bars of the smoothed trajectory), additive to ABI 7
SMOOTH_SENS_EXPORTED_SYMBOLS = [sig[0] for sig in SMOOTH_SENS_SIGNATURES["seqik_smooth_sensitivity.h"]]
SMOOTH_SENS_MAX_HALF_WIDTH = 32
SMOOTH_SENS_FLAG_NOT_PD = 1 << 8
SMOOTH_SENS_FLAG_BAD_INPUT = 1 << 16
SMOOTH_SENS_FLAG_BAD_SIGMA = 1 << 17


def _smooth_vector(smooth):
    """``smooth`` (a scalar or (7,)) as the ``const double[7]`` of include/seqik_smooth_sensitivity.h."""
    s = np.asarray(smooth, dtype=np.float64)
    if s.shape not in ((), (7,)):
        raise ValueError(f"smooth must be a scalar or (7,), got {s.shape}")
    return (ctypes.c_double * 7)(*np.broadcast_to(s, (7,)))


def smooth_sensitivity_workspace_bytes(n_seq, n_legs, n_frames, half_width=0):
    """``seqik_smooth_sensitivity_workspace_bytes``: the device workspace ``smooth_sensitivity_device`` needs."""
    n = (_lib or load()).seqik_smooth_sensitivity_workspace_bytes(int(n_seq), int(n_legs), int(n_frames), int(half_width))
    if n < 0:
        _raise(ERR_ARG)
    return n


def smooth_sensitivity(angles, pose, legs, smooth=SMOOTH_DEFAULT, kp_weight=None, kp_sigma=None, half_width=0,
                       bound_tol=SENS_BOUND_TOL, want_sens=True, want_std=None, want_grad=True, want_flags=True, device=None):
    """``seqik_smooth_sensitivity`` on host arrays: angles (S, L, N, 7) that minimise the trajectory fit -- the output of
    ``smooth_legs`` with the same ``smooth`` and ``kp_weight`` -- and the aligned key points (S, L, N, 5, 3) they were
    fitted to -> dict(sens (S, L, N, 2 W + 1, 7, 4, 3), std (S, L, N, 7), grad (S, L, N), flags (S, L, N) int32; None for
    what is not asked for), W = ``half_width`` (0..32).

    ``sens[..., t, d, j, k, c]`` is the derivative of angle ``DOFS[j]`` of frame t with respect to component c of aligned
    key point k + 1 of frame t + d - W: the trajectory fit couples the frames, so an angle answers to the key points of
    its neighbours too.  A block whose source frame lies outside the recording, or beyond a frame with bad input, is 0.
    ``std``: the standard deviation of every angle under key-point noise ``kp_sigma`` that is independent between
    frames, key points and components -- ALL frames' noise, whatever ``half_width``.  THE VALUES ARE THE FIT'S RESPONSE
    ONLY AT ANGLES THAT MINIMISE IT: ``grad`` (per frame; its maximum over a trajectory is the left side of the gradient
    test of ``smooth_legs``) tells whether they do.  ``flags``: bits 0..6 DOF held, bit 8 (``SMOOTH_SENS_FLAG_NOT_PD``) the
    run of frames is not a strict minimum (free rows NaN), bit 16 bad input (the frame's values are NaN), bit 17
    (``SMOOTH_SENS_FLAG_BAD_SIGMA``) a negative or non-finite sigma (``std`` of the run is NaN).  ``device=None``: the
    current device."""
    angles, (S, L, N), _, head = _angles_batch(angles, legs, 0)
    pose = np.ascontiguousarray(pose, dtype=np.float64)
    if pose.shape != (S, L, N, 5, 3):
        raise ValueError(f"pose must have shape {(S, L, N, 5, 3)}, got {pose.shape}")
    try:
        weight = _sigma_batch(kp_weight, (S, L, N))
    except ValueError:
        raise ValueError(f"kp_weight must broadcast to {(S, L, N, 4)}, got {np.shape(kp_weight)}") from None
    try:
        sigma = _sigma_batch(kp_sigma, (S, L, N))
    except ValueError:
        raise ValueError(f"kp_sigma must broadcast to {(S, L, N, 4)}, got {np.shape(kp_sigma)}") from None
    if want_std is None:
        want_std = sigma is not None
    if want_std and sigma is None:
        raise ValueError("std needs kp_sigma")
    W = int(half_width)
    if not 0 <= W <= SMOOTH_SENS_MAX_HALF_WIDTH:
        raise ValueError(f"half_width must lie in 0..{SMOOTH_SENS_MAX_HALF_WIDTH}, got {half_width}")
    sens = np.full((S, L, N, 2 * W + 1, 7, 4, 3), np.nan) if want_sens else None
    std = np.full((S, L, N, 7), np.nan) if want_std else None
    grad = np.full((S, L, N), np.nan) if want_grad else None
    flags = np.zeros((S, L, N), dtype=np.int32) if want_flags else None
    _call("seqik_smooth_sensitivity", head[0], _data(pose), *head[1:], _data(weight), _data(sigma if want_std else None),
          _smooth_vector(smooth), float(bound_tol), W, _data(sens), _data(std), _data(grad), _data(flags, _ip),
          -1 if device is None else int(device))
    return dict(sens=sens, std=std, grad=grad, flags=flags)


def smooth_sensitivity_device(d_angles, d_pose, n_seq, n_legs, n_frames, legs, d_workspace, workspace_bytes, d_kp_weight=0,
                              d_kp_sigma=0, d_sens=0, d_std=0, d_grad=0, d_flags=0, smooth=SMOOTH_DEFAULT, half_width=0,
                              bound_tol=SENS_BOUND_TOL, stream=None):
    """``seqik_smooth_sensitivity_device``: raw device pointers (ints) or torch tensors in the dense layouts of
    ``include/seqik_smooth_sensitivity.h`` (``d_sens`` (S, L, N, 2 W + 1, 7, 4, 3), ``d_std`` (S, L, N, 7), ``d_grad`` (S,
    L, N) doubles, ``d_flags`` (S, L, N) int32; 0 / None: all weights 1, not computed, not written; at least one output)
    and a workspace of ``smooth_sensitivity_workspace_bytes`` bytes, asynchronous on ``stream`` of the current device.
    Unlike ``smooth_legs_device`` it allocates nothing and waits for nothing: at most five launches, fit for graph
    capture.  ``d_angles`` may be the output buffer of ``smooth_legs_device`` enqueued before it on the same stream."""
    lf, head = _angle_map_head(d_angles, n_seq, n_legs, n_frames, legs, 0)
    W = int(half_width)
    _call("seqik_smooth_sensitivity_device", head[0], _ptr(d_pose, "pose", lf + (5, 3)), *head[1:],
          _ptr(d_kp_weight, "kp_weight", lf + (4,)), _ptr(d_kp_sigma, "kp_sigma", lf + (4,)), _smooth_vector(smooth),
          float(bound_tol), W, _ptr(d_sens, "sens", lf + (2 * W + 1, 7, 4, 3)), _ptr(d_std, "std", lf + (7,)),
          _ptr(d_grad, "grad", lf), _ptr(d_flags, "flags", lf, dtype="int32"),
          _ptr(d_workspace, "workspace", None, dtype="uint8"), int(workspace_bytes), _stream_ptr(stream))
