"""Antenna alignment on the GPU: (a) host align_head + head kernel against GPU statistics + fused kernel, host arrays in
and out on both sides (uploads included); (b) the fused kernel against the plain head kernel on pre-aligned device input.
Medians of repeated runs after a warm-up; (a) wall clock around synchronising calls, (b) HIP events.

    python scripts/bench_head_align.py [frames ...] [--out FILE]        (default: 1000000 16000000)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sequential-inverse-kinematics_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from seqikpy_amd import _lib  # noqa: E402
from seqikpy_amd.alignment import AlignPose  # noqa: E402
from seqikpy_amd.data import NMF_TEMPLATE  # noqa: E402
from seqikpy_amd.head_inverse_kinematics import HeadInverseKinematics  # noqa: E402


def recording(n):
    z = np.load(os.path.join(ROOT, "tests", "golden", "anipose_raw_cut.npz"))
    rng = np.random.default_rng(5)
    reps = -(-n // 1500)
    pose = {}
    for k in ("R_head", "L_head", "Thorax"):
        a = np.tile(z[f"raw_{k}"], (reps, 1, 1))[:n]
        pose[k] = a + rng.normal(scale=1e-4, size=a.shape)
    return pose


def median_wall(fn, repeats, warmup=1):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3, [round(v * 1e3, 3) for v in t]


def median_events(fn, launches=40, warmup=15):
    for _ in range(warmup):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(launches + 1)]
    ev[0].record()
    for i in range(launches):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    each = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(launches)])
    return float(np.median(each)), float(each.min()), float(each.max())


def bench(n):
    pose = recording(n)
    al = AlignPose(pose, legs_list=["RF", "LF"], include_claw=False, body_template=NMF_TEMPLATE, log_level="ERROR")
    neck = np.asarray(NMF_TEMPLATE["Neck"], dtype=np.float64).reshape(1, 3)
    hk0 = HeadInverseKinematics.from_raw(pose, NMF_TEMPLATE, al.head_affines(on_gpu=True), log_level="ERROR")
    rest = (hk0.rest_head_pitch, hk0.rest_antenna_pitch)
    keep = {}

    def host_align():
        keep["aligned"] = {s: al.align_head(pose[f"{s}_head"], s) for s in "RL"}

    def plain_kernel_host_arrays():
        keep["angles"] = _lib.head_angles(keep["aligned"]["R"], keep["aligned"]["L"], neck, *rest)

    def gpu_stats():
        keep["consts"] = al.head_affines(on_gpu=True)

    def fused_kernel_host_arrays():
        keep["angles_raw"] = _lib.head_angles_raw(pose["R_head"], pose["L_head"], neck, *rest, keep["consts"])

    big = n > 4_000_000
    out = {"frames": n}
    out["a_parent_align_head_both_sides_ms"], out["a_parent_align_head_runs_ms"] = median_wall(host_align, 3 if big else 5, 1)
    out["a_parent_head_angles_host_arrays_ms"], _ = median_wall(plain_kernel_host_arrays, 5, 2)
    out["a_new_head_affines_on_gpu_ms"], out["a_new_head_affines_runs_ms"] = median_wall(gpu_stats, 5, 2)
    out["a_new_head_angles_raw_host_arrays_ms"], _ = median_wall(fused_kernel_host_arrays, 5, 2)
    out["a_parent_total_ms"] = out["a_parent_align_head_both_sides_ms"] + out["a_parent_head_angles_host_arrays_ms"]
    out["a_new_total_ms"] = out["a_new_head_affines_on_gpu_ms"] + out["a_new_head_angles_raw_host_arrays_ms"]
    out["a_speedup"] = out["a_parent_total_ms"] / out["a_new_total_ms"]
    host_consts = al.head_affines()
    out["constants_equal_host"] = all(np.array_equal(np.asarray(a), np.asarray(b)) for s in "RL"
                                      for a, b in zip(keep["consts"][s], host_consts[s]))
    out["angles_equal"] = bool(np.array_equal(keep["angles"], keep["angles_raw"]))
    # (b) device buffers, kernels only
    d_raw = [torch.from_numpy(pose[k]).cuda() for k in ("R_head", "L_head")]
    d_al = [torch.from_numpy(keep["aligned"][s]).cuda() for s in "RL"]
    d_neck = torch.from_numpy(neck.copy()).cuda()
    d_ang = torch.zeros((7, n), dtype=torch.float64, device="cuda")
    d_out = [torch.zeros((n, 2, 3), dtype=torch.float64, device="cuda") for _ in range(2)]
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream

    def plain():
        assert lib.seqik_head_angles_device(d_al[0].data_ptr(), d_al[1].data_ptr(), n, d_neck.data_ptr(), 0, rest[0], rest[1],
                                            1, d_ang.data_ptr(), st) == 0
    aff = _lib._head_affine_pair(keep["consts"])

    def fused(with_out):
        def run():
            _lib.head_angles_raw_device(d_raw[0], d_raw[1], n, 2, d_neck, 0, rest[0], rest[1], aff, d_ang,
                                        d_r_aligned=d_out[0] if with_out else 0, d_l_aligned=d_out[1] if with_out else 0,
                                        stream=st)
        return run
    for name, fn in (("b_plain_kernel_ms", plain), ("b_fused_kernel_ms", fused(False)),
                     ("b_fused_kernel_aligned_out_ms", fused(True)), ("b_plain_kernel_again_ms", plain)):
        out[name], out[name + "_min"], out[name + "_max"] = median_events(fn)
    out["b_fused_over_plain"] = out["b_fused_kernel_ms"] / out["b_plain_kernel_ms"]
    return out


def main():
    args = sys.argv[1:]
    dest = None
    if "--out" in args:
        i = args.index("--out")
        dest = args[i + 1]
        del args[i:i + 2]
    sizes = [int(a) for a in args] or [1_000_000, 16_000_000]
    result = {"device": torch.cuda.get_device_name(0), "csrc_files": _lib.HEAD_ALIGN_SOURCES,
              "csrc_sha256": _lib.csrc_sha256(_lib.HEAD_ALIGN_SOURCES), "runs": [bench(n) for n in sizes]}
    text = json.dumps(result, indent=1)
    print(text)
    if dest:
        with open(dest, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
