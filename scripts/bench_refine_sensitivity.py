"""Error bars of the whole-leg refinement (seqik_refine_sensitivity_device): HIP events around the device entry point,
median of 3 timings after a warm-up, for the sens, the std-only and the flags-only request, on RF + LF x 6000 frames of the
shipped recording (refined on the GPU first) and on 1 M synthetic leg-frames (the same refined frames tiled, the key
points jittered); next to each a device-to-device copy of the bytes the sens request moves (672 + 56 + 120 B per
leg-frame), so that one can see whether the unit is bound by its store or by its FP64 arithmetic.  A timing is a run of
back-to-back launches long enough to be measured (one launch of 12 000 leg-frames is a few tens of microseconds).

    python scripts/bench_refine_sensitivity.py [--out FILE]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sequential-inverse-kinematics_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from seqikpy_amd import _lib  # noqa: E402

BYTES_IN, BYTES_SENS, BYTES_STD = 56 + 120, 672, 56


def timed(fn, launches):
    """Median, min, max of 3 timings (ms per launch) of `launches` back-to-back calls, after one warm-up run."""
    fn()
    torch.cuda.synchronize()
    each = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        each.append(a.elapsed_time(b) / launches)
    return dict(median_ms=float(np.median(each)), min_ms=float(min(each)), max_ms=float(max(each)), launches=launches)


def bench(name, ang, pose, params, launches):
    S, L, N = ang.shape[:3]
    n = S * L * N
    d_ang, d_pose = torch.from_numpy(ang).cuda(), torch.from_numpy(pose).cuda()
    d_sigma = torch.full((S, L, N, 4), 0.01, dtype=torch.float64, device="cuda")
    d_sens = torch.empty((S, L, N, 7, 4, 3), dtype=torch.float64, device="cuda")
    d_std = torch.empty((S, L, N, 7), dtype=torch.float64, device="cuda")
    d_grad = torch.empty((S, L, N), dtype=torch.float64, device="cuda")
    d_flags = torch.empty((S, L, N), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    # the angles the unit is for: the refinement's own, which never leave the device
    _lib.refine_legs_device(d_ang, d_pose, S, L, N, params, d_ang, stream=stream)
    torch.cuda.synchronize()
    call = lambda **out: (lambda: _lib.refine_sensitivity_device(d_ang, d_pose, S, L, N, params, d_kp_sigma=d_sigma,  # noqa: E731
                                                                 stream=stream, **out))
    moved = n * (BYTES_IN + BYTES_SENS + BYTES_STD)
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")     # a copy reads and writes: half the bytes each way
    dst = torch.empty_like(src)
    out = dict(name=name, leg_frames=n, bytes_per_leg_frame=BYTES_IN + BYTES_SENS + BYTES_STD)
    out["sens"] = timed(call(d_sens=d_sens), launches)
    out["sens_std_grad_flags"] = timed(call(d_sens=d_sens, d_std=d_std, d_grad=d_grad, d_flags=d_flags), launches)
    out["std_only"] = timed(call(d_std=d_std), launches)
    out["flags_only"] = timed(call(d_flags=d_flags), launches)
    out["copy_same_bytes"] = timed(lambda: dst.copy_(src), launches)
    out["sens_again"] = timed(call(d_sens=d_sens), launches)
    for k in ("sens", "sens_std_grad_flags", "std_only", "flags_only", "sens_again"):
        out[k]["leg_frames_per_s"] = n / (out[k]["median_ms"] * 1e-3)
    out["sens"]["store_GB_per_s"] = n * BYTES_SENS / (out["sens"]["median_ms"] * 1e-3) / 1e9
    out["copy_same_bytes"]["GB_per_s_read_plus_write"] = moved / (out["copy_same_bytes"]["median_ms"] * 1e-3) / 1e9
    out["sens_over_copy"] = out["sens"]["median_ms"] / out["copy_same_bytes"]["median_ms"]
    flags = d_flags.cpu().numpy()
    out["leg_frames_with_a_held_joint"] = int(((flags & 0x7F) != 0).sum())
    out["leg_frames_not_a_strict_minimum"] = int(((flags & _lib.REFINE_SENS_FLAG_NOT_PD) != 0).sum())
    std = d_std.cpu().numpy()
    out["median_std_per_angle_at_sigma_0.01"] = [float(v) for v in np.nanmedian(std.reshape(-1, 7), axis=0)]
    return out


def main():
    args = sys.argv[1:]
    dest = args[args.index("--out") + 1] if "--out" in args else None
    z = np.load(os.path.join(ROOT, "tests", "golden", "anipose_shipped.npz"))
    legs = ["RF", "LF"]
    params = [_lib.leg_params_from_arrays(z[f"{l}_seg"], z[f"{l}_bounds"], z[f"{l}_seeds"]) for l in legs]
    ang = np.ascontiguousarray(np.stack([z[f"{l}_angles"] for l in legs])[None])
    pose = np.ascontiguousarray(np.stack([z[f"{l}_pose"][:, :5] for l in legs])[None])
    runs = [bench("shipped RF + LF x 6000", ang, pose, params, launches=200)]
    reps = -(-500_000 // ang.shape[2])
    big_ang = np.ascontiguousarray(np.tile(ang, (1, 1, reps, 1))[:, :, :500_000])
    big_pose = np.ascontiguousarray(np.tile(pose, (1, 1, reps, 1, 1))[:, :, :500_000])
    big_pose[..., 1:, :] += np.random.default_rng(7).normal(scale=1e-3, size=big_pose[..., 1:, :].shape)
    runs.append(bench("synthetic 2 x 500000", big_ang, big_pose, params, launches=5))
    result = {"device": torch.cuda.get_device_name(0), "runs": runs}
    text = json.dumps(result, indent=1)
    print(text)
    if dest:
        os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
        with open(dest, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
