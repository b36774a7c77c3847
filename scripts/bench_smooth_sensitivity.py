"""Error bars of the smoothed trajectory (seqik_smooth_sensitivity_device): HIP events around the device entry point,
median of 3 timings after a warm-up, next to the seqik_smooth_legs_device call of the same inputs in the same visit.

Workloads: RF + LF x 6000 frames of the shipped recording, and 64 recordings x 1000 frames x 2 legs (the first 1000 frames
tiled, the key points jittered).  Requests: std only, sens at half_width 0 and 4, and -- to see where the time goes --
flags only (assemble, Schur sweeps, verdict) and grad only (assemble).  The two serial launches are not timed from inside
the entry point; their share is read from differences: Schur sweeps <= flags_only - grad_only, covariance sweeps <=
std_only - sens_w0 (each difference also holds one cheap per-frame launch).

Every timed call runs in a process of its own under its own `timeout`, one after the other; the first that fails ends the
run.  The smoothed angles are made once per workload (by the process that times smooth_legs) and handed on in a file.

    python scripts/bench_smooth_sensitivity.py [--out FILE] [--limit SECONDS]
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sequential-inverse-kinematics_amd"))
import numpy as np  # noqa: E402

WORKLOADS = ("shipped", "batch64")
REQUESTS = ("smooth_legs", "std_only", "sens_w0", "sens_w4", "flags_only", "grad_only")
SMOOTH, SIGMA = 0.1, 0.01


def inputs(workload):
    from seqikpy_amd import _lib
    z = np.load(os.path.join(ROOT, "tests", "golden", "anipose_shipped.npz"))
    legs = ["RF", "LF"]
    params = [_lib.leg_params_from_arrays(z[f"{l}_seg"], z[f"{l}_bounds"], z[f"{l}_seeds"]) for l in legs]
    ang = np.ascontiguousarray(np.stack([z[f"{l}_angles"] for l in legs])[None])
    pose = np.ascontiguousarray(np.stack([z[f"{l}_pose"][:, :5] for l in legs])[None])
    if workload == "batch64":
        ang = np.ascontiguousarray(np.tile(ang[:, :, :1000], (64, 1, 1, 1)))
        pose = np.ascontiguousarray(np.tile(pose[:, :, :1000], (64, 1, 1, 1, 1)))
        pose[..., 1:, :] += np.random.default_rng(7).normal(scale=1e-3, size=pose[..., 1:, :].shape)
    return ang, pose, params


def timed(fn):
    """Median, min, max of 3 timings (ms) of one call, after one warm-up call."""
    import torch
    fn()
    torch.cuda.synchronize()
    each = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        each.append(a.elapsed_time(b))
    return dict(median_ms=float(np.median(each)), min_ms=float(min(each)), max_ms=float(max(each)))


def one(workload, request, cache):
    import torch
    from seqikpy_amd import _lib
    ang, pose, params = inputs(workload)
    S, L, N = ang.shape[:3]
    d_ang, d_pose = torch.from_numpy(ang).cuda(), torch.from_numpy(pose).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    out = dict(workload=workload, request=request, n_seq=S, n_legs=L, n_frames=N)
    if request == "smooth_legs":
        ws_bytes = _lib.smooth_workspace_bytes(S, L, N)
        d_ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")
        d_out = torch.empty_like(d_ang)
        d_info = torch.empty((S, L, 3), dtype=torch.int32, device="cuda")
        out.update(timed(lambda: _lib.smooth_legs_device(d_ang, d_pose, S, L, N, params, d_out, d_ws, ws_bytes, d_info=d_info,
                                                         smooth=SMOOTH, stream=stream)))
        info = d_info.cpu().numpy()
        reasons, counts = np.unique(info[..., 0], return_counts=True)      # over ALL trajectories
        out.update(workspace_bytes=int(ws_bytes), trajectories=int(S * L),
                   stop_reason_counts={str(int(r)): int(c) for r, c in zip(reasons, counts)},
                   steps_min_median_max=[int(info[..., 1].min()), float(np.median(info[..., 1])), int(info[..., 1].max())])
        np.save(cache, d_out.cpu().numpy())
        return out
    W = 4 if request == "sens_w4" else 0
    d_q = torch.from_numpy(np.load(cache)).cuda()
    ws_bytes = _lib.smooth_sensitivity_workspace_bytes(S, L, N, W)
    d_ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")
    d_sigma = torch.full((S, L, N, 4), SIGMA, dtype=torch.float64, device="cuda")
    bufs = dict(d_sens=torch.empty((S, L, N, 2 * W + 1, 7, 4, 3), dtype=torch.float64, device="cuda"),
                d_std=torch.empty((S, L, N, 7), dtype=torch.float64, device="cuda"),
                d_grad=torch.empty((S, L, N), dtype=torch.float64, device="cuda"),
                d_flags=torch.empty((S, L, N), dtype=torch.int32, device="cuda"))
    want = dict(std_only=("d_std",), sens_w0=("d_sens",), sens_w4=("d_sens",), flags_only=("d_flags",), grad_only=("d_grad",))[request]
    call = lambda keys: _lib.smooth_sensitivity_device(d_q, d_pose, S, L, N, params, d_ws, ws_bytes, d_kp_sigma=d_sigma,  # noqa: E731
                                                       smooth=SMOOTH, half_width=W, stream=stream, **{k: bufs[k] for k in keys})
    out.update(timed(lambda: call(want)))
    out.update(workspace_bytes=int(ws_bytes), half_width=W)
    if request == "std_only":      # what the numbers are: one more call, not timed
        call(("d_std", "d_grad", "d_flags"))
        torch.cuda.synchronize()
        std, grad, flags = (bufs[k].cpu().numpy() for k in ("d_std", "d_grad", "d_flags"))
        out["median_std_per_leg_at_sigma_0.01"] = [float(np.nanmedian(std[0, l])) for l in range(L)]
        out["median_std_per_angle_at_sigma_0.01"] = [[float(v) for v in np.nanmedian(std[0, l], axis=0)] for l in range(L)]
        out["max_grad_per_leg"] = [float(np.nanmax(grad[0, l])) for l in range(L)]
        out["frames_with_a_held_joint"] = int(((flags & 0x7F) != 0).sum())
        out["frames_not_a_strict_minimum"] = int(((flags & _lib.SMOOTH_SENS_FLAG_NOT_PD) != 0).sum())
    return out


def main():
    args = sys.argv[1:]
    if "--one" in args:
        i = args.index("--one")
        print("RESULT " + json.dumps(one(args[i + 1], args[i + 2], args[i + 3])))
        return 0
    dest = args[args.index("--out") + 1] if "--out" in args else None
    limit = args[args.index("--limit") + 1] if "--limit" in args else "150"
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        for workload in WORKLOADS:
            cache = os.path.join(tmp, workload + ".npy")
            for request in REQUESTS:
                cmd = ["timeout", "-k", "10", limit, sys.executable, os.path.abspath(__file__), "--one", workload, request, cache]
                proc = subprocess.run(cmd, capture_output=True, text=True)
                lines = [l for l in proc.stdout.splitlines() if l.startswith("RESULT ")]
                if proc.returncode != 0 or not lines:      # nothing more is started on the device after a failure
                    print(f"{workload} {request}: exit status {proc.returncode}\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}")
                    return 1
                runs.append(json.loads(lines[-1][7:]))
                print(lines[-1][7:], flush=True)
    by = {(r["workload"], r["request"]): r["median_ms"] for r in runs}
    summary = {}
    for w in WORKLOADS:
        summary[w] = dict(schur_sweeps_at_most_ms=by[w, "flags_only"] - by[w, "grad_only"],
                          covariance_sweeps_at_most_ms=by[w, "std_only"] - by[w, "sens_w0"],
                          std_only_over_smooth_legs=by[w, "std_only"] / by[w, "smooth_legs"])
        summary[w]["sweeps_share_of_std_only"] = ((summary[w]["schur_sweeps_at_most_ms"] + summary[w]["covariance_sweeps_at_most_ms"])
                                                  / by[w, "std_only"])
    import torch
    result = {"device": torch.cuda.get_device_name(0), "smooth": SMOOTH, "sigma": SIGMA, "runs": runs, "summary": summary}
    text = json.dumps(result, indent=1)
    print(text)
    if dest:
        os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
        with open(dest, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
