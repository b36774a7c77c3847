"""PCHIP resampling of joint angles (seqik_resample_pchip_device): 6 legs x 1 M frames of width 7, HIP-event timed.

One JSON line.  Per case (ratio 10 and 100 in default mode, ratio 10 in bridge mode with 5 % missing frames -- the
neighbour tables are part of the timed call -- and ratio 1/10) the time per call, GB/s over the algorithmic bytes
(8 * width * (n_frames + n_out) per chain, + 8 B per knot in bridge mode) and, as the bar, a device-to-device copy that
moves the same bytes, timed in the same process.  Then what a user sees: utils.interpolate_joint_angles on the shipped
6000-frame, 14-series recording at 1e-2 -> 1e-4 s with on_gpu=False (scipy on the host) and on_gpu=True (both copies
included), wall clock.
Usage: python scripts/bench_resample.py [n_frames] [launches]"""
import json, os, sys, time
import numpy as np, torch
from bench_common import ROOT, copy_bar, timed
from seqikpy_amd import _lib, utils

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
K = int(sys.argv[2]) if len(sys.argv) > 2 else 20
C, W = 6, 7
st = torch.cuda.current_stream().cuda_stream


g = torch.Generator(device="cuda").manual_seed(5)
y = torch.cumsum(torch.randn((C, N, W), dtype=torch.float64, device="cuda", generator=g) * 0.01, dim=1).contiguous()
y_gaps = y.clone()
y_gaps[torch.rand((C, N), device="cuda", generator=g) < 0.05] = float("nan")
ws = torch.empty((2, C, N), dtype=torch.int32, device="cuda")
out = {"kernel": "seqik_resample_kernel", "n_chains": C, "n_frames": N, "width": W, "leg_frames": C * N, "launches": K}
for name, ots, nts, bridge in (("ratio_10", 1e-2, 1e-3, False), ("ratio_100", 1e-2, 1e-4, False),
                               ("ratio_10_bridge_5pct", 1e-2, 1e-3, True), ("ratio_0.1", 1e-3, 1e-2, False)):
    n_out = _lib.resample_count(N, ots, nts)
    launches = max(5, K // 4) if n_out > 20 * N else K
    nbytes = C * (8 * W * (N + n_out) + (8 * N if bridge else 0))
    bar = copy_bar(nbytes // 2, launches, 5)
    del bar["GBps_median"]
    d_out = torch.empty((C, n_out, W), dtype=torch.float64, device="cuda")
    src = y_gaps if bridge else y
    t = timed(lambda: _lib.resample_pchip_device(src, C, N, W, ots, nts, d_out, missing="bridge" if bridge else "error",
                                                 d_workspace=ws if bridge else 0, stream=st), launches, 5)
    gbps = nbytes / t["ms"] / 1e6
    out[name] = dict(t, n_out=n_out, algorithmic_bytes=nbytes, GBps=gbps, GBps_best_launch=nbytes / t["ms_min"] / 1e6,
                     samples_per_s=C * n_out / t["ms"] * 1e3, copy_bar=bar, rate_vs_copy=gbps / bar["GBps"])
    del d_out
    torch.cuda.empty_cache()

z = np.load(os.path.join(ROOT, "tests", "golden", "anipose_shipped.npz"))
series = {f"{leg}_{i}": np.array(z[f"{leg}_angles"][:, i]) for leg in ("RF", "LF") for i in range(7)}


def wall(fn, reps=3):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return {"s_best": min(ts), "s_all": ts}


utils.interpolate_joint_angles(series, original_ts=1e-2, new_ts=1e-3, on_gpu=True)  # context and arena exist
out["shipped_6000x14_1e-2_to_1e-4"] = {
    "host_scipy": wall(lambda: utils.interpolate_joint_angles(series, original_ts=1e-2, new_ts=1e-4)),
    "on_gpu_with_copies": wall(lambda: utils.interpolate_joint_angles(series, original_ts=1e-2, new_ts=1e-4, on_gpu=True)),
    "host_cpus": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()}
print(json.dumps(out))
