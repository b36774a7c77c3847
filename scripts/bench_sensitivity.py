"""Key-point sensitivity of the sequential fit (seqik_fit_sensitivity_device): config-3 size, HIP-event timed.

One JSON line: 6 legs x 1 M frames (15625 recordings of 64 frames), for three requests -- the record alone (176 B in, 672 B
out per leg-frame), std + flags alone (208 B in, 60 B out: no record is formed), all three (208 B in, 732 B out) -- each
with the per-lane and the LDS-staged kernel (SEQIK_SENS_STAGED; staging concerns the record only), and as the bar a
device-to-device copy with the same algorithmic traffic (read + write bytes = the call's) timed in the same process.  The
key points are random (the timing does not depend on them: the rule has no data-dependent branch).
Usage: python scripts/bench_sensitivity.py [n_seq] [launches]"""
import json, os, sys
import torch
from bench_common import config3_input, copy_bar, timed
from seqikpy_amd import _lib

K = int(sys.argv[2]) if len(sys.argv) > 2 else 40
(S, L, N), params, ang, g, st = config3_input(int(sys.argv[1]) if len(sys.argv) > 1 else 15625)
n = S * L * N
pose = torch.randn((S, L, N, 5, 3), dtype=torch.float64, device="cuda", generator=g)
kp_sigma = torch.rand((S, L, N, 4), dtype=torch.float64, device="cuda", generator=g)
sens = torch.empty((S, L, N, 7, 4, 3), dtype=torch.float64, device="cuda")
std = torch.empty((S, L, N, 7), dtype=torch.float64, device="cuda")
flags = torch.empty((S, L, N), dtype=torch.int32, device="cuda")

REQUESTS = {"sens_only": dict(bytes=176 + 672, s=1, r=0), "std_flags_only": dict(bytes=208 + 60, s=0, r=1),
            "all_three": dict(bytes=208 + 732, s=1, r=1)}
out = {"kernel": "seqik_sensitivity_kernel", "leg_frames": n, "n_seq": S, "n_legs": L, "n_frames": N, "launches": K}
for name, r in REQUESTS.items():
    nbytes = n * r["bytes"]
    bar = copy_bar(nbytes // 2, K, 10)
    res = {"algorithmic_bytes": nbytes, "copy_bar": bar}
    for variant, staged in (("per_lane", "0"), ("lds_staged", "1")):
        if not r["s"] and staged == "1":
            continue   # no record, nothing to stage: the same kernel
        os.environ["SEQIK_SENS_STAGED"] = staged
        t = timed(lambda: _lib.fit_sensitivity_device(
            ang.data_ptr(), pose.data_ptr(), S, L, N, params, d_kp_sigma=kp_sigma.data_ptr() if r["r"] else 0,
            d_sens=sens.data_ptr() if r["s"] else 0, d_std=std.data_ptr() if r["r"] else 0,
            d_flags=flags.data_ptr() if r["r"] else 0, stream=st), K, 10)
        res[variant] = dict(t, leg_frames_per_s=n / t["ms_median"] * 1e3, GBps_median=nbytes / t["ms_median"] / 1e6,
                            rate_vs_copy=bar["ms_median"] / t["ms_median"])
    os.environ.pop("SEQIK_SENS_STAGED", None)
    out[name] = res
print(json.dumps(out))
