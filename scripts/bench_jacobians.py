"""Leg Jacobians from joint angles (seqik_leg_jacobians_device): config-3 size, HIP-event timed.

One JSON line: 6 legs x 1 M frames (15625 recordings of 64 frames), for three requests -- the Jacobian record alone (56 B
in, 672 B out per leg-frame), sigma + vel alone (112 B in, 160 B out: no record is formed), all three (112 B in, 832 B
out) -- each with the per-lane and the LDS-staged kernel (SEQIK_JAC_STAGED; staging concerns the record only), both chain
kinds, and as the bar a device-to-device copy with the same algorithmic traffic (read + write bytes = the call's) timed
in the same process.
Usage: python scripts/bench_jacobians.py [n_seq] [launches]"""
import json, os, sys
import torch
from bench_common import config3_input, copy_bar, timed
from seqikpy_amd import _lib

K = int(sys.argv[2]) if len(sys.argv) > 2 else 40
(S, L, N), params, ang, g, st = config3_input(int(sys.argv[1]) if len(sys.argv) > 1 else 15625)
n = S * L * N
qdot = torch.randn((S, L, N, 7), dtype=torch.float64, device="cuda", generator=g)
jac = torch.empty((S, L, N, 4, 3, 7), dtype=torch.float64, device="cuda")
sigma = torch.empty((S, L, N, 8), dtype=torch.float64, device="cuda")
vel = torch.empty((S, L, N, 4, 3), dtype=torch.float64, device="cuda")

REQUESTS = {"jac_only": dict(bytes=56 + 672, q=0, j=1, s=0, v=0), "sigma_vel_only": dict(bytes=112 + 160, q=1, j=0, s=1, v=1),
            "all_three": dict(bytes=112 + 832, q=1, j=1, s=1, v=1)}
out = {"kernel": "seqik_jacobian_kernel", "leg_frames": n, "n_seq": S, "n_legs": L, "n_frames": N, "launches": K}
for name, r in REQUESTS.items():
    nbytes = n * r["bytes"]
    bar = copy_bar(nbytes // 2, K, 10)
    res = {"algorithmic_bytes": nbytes, "copy_bar": bar}
    for kind in ("seq", "generic"):
        for variant, staged in (("per_lane", "0"), ("lds_staged", "1")):
            if not r["j"] and staged == "1":
                continue   # no record, nothing to stage: the same kernel
            os.environ["SEQIK_JAC_STAGED"] = staged
            t = timed(lambda: _lib.leg_jacobians_device(
                ang.data_ptr(), S, L, N, params, kind=kind, d_qdot=qdot.data_ptr() if r["q"] else 0,
                d_jac=jac.data_ptr() if r["j"] else 0, d_sigma=sigma.data_ptr() if r["s"] else 0,
                d_vel=vel.data_ptr() if r["v"] else 0, stream=st), K, 10)
            res[f"{kind}_{variant}"] = dict(t, leg_frames_per_s=n / t["ms_median"] * 1e3, GBps=nbytes / t["ms"] / 1e6,
                                            GBps_median=nbytes / t["ms_median"] / 1e6,
                                            rate_vs_copy=bar["ms_median"] / t["ms_median"])
    os.environ.pop("SEQIK_JAC_STAGED", None)
    out[name] = res
print(json.dumps(out))
