"""Forward kinematics from joint angles (seqik_forward_kinematics_device): config-3 size, HIP-event timed.

One JSON line: 6 legs x 1 M frames (15625 recordings of 64 frames), sequential chain, without and with pose + dist, for
the per-lane and the LDS-staged kernel (SEQIK_FK_STAGED), and as the bar a device-to-device copy with the same
algorithmic traffic (read + write bytes = the FK call's) timed in the same process.
Usage: python scripts/bench_fk.py [n_seq] [launches]"""
import json, os, sys
import torch
from bench_common import config3_input, copy_bar, timed
from seqikpy_amd import _lib

K = int(sys.argv[2]) if len(sys.argv) > 2 else 40
(S, L, N), params, ang, g, st = config3_input(int(sys.argv[1]) if len(sys.argv) > 1 else 15625)
n = S * L * N
pose = torch.randn((S, L, N, 5, 3), dtype=torch.float64, device="cuda", generator=g)
fk = torch.empty((S, L, N, 9, 3), dtype=torch.float64, device="cuda")
dist = torch.empty((S, L, N, 4), dtype=torch.float64, device="cuda")

cases = {"fk": dict(d_pose=0, d_dist=0, bytes=n * (56 + 216)),
         "fk_pose_dist": dict(d_pose=pose.data_ptr(), d_dist=dist.data_ptr(), bytes=n * (56 + 120 + 216 + 32))}
out = {"kernel": "seqik_fk_kernel", "leg_frames": n, "n_seq": S, "n_legs": L, "n_frames": N, "launches": K, "kind": "seq"}
for name, c in cases.items():
    bar = copy_bar(c["bytes"] // 2, K, 10)
    del bar["GBps_median"]
    row = {"algorithmic_bytes": c["bytes"], "copy_bar": bar}
    for variant in ("per_lane", "lds_staged"):
        os.environ["SEQIK_FK_STAGED"] = "1" if variant == "lds_staged" else "0"
        t = timed(lambda: _lib.forward_kinematics_device(ang.data_ptr(), S, L, N, params, fk.data_ptr(), kind="seq",
                                                         d_pose=c["d_pose"], d_dist=c["d_dist"], stream=st), K, 10)
        gbps = c["bytes"] / t["ms"] / 1e6
        row[variant] = dict(t, leg_frames_per_s=n / t["ms"] * 1e3, GBps=gbps, GBps_best_launch=c["bytes"] / t["ms_min"] / 1e6,
                            rate_vs_copy=gbps / bar["GBps"])
    os.environ.pop("SEQIK_FK_STAGED", None)
    out[name] = row
print(json.dumps(out))
