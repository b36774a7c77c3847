"""Forward kinematics from joint angles (seqik_forward_kinematics_device): config-3 size, HIP-event timed.

One JSON line: 6 legs x 1 M frames (15625 recordings of 64 frames), sequential chain, without and with pose + dist, for
the per-lane and the LDS-staged kernel (SEQIK_FK_STAGED), and as the bar a device-to-device copy with the same
algorithmic traffic (read + write bytes = the FK call's) timed in the same process.
Usage: python scripts/bench_fk.py [n_seq] [launches]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "sequential-inverse-kinematics_amd"))
import json
import numpy as np, torch
from seqikpy_amd import _lib, data, utils

S = int(sys.argv[1]) if len(sys.argv) > 1 else 15625
K = int(sys.argv[2]) if len(sys.argv) > 2 else 40
L, N = 6, 64
n = S * L * N
legs = data.LEGS
body = utils.calculate_body_size(data.TEMPLATE_NMF_LOCOMOTION, legs)
params = [_lib.make_leg_params(l, data.BOUNDS_LOCOMOTION, body, data.INITIAL_ANGLES_LOCOMOTION) for l in legs]
lb = torch.tensor([[data.BOUNDS_LOCOMOTION[f"{l}_{d}"][0] for d in data.DOFS] for l in legs], dtype=torch.float64).cuda()
ub = torch.tensor([[data.BOUNDS_LOCOMOTION[f"{l}_{d}"][1] for d in data.DOFS] for l in legs], dtype=torch.float64).cuda()
g = torch.Generator(device="cuda").manual_seed(3)
ang = (lb[None, :, None] + torch.rand((S, L, N, 7), dtype=torch.float64, device="cuda", generator=g) *
       (ub - lb)[None, :, None]).contiguous()
pose = torch.randn((S, L, N, 5, 3), dtype=torch.float64, device="cuda", generator=g)
fk = torch.empty((S, L, N, 9, 3), dtype=torch.float64, device="cuda")
dist = torch.empty((S, L, N, 4), dtype=torch.float64, device="cuda")
st = torch.cuda.current_stream().cuda_stream


def timed(fn):
    for _ in range(10):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(K + 1)]
    ev[0].record()
    for i in range(K):
        fn(); ev[i + 1].record()
    torch.cuda.synchronize()
    each = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(K)])
    return {"ms": float(each.mean()), "ms_min": float(each.min()), "ms_median": float(np.median(each))}


def copy_bar(nbytes):
    src = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    dst = torch.empty_like(src)
    t = timed(lambda: dst.copy_(src))
    del src, dst
    return dict(t, bytes=2 * (nbytes // 8) * 8, GBps=2 * (nbytes // 8) * 8 / t["ms"] / 1e6)


cases = {"fk": dict(d_pose=0, d_dist=0, bytes=n * (56 + 216)),
         "fk_pose_dist": dict(d_pose=pose.data_ptr(), d_dist=dist.data_ptr(), bytes=n * (56 + 120 + 216 + 32))}
out = {"kernel": "seqik_fk_kernel", "leg_frames": n, "n_seq": S, "n_legs": L, "n_frames": N, "launches": K, "kind": "seq"}
for name, c in cases.items():
    bar = copy_bar(c["bytes"] // 2)
    row = {"algorithmic_bytes": c["bytes"], "copy_bar": bar}
    for variant in ("per_lane", "lds_staged"):
        os.environ["SEQIK_FK_STAGED"] = "1" if variant == "lds_staged" else "0"
        t = timed(lambda: _lib.forward_kinematics_device(ang.data_ptr(), S, L, N, params, fk.data_ptr(), kind="seq",
                                                         d_pose=c["d_pose"], d_dist=c["d_dist"], stream=st))
        gbps = c["bytes"] / t["ms"] / 1e6
        row[variant] = dict(t, leg_frames_per_s=n / t["ms"] * 1e3, GBps=gbps, GBps_best_launch=c["bytes"] / t["ms_min"] / 1e6,
                            rate_vs_copy=gbps / bar["GBps"])
    os.environ.pop("SEQIK_FK_STAGED", None)
    out[name] = row
print(json.dumps(out))
