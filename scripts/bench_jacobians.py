"""Leg Jacobians from joint angles (seqik_leg_jacobians_device): config-3 size, HIP-event timed.

One JSON line: 6 legs x 1 M frames (15625 recordings of 64 frames), for three requests -- the Jacobian record alone (56 B
in, 672 B out per leg-frame), sigma + vel alone (112 B in, 160 B out: no record is formed), all three (112 B in, 832 B
out) -- each with the per-lane and the LDS-staged kernel (SEQIK_JAC_STAGED; staging concerns the record only), both chain
kinds, and as the bar a device-to-device copy with the same algorithmic traffic (read + write bytes = the call's) timed
in the same process.
Usage: python scripts/bench_jacobians.py [n_seq] [launches]"""
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
qdot = torch.randn((S, L, N, 7), dtype=torch.float64, device="cuda", generator=g)
jac = torch.empty((S, L, N, 4, 3, 7), dtype=torch.float64, device="cuda")
sigma = torch.empty((S, L, N, 8), dtype=torch.float64, device="cuda")
vel = torch.empty((S, L, N, 4, 3), dtype=torch.float64, device="cuda")
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
    total = 2 * (nbytes // 8) * 8
    return dict(t, bytes=total, GBps=total / t["ms"] / 1e6, GBps_median=total / t["ms_median"] / 1e6)


REQUESTS = {"jac_only": dict(bytes=56 + 672, q=0, j=1, s=0, v=0), "sigma_vel_only": dict(bytes=112 + 160, q=1, j=0, s=1, v=1),
            "all_three": dict(bytes=112 + 832, q=1, j=1, s=1, v=1)}
out = {"kernel": "seqik_jacobian_kernel", "leg_frames": n, "n_seq": S, "n_legs": L, "n_frames": N, "launches": K}
for name, r in REQUESTS.items():
    nbytes = n * r["bytes"]
    bar = copy_bar(nbytes // 2)
    res = {"algorithmic_bytes": nbytes, "copy_bar": bar}
    for kind in ("seq", "generic"):
        for variant, staged in (("per_lane", "0"), ("lds_staged", "1")):
            if not r["j"] and staged == "1":
                continue   # no record, nothing to stage: the same kernel
            os.environ["SEQIK_JAC_STAGED"] = staged
            t = timed(lambda: _lib.leg_jacobians_device(
                ang.data_ptr(), S, L, N, params, kind=kind, d_qdot=qdot.data_ptr() if r["q"] else 0,
                d_jac=jac.data_ptr() if r["j"] else 0, d_sigma=sigma.data_ptr() if r["s"] else 0,
                d_vel=vel.data_ptr() if r["v"] else 0, stream=st))
            res[f"{kind}_{variant}"] = dict(t, leg_frames_per_s=n / t["ms_median"] * 1e3, GBps=nbytes / t["ms"] / 1e6,
                                            GBps_median=nbytes / t["ms_median"] / 1e6,
                                            rate_vs_copy=bar["ms_median"] / t["ms_median"])
    os.environ.pop("SEQIK_JAC_STAGED", None)
    out[name] = res
print(json.dumps(out))
