"""Link frames from joint angles (seqik_link_frames_device): config-3 size, HIP-event timed.

One JSON line: 6 legs x 1 M frames (15625 recordings of 64 frames), sequential chain with an origin (80 B in, 864 B out per
leg-frame), for the per-lane and the LDS-staged kernel (SEQIK_FRAMES_STAGED; the staged one at 64, 128 and 256 threads per
workgroup, SEQIK_FRAMES_BLOCK), and as the bar a device-to-device copy with the same algorithmic traffic (read + write
bytes = the call's) timed in the same process.  Then Chain.forward_kinematics_many of the generic chain on the shipped
6000-frame recording through the GPU against the host loop, both timed here.
Usage: python scripts/bench_link_frames.py [n_seq] [launches]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "sequential-inverse-kinematics_amd"))
import json
import numpy as np, torch
from seqikpy_amd import _lib, data, utils
from seqikpy_amd.kinematic_chain import KinematicChainGeneric

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
org = torch.randn((S, L, N, 3), dtype=torch.float64, device="cuda", generator=g)
frames = torch.empty((S, L, N, 9, 3, 4), dtype=torch.float64, device="cuda")
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


nbytes = n * (80 + 864)
bar = copy_bar(nbytes // 2)
out = {"kernel": "seqik_frames_kernel", "leg_frames": n, "n_seq": S, "n_legs": L, "n_frames": N, "launches": K, "kind": "seq",
       "algorithmic_bytes": nbytes, "copy_bar": bar}
for variant, staged, block in (("per_lane", "0", "256"), ("lds_staged_64", "1", "64"), ("lds_staged_128", "1", "128"),
                               ("lds_staged_256", "1", "256")):
    os.environ["SEQIK_FRAMES_STAGED"], os.environ["SEQIK_FRAMES_BLOCK"] = staged, block
    t = timed(lambda: _lib.link_frames_device(ang.data_ptr(), S, L, N, params, frames.data_ptr(), kind="seq",
                                              d_origin=org.data_ptr(), stream=st))
    out[variant] = dict(t, leg_frames_per_s=n / t["ms_median"] * 1e3, GBps=nbytes / t["ms"] / 1e6,
                        GBps_median=nbytes / t["ms_median"] / 1e6, rate_vs_copy=bar["ms_median"] / t["ms_median"])
os.environ.pop("SEQIK_FRAMES_STAGED", None); os.environ.pop("SEQIK_FRAMES_BLOCK", None)
t = timed(lambda: _lib.link_frames_device(ang.data_ptr(), S, L, N, params, frames.data_ptr(), kind="seq",
                                          d_origin=org.data_ptr(), stream=st))
out["default"] = dict(t, rate_vs_copy=bar["ms_median"] / t["ms_median"])
del frames, ang, org

# Chain.forward_kinematics_many on the shipped recording: GPU route against the host loop, wall clock, same process
z = np.load(os.path.join(ROOT, "tests", "golden", "anipose_shipped.npz"))
chain = KinematicChainGeneric(data.BOUNDS, ["RF"]).create_leg_chain("RF")
q = np.zeros((z["RF_angles"].shape[0], 9))
q[:, 1:8] = z["RF_angles"][:, [2, 0, 1, 3, 4, 5, 6]]
chain.forward_kinematics_many(q[:64])  # library, context and arena warm
gpu = []
for _ in range(5):
    t0 = time.perf_counter(); a = chain.forward_kinematics_many(q); gpu.append(time.perf_counter() - t0)
t0 = time.perf_counter()
b = np.stack([np.stack(chain.forward_kinematics(r, full_kinematics=True)) for r in q])
host = time.perf_counter() - t0
out["forward_kinematics_many"] = {"frames": int(q.shape[0]), "gpu_route_ms_median": 1e3 * float(np.median(gpu)),
                                  "host_loop_ms": 1e3 * host, "speedup": host / float(np.median(gpu)),
                                  "max_abs_diff": float(np.abs(a - b).max())}
print(json.dumps(out))
