"""Link frames from joint angles (seqik_link_frames_device): config-3 size, HIP-event timed.

One JSON line: 6 legs x 1 M frames (15625 recordings of 64 frames), sequential chain with an origin (80 B in, 864 B out per
leg-frame), for the per-lane and the LDS-staged kernel (SEQIK_FRAMES_STAGED; the staged one at 64, 128 and 256 threads per
workgroup, SEQIK_FRAMES_BLOCK), and as the bar a device-to-device copy with the same algorithmic traffic (read + write
bytes = the call's) timed in the same process.  Then Chain.forward_kinematics_many of the generic chain on the shipped
6000-frame recording through the GPU against the host loop, both timed here.
Usage: python scripts/bench_link_frames.py [n_seq] [launches]"""
import json, os, sys, time
import numpy as np, torch
from bench_common import ROOT, config3_input, copy_bar, timed
from seqikpy_amd import _lib, data
from seqikpy_amd.kinematic_chain import KinematicChainGeneric

K = int(sys.argv[2]) if len(sys.argv) > 2 else 40
(S, L, N), params, ang, g, st = config3_input(int(sys.argv[1]) if len(sys.argv) > 1 else 15625)
n = S * L * N
org = torch.randn((S, L, N, 3), dtype=torch.float64, device="cuda", generator=g)
frames = torch.empty((S, L, N, 9, 3, 4), dtype=torch.float64, device="cuda")

nbytes = n * (80 + 864)
bar = copy_bar(nbytes // 2, K, 10)
out = {"kernel": "seqik_frames_kernel", "leg_frames": n, "n_seq": S, "n_legs": L, "n_frames": N, "launches": K, "kind": "seq",
       "algorithmic_bytes": nbytes, "copy_bar": bar}
for variant, staged, block in (("per_lane", "0", "256"), ("lds_staged_64", "1", "64"), ("lds_staged_128", "1", "128"),
                               ("lds_staged_256", "1", "256")):
    os.environ["SEQIK_FRAMES_STAGED"], os.environ["SEQIK_FRAMES_BLOCK"] = staged, block
    t = timed(lambda: _lib.link_frames_device(ang.data_ptr(), S, L, N, params, frames.data_ptr(), kind="seq",
                                              d_origin=org.data_ptr(), stream=st), K, 10)
    out[variant] = dict(t, leg_frames_per_s=n / t["ms_median"] * 1e3, GBps=nbytes / t["ms"] / 1e6,
                        GBps_median=nbytes / t["ms_median"] / 1e6, rate_vs_copy=bar["ms_median"] / t["ms_median"])
os.environ.pop("SEQIK_FRAMES_STAGED", None); os.environ.pop("SEQIK_FRAMES_BLOCK", None)
t = timed(lambda: _lib.link_frames_device(ang.data_ptr(), S, L, N, params, frames.data_ptr(), kind="seq",
                                          d_origin=org.data_ptr(), stream=st), K, 10)
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
