"""Whole-leg refinement (seqik_refine_legs_device): leg-frames per second and iterations per lane, HIP-event timed.

One JSON line.  The time of a lane is its number of iterations, which depends on the data, so the input is real: RF and LF
of the shipped anipose recording (tests/golden/anipose_shipped.npz, 2 x 6000 frames), started from the shipped sequential
angles, repeated n_seq times (every copy does the same work: the rate is that of this recording, whatever the batch
size).  Reported: the rate, the accepted iterations per lane (mean, median, maximum), the mean over wavefronts of their
slowest lane (a wavefront takes as long as that lane: the ratio to the mean is what lane imbalance costs), the stop
reasons, and the rms key-point distance before and after.
Usage: python scripts/bench_refine.py [n_seq] [launches]"""
import json, os, sys
import numpy as np, torch
from bench_common import ROOT, timed
from seqikpy_amd import _lib

S = int(sys.argv[1]) if len(sys.argv) > 1 else 16
K = int(sys.argv[2]) if len(sys.argv) > 2 else 10
z = np.load(os.path.join(ROOT, "tests", "golden", "anipose_shipped.npz"))
legs = ["RF", "LF"]
L, N = len(legs), z["RF_angles"].shape[0]
params = [_lib.leg_params_from_arrays(z[f"{l}_seg"], z[f"{l}_bounds"], z[f"{l}_seeds"]) for l in legs]
ang = torch.from_numpy(np.broadcast_to(np.stack([z[f"{l}_angles"] for l in legs])[None], (S, L, N, 7)).copy()).cuda()
pose = torch.from_numpy(np.broadcast_to(np.stack([z[f"{l}_pose"][:, :5] for l in legs])[None], (S, L, N, 5, 3)).copy()).cuda()
out = torch.empty_like(ang)
cost = torch.empty((S, L, N, 2), dtype=torch.float64, device="cuda")
info = torch.empty((S, L, N), dtype=torch.int32, device="cuda")
st = torch.cuda.current_stream().cuda_stream
n = S * L * N

t = timed(lambda: _lib.refine_legs_device(ang.data_ptr(), pose.data_ptr(), S, L, N, params, out.data_ptr(),
                                          d_cost=cost.data_ptr(), d_info=info.data_ptr(), stream=st), K, 2)
torch.cuda.synchronize()
inf, c = info.cpu().numpy().reshape(-1), cost.cpu().numpy().reshape(-1, 2)
its = _lib.refine_iterations(inf)
waves = its[:len(its) // 64 * 64].reshape(-1, 64)
print(json.dumps({"kernel": "seqik_refine_kernel", "leg_frames": n, "n_seq": S, "n_legs": L, "n_frames": N, "launches": K, **t,
                  "leg_frames_per_s": n / t["ms_median"] * 1e3,
                  "iterations_per_lane": {"mean": float(its.mean()), "median": float(np.median(its)), "max": int(its.max())},
                  "mean_over_wavefronts_of_their_slowest_lane": float(waves.max(1).mean()),
                  "stop_reasons": {str(k): int(v) for k, v in enumerate(np.bincount(_lib.refine_stop_reason(inf), minlength=5)) if v},
                  "bad_input_lanes": int((inf == _lib.REFINE_BAD_INPUT).sum()),
                  "rms_key_point_distance": {"before": float(np.sqrt(c[:, 0].mean() / 4)), "after": float(np.sqrt(c[:, 1].mean() / 4))}}))
