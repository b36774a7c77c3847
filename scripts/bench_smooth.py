"""Trajectory refinement (seqik_smooth_legs_device): milliseconds per call and per trial round, HIP-event timed.

One JSON line per case.  The work of a call is its number of trial rounds, which depends on the data, so the input is
real: the shipped anipose recording (tests/golden/anipose_shipped.npz) from the shipped sequential angles, smooth = 0.1.
  recording   RF + LF, 1 x 2 x 6000 frames: two long trajectories (13 strides of the cyclic reduction per round)
  batch       64 recordings of 1000 frames (the first 64 windows of 1000 frames that fit, RF and LF: 128 trajectories,
              10 strides per round); a trajectory that has stopped is skipped, so the late rounds are cheaper
The entry point waits for the stream once per round; the events span the whole call, those waits included.  A round is a
trial: rounds = the largest (accepted + rejected) of any trajectory.  Launches per round: 6 + 2 ceil(log2 n_frames).
Usage: python scripts/bench_smooth.py [calls]"""
import json, math, os, sys
import numpy as np, torch
from bench_common import ROOT, timed
from seqikpy_amd import _lib

K = int(sys.argv[1]) if len(sys.argv) > 1 else 3
z = np.load(os.path.join(ROOT, "tests", "golden", "anipose_shipped.npz"))
legs = ["RF", "LF"]
params = [_lib.leg_params_from_arrays(z[f"{l}_seg"], z[f"{l}_bounds"], z[f"{l}_seeds"]) for l in legs]
full_ang = np.stack([z[f"{l}_angles"] for l in legs])           # (2, 6000, 7)
full_pose = np.stack([z[f"{l}_pose"][:, :5] for l in legs])     # (2, 6000, 5, 3)


def windows(n_seq, n_frames):
    """n_seq windows of n_frames, every 78 frames, so that 64 windows of 1000 fit the 6000"""
    starts = [(78 * i) % (full_ang.shape[1] - n_frames + 1) for i in range(n_seq)]
    return (np.stack([full_ang[:, s:s + n_frames] for s in starts]), np.stack([full_pose[:, s:s + n_frames] for s in starts]))


def bench(name, ang, pose):
    S, L, N = ang.shape[:3]
    d_ang, d_pose = torch.from_numpy(np.ascontiguousarray(ang)).cuda(), torch.from_numpy(np.ascontiguousarray(pose)).cuda()
    out = torch.empty_like(d_ang)
    cost = torch.empty((S, L, 2), dtype=torch.float64, device="cuda")
    info = torch.empty((S, L, 3), dtype=torch.int32, device="cuda")
    need = _lib.smooth_workspace_bytes(S, L, N)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    t = timed(lambda: _lib.smooth_legs_device(d_ang.data_ptr(), d_pose.data_ptr(), S, L, N, params, out.data_ptr(), ws.data_ptr(),
                                              need, d_cost=cost.data_ptr(), d_info=info.data_ptr(), smooth=0.1, stream=st), K, 1)
    torch.cuda.synchronize()
    inf, c, q = info.cpu().numpy().reshape(-1, 3), cost.cpu().numpy().reshape(-1, 2), out.cpu().numpy()
    rounds = int((inf[:, 1] + inf[:, 2]).max())
    lb, ub = (np.stack([z[f"{l}_bounds"][:, i] for l in legs])[None, :, None] for i in (0, 1))
    jump = lambda a: float(np.abs(np.diff(a, axis=2)).max())  # noqa: E731
    print(json.dumps({"case": name, "n_seq": S, "n_legs": L, "n_frames": N, "calls": K, **t, "rounds": rounds,
                      "ms_per_round": t["ms_median"] / rounds, "launches_per_round": 6 + 2 * math.ceil(math.log2(N)),
                      "workspace_bytes": need, "accepted_steps": {"mean": float(inf[:, 1].mean()), "max": int(inf[:, 1].max())},
                      "rejected_trials": int(inf[:, 2].sum()),
                      "stop_reasons": {str(k): int(v) for k, v in enumerate(np.bincount(inf[:, 0], minlength=5)) if v},
                      "cost": {"start": float(c[:, 0].sum()), "result": float(c[:, 1].sum())},
                      "largest_change_rad": {"start": jump(np.clip(ang, lb, ub)), "result": jump(q)}}))


bench("recording", full_ang[None], full_pose[None])
bench("batch", *windows(64, 1000))
