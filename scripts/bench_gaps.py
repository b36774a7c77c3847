"""Skip mode for missing key points (include/seqik_gaps.h): compaction and expansion kernels, HIP-event timed.

One JSON line.  For two shapes -- many short chains (15625 recordings x 6 legs x 64 frames, config 3) and few long ones
(1 recording x 6 legs x 1 M frames) -- and 0 %, 5 % and 50 % missing leg-frames (a NaN in key point 2):
  compact  seqik_gaps_compact_device: pose in (120 B), compacted pose (120 B) and map (4 B) out per leg-frame
  expand   seqik_gaps_expand_device of angles + FK: map (4 B) and compact angles / FK (56 + 216 B) in, 272 B out
each against a device-to-device copy of the same algorithmic bytes timed in the same process.  Then a whole solve at
config-3 size with nothing missing: solve_seq_device against compact -> solve_seq_device -> expand (dense layout, serial
walk, FK on), the cost of skip mode when the data has no gaps.
Usage: python scripts/bench_gaps.py [launches]"""
import json, sys
import torch
import bench_common
from seqikpy_amd import _lib
from bench_support import make_workload

K = int(sys.argv[1]) if len(sys.argv) > 1 else 20
L = 6
SHAPES = {"short_chains": (15625, 64), "long_chains": (1, 1_000_000)}
FRACTIONS = (0.0, 0.05, 0.5)
st = torch.cuda.current_stream().cuda_stream


def timed(fn, k=K):
    return bench_common.timed(fn, k, 3)


def copy_bar(nbytes):
    bar = bench_common.copy_bar(nbytes, K, 3)
    del bar["GBps_median"]
    return bar


def rate(t, nbytes, bar):
    gbps = nbytes / t["ms"] / 1e6
    return dict(t, algorithmic_bytes=nbytes, GBps=gbps, rate_vs_copy=gbps / bar["GBps"])


_, _, pose0, params = make_workload(4, 64, "iid", 11)
legs = params
out = {"kernels": ["seqik_gaps_count_kernel", "seqik_gaps_scan_kernel", "seqik_gaps_permute_kernel",
                   "seqik_gaps_pad_kernel", "seqik_gaps_expand_kernel<4>"], "launches": K}
g = torch.Generator(device="cuda").manual_seed(5)
for shape, (S, N) in SHAPES.items():
    n = S * L * N
    pose = torch.randn((S, L, N, 5, 3), dtype=torch.float64, device="cuda", generator=g)
    cpose = torch.empty_like(pose)
    mp = torch.empty((S, L, N), dtype=torch.int32, device="cuda")
    nv = torch.empty((S, L), dtype=torch.int32, device="cuda")
    cang = torch.randn((S, L, N, 7), dtype=torch.float64, device="cuda", generator=g)
    cfk = torch.randn((S, L, N, 9, 3), dtype=torch.float64, device="cuda", generator=g)
    ang, fk = torch.empty_like(cang), torch.empty_like(cfk)
    b_compact, b_expand = n * (120 + 120 + 4), n * (4 + 56 + 216 + 56 + 216)
    row = {"n_seq": S, "n_legs": L, "n_frames": N, "leg_frames": n,
           "copy_bar_compact": copy_bar(b_compact // 2), "copy_bar_expand": copy_bar(b_expand // 2)}
    clean = pose[..., 2, 1].clone()
    for frac in FRACTIONS:
        hit = torch.rand((S, L, N), device="cuda", generator=g) < frac
        pose[..., 2, 1] = torch.where(hit, torch.full_like(clean, float("nan")), clean)
        tc = timed(lambda: _lib.gaps_compact_device(pose, S, L, N, legs, cpose, mp, nv, stream=st))
        te = timed(lambda: _lib.gaps_expand_device(mp, S, L, N, cang, ang, cfk, fk, stream=st))
        torch.cuda.synchronize()
        row[f"missing_{int(round(frac * 100))}pct"] = {
            "missing_leg_frames": int(hit.sum().item()), "n_valid_total": int(nv.sum().item()),
            "compact": rate(tc, b_compact, row["copy_bar_compact"]), "expand": rate(te, b_expand, row["copy_bar_expand"])}
    out[shape] = row
    del pose, cpose, mp, nv, cang, cfk, ang, fk
    torch.cuda.empty_cache()

# whole solve at config-3 size, nothing missing: plain solve_seq_device vs the skip-mode composition
S, N = SHAPES["short_chains"]
_, _, pose_np, params = make_workload(S, N, "iid", 7)
pose = torch.from_numpy(pose_np).cuda()
bufs = dict(d_angles=torch.empty((S, L, N, 7), dtype=torch.float64, device="cuda"),
            d_cpose=torch.empty_like(pose), d_map=torch.empty((S, L, N), dtype=torch.int32, device="cuda"),
            d_n_valid=torch.empty((S, L), dtype=torch.int32, device="cuda"),
            d_cangles=torch.empty((S, L, N, 7), dtype=torch.float64, device="cuda"),
            d_fk=torch.empty((S, L, N, 9, 3), dtype=torch.float64, device="cuda"),
            d_cfk=torch.empty((S, L, N, 9, 3), dtype=torch.float64, device="cuda"))
k_solve = max(3, K // 4)
plain = timed(lambda: _lib.solve_seq_device(pose.data_ptr(), S, L, N, params, bufs["d_angles"].data_ptr(),
                                            bufs["d_fk"].data_ptr(), stream=st), k_solve)
skip = timed(lambda: _lib.solve_seq_gaps_device(pose, S, L, N, params, stream=st, **bufs), k_solve)
torch.cuda.synchronize()
ref = torch.empty_like(bufs["d_angles"])
_lib.solve_seq_device(pose.data_ptr(), S, L, N, params, ref.data_ptr(), bufs["d_cfk"].data_ptr(), stream=st)
torch.cuda.synchronize()
out["solve_config3_no_gaps"] = {"n_seq": S, "n_legs": L, "n_frames": N, "layout": "dense", "frame_chunk": 0,
                                "plain": plain, "skip": skip, "overhead": skip["ms"] / plain["ms"] - 1.0,
                                "bit_identical": bool(torch.equal(ref, bufs["d_angles"]))}
print(json.dumps(out))
