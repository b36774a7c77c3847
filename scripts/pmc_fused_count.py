#!/usr/bin/env python3
"""Wave-level VALU instructions of ONE launch of seqik_fused_kernel<true> on the benchmark batch (15 625 sequences x 6 legs x
64 frames, the seeds of bench.py), iid and smooth -- the deterministic count of EXPERIMENTS.md 16.1.

    rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_VALU_TRANS_F64 --output-format csv -d OUT -- python scripts/pmc_fused_count.py run [CACHE_DIR]
    python scripts/pmc_fused_count.py read OUT [OUT2 ...]        # -> one JSON line per directory

`run` makes one launch per variant, iid first (counters-only profiler run of its own: no tracing beside it); `read` takes
the fused kernel's dispatches of such a run in dispatch order.  Where the run also collected SQ_INSTS_VALU_TRANS_F64 (the
v_rcp_f64 / v_rsq_f64 / v_sqrt_f64 seeds of every division and square root), `read` adds the WEIGHTED count
W = VALU + 2.8 x TRANS_F64: a transcendental issues in 16.2 cycles where every other FP64 instruction takes 4.2-4.3
(profiles/r03_valu_issue_costs.json, 3 waves per SIMD), so it stands for 16.2 / 4.25 = 3.8 ordinary instructions, 2.8 more
than the plain count gives it.  CACHE_DIR keeps the generated key points (0.75 GB per
variant) for the next build's run.  SEQIK_LIB selects the library (A/B builds).  The count is a
property of the code and the data: it does not vary from run to run, unlike a time."""
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sequential-inverse-kinematics_amd"))
sys.path.insert(0, ROOT)
VARIANTS = ("iid", "smooth")
COUNTERS = ("SQ_INSTS_VALU", "SQ_INSTS_VALU_TRANS_F64")
TRANS_EXTRA = 2.8   # 16.2 / 4.25 - 1: issue cycles of v_rcp_f64 / v_rsq_f64 over those of an FP64 add / multiply / FMA, less the one counted


def run(cache=None):
    import numpy as np
    import torch
    import bench_support as bs
    from seqikpy_amd import _lib, synthetic
    S, T = 15625, 64
    for variant in VARIANTS:
        kept = os.path.join(cache, f"pmc_fused_count_{variant}.npy") if cache else None
        if kept and os.path.exists(kept):
            legs, body, _, params = bs.make_workload(1, T, variant, synthetic.SEED_BASE)
            pose = np.load(kept)
        else:
            legs, body, pose, params = bs.make_workload(S, T, variant, synthetic.SEED_BASE)
            if kept:
                np.save(kept, pose)
        d_pose = torch.from_numpy(np.ascontiguousarray(pose.transpose(0, 1, 3, 2, 4))).cuda()
        d_ang = torch.zeros((S, len(legs), 7, T), dtype=torch.float64, device="cuda")
        d_fk = torch.zeros((S, len(legs), T, 9, 3), dtype=torch.float64, device="cuda")
        _lib.solve_seq_device(d_pose.data_ptr(), S, len(legs), T, params, d_ang.data_ptr(), d_fk.data_ptr(),
                              layout=_lib.planar_layout(T))
        torch.cuda.synchronize()
        print(json.dumps({"variant": variant, "units": S * len(legs) * T, "angles_sum": float(d_ang.sum().item()),
                          "fk_sum": float(d_fk.sum().item())}), flush=True)


def read(dirs):
    for d in dirs:
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            rows += [r for r in csv.DictReader(open(f)) if "seqik_fused_kernel" in r["Kernel_Name"] and r["Counter_Name"] in COUNTERS]
        per_dispatch, trans = {}, {}
        for r in rows:
            acc = per_dispatch if r["Counter_Name"] == "SQ_INSTS_VALU" else trans
            acc[int(r["Dispatch_Id"])] = acc.get(int(r["Dispatch_Id"]), 0.0) + float(r["Counter_Value"])
        out = {"dir": os.path.basename(os.path.normpath(d)), "launches": len(per_dispatch)}
        for variant, k in zip(VARIANTS, sorted(per_dispatch)):
            out[f"{variant}_valu_insts_per_launch"] = per_dispatch[k]
            if k in trans:
                out[f"{variant}_f64_trans_insts_per_launch"] = trans[k]
                out[f"{variant}_weighted_insts_per_launch"] = per_dispatch[k] + TRANS_EXTRA * trans[k]
        print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run(sys.argv[2] if len(sys.argv) > 2 else None)
    elif len(sys.argv) >= 3 and sys.argv[1] == "read":
        read(sys.argv[2:])
    else:
        sys.exit(__doc__)
