#!/usr/bin/env python3
"""TEST INFRASTRUCTURE -- bound, IN ISSUE CYCLES, of running stages 2 and 3 of the lane-per-chain kernel as ONE pass loop.

Stages 2 and 3 instantiate the same code (two active joints, axes Z and Y, full rank); today a wavefront finishes stage 2
for all its 64 chains -- tail of ever fewer active lanes included -- before any lane starts stage 3.  Merged, a lane that has
walked its frames in stage 2 goes straight on to its stage-3 frames: one tail instead of two.  Which chain a lane walks does
not change, so this is the only schedule of that kind the chain queue (tests/tools/queue_bound.py) does not cover.

Model: queue_bound.py's.  A lane's passes per stage from the oracle's evaluation counts on the benchmark data; the cost of
one wave pass from the measured block shares and entry counts (profiles/r03_block_entries_*.json): a pass costs the union
of its lanes' paths.  In the merged loop a pass has n2 lanes still in stage 2 and n3 already in stage 3; block b is entered
with probability 1 - (1 - q2_b)^n2 (1 - q3_b)^n3 and costs the lane-weighted mean of the two stages' cycles per entry.
NOT counted: what the merge would add -- a second general start evaluation (first frame of stage 3) that lanes reach one
at a time instead of all at once (up to 64 one-lane start evaluations per wavefront), and run-time instead of compile-time
angle columns / hand-off offsets.  The figure is therefore an upper bound of the gain.

    python tests/tools/stage23_merge_bound.py [n_seq]          (CPU, ~1 min; default 1024 sequences per variant)
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from queue_bound import BLOCKS, ROOT, cost_model, lane_passes, pass_cost, wave_cost_now  # noqa: E402


def named_model(entries_json, stage):
    """cost_model's (q, cycles per entry) pairs under their block names"""
    names = [b for b in BLOCKS if b in entries_json["stages"][str(stage)]["share"]]
    return dict(zip(names, cost_model(entries_json, stage)))


def wave_cost_merged(m2, m3, p2, p3):
    """p2, p3: (64,) lane pass counts of one wave in stages 2 and 3 -> (wave passes, cost) of the merged loop"""
    life = int((p2 + p3).max())
    t = np.arange(life)[:, None]
    n2 = (p2[None, :] > t).sum(1).astype(np.float64)
    n3 = ((p2[None, :] <= t) & (p2[None, :] + p3[None, :] > t)).sum(1).astype(np.float64)
    cost = 0.0
    for b in set(m2) | set(m3):
        q2, c2 = m2.get(b, (0.0, 0.0))
        q3, c3 = m3.get(b, (0.0, 0.0))
        enter = 1.0 - (1.0 - q2) ** n2 * (1.0 - q3) ** n3
        cost += float((enter * (n2 * c2 + n3 * c3) / np.maximum(n2 + n3, 1.0)).sum())
    return life, cost


def main():
    n_seq = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    res = {"what": __doc__.split("\n\n")[0].replace("\n", " "),
           "sample": f"{n_seq} sequences x 6 legs x 64 frames per variant (the benchmark's generator and seeds)"}
    for variant in ("iid", "smooth"):
        ej = json.load(open(os.path.join(ROOT, "profiles", f"r03_block_entries_{variant}.json")))
        p = lane_passes(variant, n_seq)   # (L, S, 4)
        plain = {s: cost_model(ej, s) for s in (1, 2, 3, 4)}
        m2, m3 = named_model(ej, 2), named_model(ej, 3)
        now = {s: 0.0 for s in (1, 2, 3, 4)}
        merged = passes_now = passes_merged = 0.0
        for li in range(p.shape[0]):
            for w0 in range(0, n_seq - 63, 64):
                w = p[li, w0:w0 + 64]
                for s in (1, 2, 3, 4):
                    life, c = wave_cost_now(plain[s], w[:, s - 1])
                    now[s] += c
                    if s in (2, 3):
                        passes_now += life
                life, c = wave_cost_merged(m2, m3, w[:, 1], w[:, 2])
                merged += c
                passes_merged += life
        total = sum(now.values())
        res[variant] = {"cycles_now_by_stage": now, "cycles_stages_2_3_now": now[2] + now[3], "cycles_stages_2_3_merged": merged,
                        "wave_passes_stages_2_3_now": passes_now, "wave_passes_stages_2_3_merged": passes_merged,
                        "merged_vs_now_stages_2_3": merged / (now[2] + now[3]),
                        "merged_vs_now_all_stages": (total - now[2] - now[3] + merged) / total,
                        # the model's own check: a merged loop of lanes that all finish stage 2 together is today's schedule
                        "full_pass_cost": {s: float(pass_cost(plain[s], 64)) for s in (2, 3)}}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
