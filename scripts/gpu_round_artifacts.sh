#!/bin/bash
# the bench lines committed under profiles/ for a round: the driver's command with --full, the same with --detail, and the
# --full run at the default 100 steps
set -o pipefail
R=${1:-r06}
OUT=${OUT:-bench_out}    # where the lines and records go
mkdir -p "$OUT"
python bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/${R}_bench_default_line.json 2> /dev/null && cp bench_detail.json $OUT/${R}_bench_default_detail.json || exit 1
python bench.py --gpus 1 --steps 20 --warmup 5 --detail > $OUT/${R}_bench_detail_line.json 2> /dev/null && cp bench_detail.json $OUT/${R}_bench_detail.json || exit 1
python bench.py --gpus 1 --full > $OUT/${R}_bench_k100_line.json 2> /dev/null || exit 1
cut -c1-420 $OUT/${R}_bench_default_line.json; echo; cut -c1-300 $OUT/${R}_bench_k100_line.json
