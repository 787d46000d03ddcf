#!/bin/bash
# Control-flow rehearsal of the multi-rank bench on a 1-GPU box: bench.py
# launches its own two ranks (bench.launch_ranks), both on device 0, over gloo
# (RCCL refuses two ranks on one device; collectives stage through host
# memory), 1M workload, with --full (its checks and extra passes have
# collectives of their own).  Checks the launcher, the barriers, the
# all-gathers and the max-over-ranks clock line up: one JSON line with n_gpus 2.
# The per-rank times are not a scaling measurement.  Outputs under $OUT
# (default profile_out/ in the repository root).
cd "$(dirname "$0")/.."; OUT=${OUT:-profile_out}; mkdir -p "$OUT"
LMI_DIST_BACKEND=gloo timeout -k 10 300 python -u bench.py --full --gpus 2 --scale 1M --steps 3 --warmup 1 \
    --no-cpu-baseline > "$OUT/two_ranks.json" 2> "$OUT/two_ranks.err"
rc=$?
echo "two-rank bench rc=$rc"; cut -c1-600 "$OUT/two_ranks.json"; grep -v amdgpu.ids "$OUT/two_ranks.err" | tail -5
exit $rc
