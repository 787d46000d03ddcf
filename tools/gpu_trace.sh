#!/bin/bash
# GPU parity suite, a short bench, and a kernel trace of the bench (--full: every pass) summarised
# per kernel.  Outputs under $OUT (default profile_out/ in the repository root).
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${OUT:-profile_out}
mkdir -p "$OUT"
[ -n "$TRACE_ONLY" ] || bash tools/gpu_quick.sh || exit $?
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/tr" -o run -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > "$OUT/tr.log" 2>&1
rc=$?; echo "trace rc=$rc"
if [ $rc -ne 0 ]; then tail -5 "$OUT/tr.log"; exit $rc; fi
python3 tools/trace_summary.py $(find "$OUT/tr" -name "run_kernel_trace.csv" | head -1) | tee "$OUT/tr_summary.txt"
