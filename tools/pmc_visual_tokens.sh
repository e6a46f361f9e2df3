#!/bin/bash
# PMC passes for the north-star kernel (visual_tokens_kernel) and its neighbours: separate --pmc runs for FETCH_SIZE and
# WRITE_SIZE (MI355X_MICROARCH.md, HBM / rocprofv3 section), kernel-trace only, each pass under its own time limit (PASS_LIMIT
# seconds, default 420); the first pass that fails ends the script.  Run on the GPU box:
#   bash tools/pmc_visual_tokens.sh gpurun_out/pmc_r02
set -e
OUT=${1:-gpurun_out/pmc}
cd "$(dirname "$0")/.."
mkdir -p "$OUT"
export TMPDIR=/tmp
for C in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 "${PASS_LIMIT:-420}" rocprofv3 --pmc $C --kernel-trace --kernel-include-regex 'visual_tokens|coord_pool|unproject_sampled' --output-format csv -d "$OUT/$C" -- \
    python3 bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-extras > "$OUT/$C.log" 2>&1
  find "$OUT/$C" -name '*counter_collection.csv' | head -1 | xargs -I{} cp {} "$OUT/${C}_counters.csv"
done
ls -la "$OUT"
