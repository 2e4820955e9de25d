#!/bin/bash
# The N=1 headline run with every secondary block (bench.py --full, other flags at their
# defaults: the log_fresh, log_wrapped, log_pressured and log_overfull blocks).
set -o pipefail
OUT=gpurun_out/${1:-bench_default}
mkdir -p "$OUT"
timeout -k 10 600 python -u bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err" \
  || { echo "bench failed"; tail -30 "$OUT/bench.err"; exit 1; }
cut -c1-3000 "$OUT/bench.json"
