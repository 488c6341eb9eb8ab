#!/bin/bash
# Kernel-trace stats (no counters) of the final tree: the bench with --full, and the encode leg single-stream; logs under
# $OUT/final.
set -u
cd "$(dirname "$0")/.."
fin=${OUT:-out}/final
mkdir -p "$fin"
export TMPDIR=/tmp
timeout 200 rocprofv3 --kernel-trace --stats --output-format csv -d $fin/bench -o kt -- python bench.py --full --no-cpu-baseline > $fin/bench.log 2>&1; echo "rc=$?"
tail -1 $fin/bench.log | cut -c1-300
ANCE_ENCODER_STREAMS=1 timeout 150 rocprofv3 --kernel-trace --stats --output-format csv -d $fin/encode1 -o kt -- python bench.py --full --skip-search --no-cpu-baseline --steps 2 --warmup 1 > $fin/encode1.log 2>&1; echo "rc=$?"
find $fin -name "*kernel_trace.csv" -delete
find $fin -name "*kernel_stats.csv" | head
