#!/bin/bash
# per-dispatch kernel times of one bench run (rocprofv3 kernel trace) -> $OUT/kq/
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/bench_out}; mkdir -p $OUT; cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace -d $OUT/kq -o kq --output-format csv -- python3 $R/bench.py --full --no-cpu-baseline --steps 1 --warmup 1 $BENCH_ARGS > $OUT/kq.log 2>&1
