#!/bin/bash
# bench.py --step-mode full / lean / pipe on shard-of 8 and C3, two interleaved rounds
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/bench_out}; cd $R; mkdir -p $OUT
for round in 1 2; do for cfg in "--shard-of 8 --steps 30 --warmup 3" "--config C3 --steps 10 --warmup 2"; do for m in ${MODES:-full lean pipe}; do
  timeout -k 10 300 python bench.py --full --no-cpu-baseline --dropin-frames 0 $cfg --step-mode $m > $OUT/sm.log 2> $OUT/sm.err || { tail -5 $OUT/sm.err; exit 1; }
  echo "$cfg $m $(tail -1 $OUT/sm.log | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['value'], d['ms_per_step'], d['kernel_ms_per_step_rank0'], d['config'].get('chunk_spp'))")"
done; done; done
