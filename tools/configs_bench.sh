#!/bin/bash
# side measurements of the other BASELINE configs (C3 is the headline bench line)
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/bench_out}; mkdir -p $OUT; cd $R
for args in "--config C2 --steps 20 --warmup 2" "--config C4 --steps 1 --warmup 1" "--config C5 --spp 32 --steps 1 --warmup 1"; do
  timeout -k 10 400 python bench.py --full --no-cpu-baseline $args > $OUT/cfg.log 2>&1 || { tail -5 $OUT/cfg.log; exit 1; }
  tail -1 $OUT/cfg.log >> $OUT/configs.jsonl
  tail -1 $OUT/cfg.log | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['config']['workload'], d['value'], d['unit'], d['ms_per_step'], 'ms/step', d['rays_per_path'], 'rays/path', d['kernel_ms_per_step_rank0'])"
done
