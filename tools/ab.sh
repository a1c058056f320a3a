#!/bin/bash
# A/B: bench each lib variant in raytracingrenderer_amd/lib/ab (interleaved, 2 rounds)
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/bench_out}; mkdir -p $OUT; cd $R
for round in 1 2; do
for lib in raytracingrenderer_amd/lib/ab/*.so; do
  RTG_LIB=$R/$lib timeout -k 10 300 python bench.py --full --no-cpu-baseline --steps 3 $BENCH_ARGS > $OUT/ab.log 2>&1 || { tail -5 $OUT/ab.log; exit 1; }
  echo "$(basename $lib) $(tail -1 $OUT/ab.log | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['value'], d['kernel_ms_per_step_rank0'])")"
done; done
