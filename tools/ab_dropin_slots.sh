#!/bin/bash
# lib variants on the default C3 line with its drop-in leg (queued / queued_each / sync frames), 2 rounds
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/bench_out}; mkdir -p $OUT; cd $R
for round in 1 2; do for lib in raytracingrenderer_amd/lib/ab/*.so; do
  RTG_LIB=$R/$lib timeout -k 10 300 python bench.py --full --no-cpu-baseline --steps 20 > $OUT/abd.log 2> $OUT/abd.err || { tail -5 $OUT/abd.err; exit 1; }
  echo "$(basename $lib) $(tail -1 $OUT/abd.log | python3 -c "
import json,sys
d=json.loads(sys.stdin.read()); di=d['dropin']; print(d['value'], d['ms_per_step'], 'queued', di['queued']['ms_per_frame'], 'queued_each', di['queued_each']['ms_per_frame'], 'sync', di['sync']['ms_per_frame'])")"
done; done
