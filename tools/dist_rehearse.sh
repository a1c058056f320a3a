#!/bin/bash
# N=2 rehearsal of bench.py's multi-rank path on a one-GPU box: two ranks share cuda:0, gloo for
# the film reduce; rank 0 checks the reduced film against a solo render of every tile.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/bench_out}; mkdir -p $OUT; cd $R
RTG_DIST_BACKEND=gloo timeout -k 10 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 \
  --master-addr 127.0.0.1 --master-port 29517 bench.py --full --gpus 2 --steps 1 --warmup 0 --spp 8 --no-cpu-baseline \
  --verify-film > $OUT/dist2.log 2>&1 || { tail -30 $OUT/dist2.log; exit 1; }
grep '^{' $OUT/dist2.log | tail -1
