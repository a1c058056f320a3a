#!/bin/bash
# SQ / TCC counter passes on a short bench run (each pass its own rocprofv3 call)
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/bench_out}; mkdir -p $OUT; cd /tmp; export TMPDIR=/tmp
timeout -k 10 120 rocprofv3 -L > $OUT/pmc_list.txt 2>&1 || true
B="python3 $R/bench.py --full --no-cpu-baseline --steps 1 --warmup 0 --spp 8"
timeout -k 10 300 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_INSTS_LDS SQ_WAVES -d $OUT/sq1 -o sq1 --output-format csv -- $B > $OUT/sq1.log 2>&1 || { echo sq1 failed; tail -5 $OUT/sq1.log; }
timeout -k 10 300 rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum -d $OUT/tcc -o tcc --output-format csv -- $B > $OUT/tcc.log 2>&1 || { echo tcc failed; tail -5 $OUT/tcc.log; }
timeout -k 10 300 rocprofv3 --pmc SQ_INSTS_VMEM_RD SQ_INSTS_SALU SQ_INSTS_SMEM SQ_BUSY_CYCLES GRBM_GUI_ACTIVE -d $OUT/sq2 -o sq2 --output-format csv -- $B > $OUT/sq2.log 2>&1 || { echo sq2 failed; tail -5 $OUT/sq2.log; }
echo done
