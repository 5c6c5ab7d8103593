#!/bin/bash
# dev: kernel trace (no counters) of the plain benchmark for two builds of the library, reduced by tools/value_async_trace_summary.py.
# usage: value_async_trace.sh <parent's libmodgpu.so> [output directory (default profiles)]
# Writes <out>/value_async_{parent,cand}_{kernel_stats.csv,kernel_trace.csv,trace_summary.json}: the parent through MODGPU_LIB, the candidate the tree's build.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
PARENT=${1:?the parent build of libmodgpu.so}
OUT=${2:-$R/profiles}
for who in parent cand; do
  unset MODGPU_LIB
  [ $who = parent ] && export MODGPU_LIB=$PARENT
  RAW=$(mktemp -d)
  timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $RAW -- python3 $R/bench.py --gpus 1 --steps 5 --warmup 1 > $RAW/trace.log 2>&1 || { tail -20 $RAW/trace.log; exit 1; }
  cp "$(find $RAW -name '*kernel_stats.csv' | head -1)" $OUT/value_async_${who}_kernel_stats.csv
  python3 $R/tools/value_async_trace_summary.py $RAW $OUT/value_async_$who
  rm -rf $RAW
done
