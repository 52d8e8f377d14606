#!/bin/bash
# bf16-operand and 256x512 lines at the final round-5 HEAD.
cd "$GRAFT_REPO_ROOT" || exit 1
TAG=r5k
OUT=${OUT:-out}; mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 300 python bench.py --full --no-cpu-baseline --dtype bf16 \
  --profile-json $OUT/${TAG}_profile_bf16.json > $OUT/${TAG}_bench_bf16.log 2>&1 \
  || { tail -20 $OUT/${TAG}_bench_bf16.log; exit 1; }
grep '^{' $OUT/${TAG}_bench_bf16.log | cut -c1-200
timeout -k 10 300 python bench.py --full --no-cpu-baseline --height 256 --width 512 --batch 2 \
  > $OUT/${TAG}_bench_256x512.log 2>&1 || { tail -20 $OUT/${TAG}_bench_256x512.log; exit 1; }
grep '^{' $OUT/${TAG}_bench_256x512.log | cut -c1-200
timeout -k 10 300 python bench.py --full --no-cpu-baseline --dtype bf16 --height 256 --width 512 --batch 2 \
  > $OUT/${TAG}_bench_bf16_256x512.log 2>&1 || { tail -20 $OUT/${TAG}_bench_bf16_256x512.log; exit 1; }
grep '^{' $OUT/${TAG}_bench_bf16_256x512.log | cut -c1-200
