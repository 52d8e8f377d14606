#!/bin/bash
# Full -m gpu suite, then one bench line (no CPU baseline).
#   gpurun --timeout 1100 -- bash scripts/gpu_full.sh [bench args]
cd "$GRAFT_REPO_ROOT" || exit 1
OUT=${OUT:-out}; mkdir -p "$OUT"
timeout -k 10 700 python -u -m pytest -x -v --timeout 300 --timeout-method thread tests -m gpu \
  > $OUT/full_tests.log 2>&1
rc=$?; tail -15 $OUT/full_tests.log
[ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python bench.py --full --no-cpu-baseline "$@" > $OUT/head_bench.log 2>&1 \
  || { tail -20 $OUT/head_bench.log; exit 1; }
grep '^{' $OUT/head_bench.log | cut -c1-500
