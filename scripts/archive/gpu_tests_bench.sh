#!/bin/bash
# Selected GPU tests (pytest -k expression), then one bench line.
#   gpurun -- bash scripts/gpu_tests_bench.sh "fuse_sum or pow2" [bench args]
cd "$GRAFT_REPO_ROOT" || exit 1
OUT=${OUT:-out}; mkdir -p "$OUT"
K=${1:-"fuse_sum"}
shift
timeout -k 10 600 python -u -m pytest -x -v --timeout 300 --timeout-method thread tests -m gpu \
  -k "$K" > $OUT/gtb.log 2>&1
rc=$?; tail -30 $OUT/gtb.log
[ $rc -ne 0 ] && exit $rc
timeout -k 10 400 python bench.py --full --no-cpu-baseline "$@" > $OUT/gtb_bench.log 2>&1 \
  || { tail -20 $OUT/gtb_bench.log; exit 1; }
grep '^{' $OUT/gtb_bench.log | cut -c1-400
