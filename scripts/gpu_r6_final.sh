#!/bin/bash
# Round-6 evidence in one call: the full -m gpu suite, the default bench line (CPU baseline,
# live PMC traffic + rocprofv3 trace average of the dominant kernel), the profiled bench +
# rocprofv3 kernel trace / stats + step breakdown, the bf16-operand and 256x512 lines.
#   gpurun --timeout 1200 -- bash scripts/gpu_r6_final.sh TAG
cd "$GRAFT_REPO_ROOT" || exit 1
TAG=${1:-r6f}
OUT=${OUT:-out}; mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 600 python -u -m pytest -q --timeout 300 --timeout-method thread tests -m gpu \
  > $OUT/${TAG}_tests.log 2>&1 || { tail -30 $OUT/${TAG}_tests.log; exit 1; }
tail -2 $OUT/${TAG}_tests.log
timeout -k 10 600 python bench.py --full > $OUT/${TAG}_bench_default.log 2>&1 \
  || { tail -20 $OUT/${TAG}_bench_default.log; exit 1; }
grep '^{' $OUT/${TAG}_bench_default.log | cut -c1-300
bash scripts/gpu_bench_prof.sh $TAG || exit 1
for v in "bf16::--dtype bf16" "256x512::--height 256 --width 512 --batch 2" \
         "bf16_256x512::--dtype bf16 --height 256 --width 512 --batch 2"; do
  name=${v%%::*}; args=${v#*::}
  timeout -k 10 400 python bench.py --full --no-cpu-baseline $args \
    --profile-json $OUT/${TAG}_profile_${name}.json > $OUT/${TAG}_bench_${name}.log 2>&1 \
    || { tail -20 $OUT/${TAG}_bench_${name}.log; exit 1; }
  grep '^{' $OUT/${TAG}_bench_${name}.log | cut -c1-200
done
