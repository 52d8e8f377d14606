#!/bin/bash
# bench.py (live per-family profile) and a rocprofv3 kernel-trace of the same command.
#   gpurun --timeout 900 -- bash scripts/gpu_bench_prof.sh TAG
cd "$GRAFT_REPO_ROOT" || exit 1
TAG=${1:-bp}
OUT=${OUT:-out}; mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 400 python bench.py --full --no-cpu-baseline --profile-json $OUT/${TAG}_profile.json \
  > $OUT/${TAG}_bench.log 2>&1 || { tail -20 $OUT/${TAG}_bench.log; exit 1; }
grep '^{' $OUT/${TAG}_bench.log | cut -c1-600
timeout -k 10 500 rocprofv3 --kernel-trace --stats -f csv -d $OUT/${TAG}_prof -o run -- \
  python bench.py --full --no-cpu-baseline --profile-json $OUT/${TAG}_profile_rp.json \
  > $OUT/${TAG}_bench_rp.log 2>&1 || { tail -20 $OUT/${TAG}_bench_rp.log; exit 1; }
CSV=$(find $OUT/${TAG}_prof -name '*kernel_trace.csv' | head -1)
# the 8 last graph-replayed timed steps (bench.py's 3 eager roofline steps come after them)
python vae-2_amd/tools/trace_steps.py "$CSV" --steps 8 --skip 3 --json $OUT/${TAG}_steps.json \
  > $OUT/${TAG}_steps.txt 2>&1
head -40 $OUT/${TAG}_steps.txt
