#!/bin/bash
# One parametrised launcher for GPU-box calls (repo root on the box). Steps run in order,
# each under its own time limit; the first failing step ends the call (no GPU work after a
# fault, abort or time-out). Results go to $OUT (SPECENH_OUT, default bench_out/).
#   bash tools/gpu.sh TAG STEP [STEP ...]
# STEP:
#   tests                   every -m gpu test
#   tests:FILE[,FILE...]    those test files (paths under tests/, -k via tests:FILE::name)
#   bench                   the bench.py --full line           -> $OUT/bench_TAG.json
#   prof                    rocprofv3 --kernel-trace --stats of the one-stream C5 chain
#                                                              -> $OUT/prof_TAG/
#   pmc                     tools/pmc_refresh.sh (PMC passes of the bench kernels)
#   py:SCRIPT[:ARGS]        python SCRIPT ARGS (ARGS: commas become spaces) -> $OUT/TAG_<name>.txt
TAG=${1:?tag}; shift
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${SPECENH_OUT:-bench_out}
cd "$R" && mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd)
for STEP in "$@"; do
  echo "[gpu.sh] $STEP"
  case "$STEP" in
    tests)
      timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread \
        > "$OUT/pytest_$TAG.txt" 2>&1 || { grep -v '^$' "$OUT/pytest_$TAG.txt" | tail -30; exit 1; }
      tail -1 "$OUT/pytest_$TAG.txt" ;;
    tests:*)
      FILES=$(echo "${STEP#tests:}" | tr ',' ' ')
      timeout -k 10 600 python -u -m pytest $FILES -x -q -s --timeout 120 --timeout-method thread \
        > "$OUT/pytest_$TAG.txt" 2>&1 || { grep -v '^$' "$OUT/pytest_$TAG.txt" | tail -30; exit 1; }
      tail -1 "$OUT/pytest_$TAG.txt" ;;
    bench)
      timeout -k 10 420 python bench.py --full --steps 20 --warmup 3 > "$OUT/bench_$TAG.json" \
        2> "$OUT/bench_$TAG.err" || { tail -20 "$OUT/bench_$TAG.err"; exit 1; }
      python -c "import json;d=json.load(open('$OUT/bench_$TAG.json'));print(d['value'],d['ms_per_step'],d['roofline']['frac'],d['accuracy']['pass'])" ;;
    prof)
      (cd /tmp && export TMPDIR=/tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats \
        --output-format csv -d /tmp/prof_$TAG -o prof -- python3 "$R/bench.py" --full --steps 10 --warmup 2 \
        --no-cpu-baseline --no-stages --streams 1 > "$OUT/bench_prof_$TAG.json" \
        2> "$OUT/bench_prof_$TAG.err") || exit 1
      mkdir -p "$OUT/prof_$TAG" && find /tmp/prof_$TAG -name '*stats.csv' -exec cp {} "$OUT/prof_$TAG/" \; ;;
    pmc)
      bash tools/pmc_refresh.sh || exit 1 ;;
    py:*)
      SPEC=${STEP#py:}
      SCRIPT=${SPEC%%:*}
      ARGS=""
      [ "$SPEC" != "$SCRIPT" ] && ARGS=$(echo "${SPEC#*:}" | tr ',' ' ')
      NAME=$(basename "$SCRIPT" .py)
      timeout -k 10 600 python -u $SCRIPT $ARGS > "$OUT/${TAG}_$NAME.txt" 2>&1 \
        || { tail -30 "$OUT/${TAG}_$NAME.txt"; exit 1; }
      tail -15 "$OUT/${TAG}_$NAME.txt" ;;
    *)
      echo "unknown step $STEP"; exit 2 ;;
  esac
done
echo "[gpu.sh] done"
