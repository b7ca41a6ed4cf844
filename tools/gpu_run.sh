#!/bin/bash
# GPU check on the GPU box (repo root): GPU tests, the bench with all its legs, the
# rocprofv3 kernel stats of the timed chain (one stream), optionally the PMC refresh.
# Results go to $OUT (SPECENH_OUT, default bench_out/ under the repo root).
#   bash tools/gpu_run.sh TAG [pmc] [pytest args...]
TAG=${1:-run}; shift
PMC=0
if [ "$1" = "pmc" ]; then PMC=1; shift; fi
R=$GRAFT_REPO_ROOT
OUT=${SPECENH_OUT:-bench_out}
cd $R && mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd)
echo "[gpu_run] pytest"
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread "$@" > "$OUT/pytest_$TAG.txt" 2>&1 || { tail -30 "$OUT/pytest_$TAG.txt"; exit 1; }
tail -2 "$OUT/pytest_$TAG.txt"
echo "[gpu_run] bench"
timeout -k 10 420 python bench.py --full --steps 20 --warmup 3 > "$OUT/bench_$TAG.json" 2> "$OUT/bench_$TAG.err" || { tail -20 "$OUT/bench_$TAG.err"; exit 1; }
python -c "import json;d=json.load(open('$OUT/bench_$TAG.json'));print(d['value'],d['ms_per_step'],d['roofline']['frac'],d['accuracy']['pass'])"
echo "[gpu_run] rocprof stats"
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_$TAG -o prof -- python3 $R/bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-stages --streams 1 > "$OUT/bench_prof_$TAG.json" 2> "$OUT/bench_prof_$TAG.err" || exit 1
mkdir -p "$OUT/prof_$TAG" && find /tmp/prof_$TAG -name '*stats.csv' -exec cp {} "$OUT/prof_$TAG/" \;
cd $R
if [ $PMC = 1 ]; then
  echo "[gpu_run] pmc"
  bash tools/pmc_refresh.sh || exit 1
fi
echo "[gpu_run] done"
