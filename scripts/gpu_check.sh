#!/bin/bash
# Record run: full GPU suite, smoke, full bench (with the CPU baseline), rocprof kernel stats and the
# per-kernel breakdown of one graph-replayed step.  usage: scripts/gpu_check.sh TAG
# Logs and profiles go to $RP_OUT_DIR (default: out/ in the repository root).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${RP_OUT_DIR:-out}
mkdir -p $OUT
export TMPDIR=/tmp
TAG=${1:-r2f}
PYT="python -u -m pytest -x -q --timeout 120 --timeout-method thread -p no:cacheprovider"
timeout -k 10 500 $PYT -m gpu tests > $OUT/${TAG}_tests.log 2>&1; rc=$?
tail -2 $OUT/${TAG}_tests.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 200 python -u -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1 || exit 1
timeout -k 10 400 python -u bench.py --full > $OUT/${TAG}_bench.log 2>&1 || exit $?
grep '^{' $OUT/${TAG}_bench.log | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print('ms/step', round(d['ms_per_step'],3), 'value', round(d['value']), 'frac', round(d['roofline']['frac'],3), 'cpu', round(d['cpu_baseline']['value'],1))"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG} -o run --output-format csv -- python bench.py --full --steps 3 --warmup 2 --no-cpu-baseline > $OUT/prof_${TAG}.log 2>&1; echo prof rc=$?
python3 scripts/stepsum.py $OUT/prof_${TAG}/run_kernel_trace.csv 4 > $OUT/${TAG}_step_kernels.txt; head -12 $OUT/${TAG}_step_kernels.txt
