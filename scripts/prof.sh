#!/bin/bash
# rocprofv3 kernel-trace stats of a short full bench run -> $RP_OUT_DIR/<tag>/ (default: out/<tag>/)
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${RP_OUT_DIR:-out}
mkdir -p $OUT
export TMPDIR=/tmp
TAG=${1:-prof}
shift
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/$TAG -o run --output-format csv -- python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline "$@" > $OUT/$TAG.log 2>&1
rc=$?
echo "prof rc=$rc"
grep '"metric"' $OUT/$TAG.log | head -1
exit $rc
