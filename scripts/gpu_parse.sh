#!/bin/bash
# Parse row on the GPU: its tests, smoke, then the bench (with the parse leg) under a
# rocprofv3 kernel trace.  Usage (on the GPU box): bash scripts/gpu_parse.sh <tag>
set -u
export OUT=${OUT:-bench_out}  # where the logs and result lines go
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
TAG=${1:-parse}
mkdir -p $OUT
timeout -k 10 300 python -u -m pytest tests/test_parse.py -m gpu -v --timeout 200 --timeout-method thread \
  > $OUT/pytest_parse.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -12 $OUT/pytest_parse.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 180 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1
rc=$?; echo "smoke rc=$rc"; tail -2 $OUT/smoke.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o run \
  -- python3 bench.py --full > $OUT/bench_$TAG.log 2>&1
rc=$?; echo "bench rc=$rc"; tail -1 $OUT/bench_$TAG.log
exit $rc
