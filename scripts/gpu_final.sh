#!/bin/bash
# Round-end check of the committed tree, as the driver runs it: the whole -m gpu suite,
# smoke(), the default bench line.
set -u
export OUT=${OUT:-bench_out}  # where the logs and result lines go
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
TAG=${1:-final}
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread \
  > $OUT/pytest_$TAG.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -2 $OUT/pytest_$TAG.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" || exit $?
timeout -k 10 240 python -u bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || exit $?
python3 -c "
import json;d=json.load(open('$OUT/bench_$TAG.json'))
print('step', d['ms_per_step'], 'value %.4g'%d['value'], 'roofline', d['roofline']['frac'], 'traffic', d['roofline']['traffic'], 'keyed', d['keyed']['roofline']['frac'], 'qty', d['parse']['quantity']['roofline']['frac'], 'cpu', d['cpu_baseline']['value'], d['cpu_baseline']['match'], 'chk', d['totals_checksum'])"
