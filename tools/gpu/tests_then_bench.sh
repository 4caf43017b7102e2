#!/bin/bash
# On the GPU machine: the -m gpu suite (or the given test files), then a short default
# bench with its CPU baseline and bandwidth probes. Output under $OUT_DIR
# (default bench_out/).
set -o pipefail
O=${OUT_DIR:-bench_out}
mkdir -p $O
ARGS=${@:-tests}
timeout -k 10 900 python -u -m pytest $ARGS -q -x --tb=short -rf --timeout 600 --timeout-method thread -m gpu \
  > $O/pytest_gpu.log 2>&1
rc=$?
tail -5 $O/pytest_gpu.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python bench.py --steps 10 --warmup 3 --full --cpu-seconds 5 > $O/bench.json 2> $O/bench.err
rc=$?
cut -c1-600 $O/bench.json
exit $rc
