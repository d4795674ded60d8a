#!/bin/bash
# Full GPU check: every -m gpu test (one process, per-test timeout), smoke, bench --full.
# Steps chained with &&; each under its own time limit.  Logs go to $OUT (default: out/).
set -o pipefail
OUT=${OUT:-out}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 1200 python -u -m pytest tests -m gpu -x -v -s --timeout 300 --timeout-method thread -rs > $OUT/pytest_gpu.log 2>&1 && \
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 && \
timeout -k 10 600 python bench.py --full ${BENCH_ARGS:---steps 30 --warmup 5} > $OUT/bench.log 2>&1
