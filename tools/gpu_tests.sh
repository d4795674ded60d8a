#!/bin/bash
# GPU tests of a file/selection with printed parity figures, then a bench run (every line: --full).
# usage: bash tools/gpu_tests.sh "<pytest selection>" [bench args]     logs go to $OUT (default: out/)
set -o pipefail
OUT=${OUT:-out}
mkdir -p $OUT
export TMPDIR=/tmp
SEL=${1:-tests}
timeout -k 10 900 python -u -m pytest $SEL -m gpu -v -s --timeout 300 --timeout-method thread -rA > $OUT/pytest_sel.log 2>&1
rc=$?
echo "pytest rc=$rc" >> $OUT/pytest_sel.log
[ $rc -le 1 ] && [ "${2:-}" != "" ] && timeout -k 10 600 python bench.py --full $2 > $OUT/bench.log 2>&1
exit $rc
