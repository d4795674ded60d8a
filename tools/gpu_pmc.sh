#!/bin/bash
# HBM traffic of the bench's kernels: two separate rocprofv3 --pmc passes over
# bench.py --full (FETCH_SIZE and WRITE_SIZE cannot share a pass on gfx950), no tracing
# domains combined with --pmc.  Summary -> $OUT/pmc/pmc_traffic.json (OUT defaults to out/
# in the repository).
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}
mkdir -p $OUT/pmc
cd /tmp
export TMPDIR=/tmp
B="$R/bench.py --full --steps 5 --warmup 1 --no-cpu --no-pmc"
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE -d $OUT/pmc/fetch -o fetch --output-format csv -- python3 $B > $OUT/pmc/fetch.log 2>&1 && \
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE -d $OUT/pmc/write -o write --output-format csv -- python3 $B > $OUT/pmc/write.log 2>&1 && \
python3 $R/tools/pmc_summary.py $(find $OUT/pmc/fetch -name '*counter_collection.csv') \
    $(find $OUT/pmc/write -name '*counter_collection.csv') $OUT/pmc/pmc_traffic.json
