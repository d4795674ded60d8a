#!/bin/bash
# Build tools/build/ab_base.hsaco from the kernels of a git revision (default HEAD)
# for tools/gpu_ab.sh: the revision's kernel source, parts and headers go to tools/build/ab_base/
# for the build and are removed after it.
set -e
REV=${1:-HEAD}
cd "$(dirname "$0")/.."
BASE=tools/build/ab_base
rm -rf $BASE && mkdir -p $BASE
trap 'rm -rf $BASE' EXIT
git archive $REV mitsuba3-sunsky_amd/csrc include | tar -x -C $BASE
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 --genco -DSS_XFORM_IDENTITY -I$BASE/include -I$BASE/mitsuba3-sunsky_amd/csrc \
    -o tools/build/ab_base.hsaco $BASE/mitsuba3-sunsky_amd/csrc/sunsky_kernels.hip
