#!/bin/bash
# usage: tools/build_variant.sh <name> [extra hipcc flags]: builds the working tree's library into build/abl/<name>/ (A/B timing on one box)
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
n=$1; shift
mkdir -p $R/build/abl/$n
cd $R/grok_amd/csrc
# (the library's sources: the one list of them, __graft_entry__.SOURCES)
srcs=$(cd $R && python3 -c "import __graft_entry__ as e; print(' '.join(e.SOURCES))")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function -Wno-unused-variable "$@" -shared -o $R/build/abl/$n/libgrok_amd.so \
  -x hip $srcs ../../build/source_stamp.cpp
echo built $R/build/abl/$n/libgrok_amd.so
