#!/bin/bash
# usage: tools/pipeline_timeline.sh <label> [out dir]: one rocprofv3 --kernel-trace run (no counters beside it) of the pipelined 8K
# encode (tools/prof_run.py, PROF_PIPELINE=1, 16 frames) and its timeline (tools/pipeline_timeline.py).  The library and the
# switches come from the environment (GRK_AMD_LIB, GRK_AMD_DWT_TAIL, GRK_AMD_K3_ALT).
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
label=$1; out=${2:-$R/build/timeline}
mkdir -p "$out"
tmp=$(mktemp -d)
export PROF_DECODE=0 PROF_N=16 PROF_PIPELINE=1
timeout -k 10 240 rocprofv3 --kernel-trace -d "$tmp" -o p --output-format csv -- python "$R/tools/prof_run.py" > "$tmp/run.log" 2>&1 || { tail -5 "$tmp/run.log"; exit 1; }
f=$(find "$tmp" -name "*kernel_trace.csv" | head -1)
[ -n "$f" ] || { echo "no kernel trace"; exit 1; }
cp "$f" "$out/$label.trace.csv"
python3 "$R/tools/pipeline_timeline.py" "$out/$label.trace.csv" "$label"
