#!/bin/bash
# One GPU visit: GPU parity tests, smoke, the full bench.  Every GPU step has its own time limit;
# a timeout / signal / crash (rc >= 124) ends the script, a plain test failure does not.
# Logs and the bench line go to $OUT (default out/gpu_check under the repository root).
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-out/gpu_check}
mkdir -p "$OUT"
export TMPDIR=/tmp
STEPS=${STEPS:-10}
fatal() { [ "$1" -ge 124 ] && { echo "fatal rc=$1 in $2"; exit "$1"; }; }
timeout -k 10 600 python -m pytest tests -m gpu -q -rs ${PYTEST_ARGS} > "$OUT/pytest_gpu.log" 2>&1
rc=$?; tail -25 "$OUT/pytest_gpu.log"; fatal $rc pytest
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1
rc=$?; tail -5 "$OUT/smoke.log"; fatal $rc smoke
timeout -k 10 600 python bench.py --full --steps $STEPS --warmup 2 ${BENCH_ARGS} > "$OUT/bench.json" 2> "$OUT/bench.err"
rc=$?; tail -5 "$OUT/bench.err"; cat "$OUT/bench.json"; fatal $rc bench
exit 0
