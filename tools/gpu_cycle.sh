#!/bin/bash
# GPU-box cycle: parity tests, the full bench line, kernel trace of a short bench.
# usage: [SSIP_OUT=<dir>] bash tools/gpu_cycle.sh <tag> [tests|notests]   (logs under $SSIP_OUT, default bench_out/)
set -o pipefail
tag=${1:-cycle}
out=${SSIP_OUT:-bench_out}
mkdir -p $out
export TMPDIR=/tmp
if [ "${2:-tests}" = "tests" ]; then
  timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread \
    > $out/${tag}_tests.log 2>&1 || { tail -30 $out/${tag}_tests.log; exit 1; }
  tail -2 $out/${tag}_tests.log
fi
timeout -k 10 600 python bench.py --full > $out/${tag}_bench.log 2>&1 || { tail -20 $out/${tag}_bench.log; exit 1; }
tail -1 $out/${tag}_bench.log
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $out/${tag}_prof -o run -- \
  python bench.py --full --steps 5 --warmup 3 --no-cpu-baseline > $out/${tag}_prof.log 2>&1 || { tail -20 $out/${tag}_prof.log; exit 1; }
echo cycle done
