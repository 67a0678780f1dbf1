#!/bin/bash
# GPU box (round 6, final tree): the whole -m gpu suite + smoke, then the default bench line
set -o pipefail
export TMPDIR=/tmp
bash tools/gpu_r6_full.sh r6final || exit 1
o=$(dirname $(ls -d */r6final/tests.log))  # where gpu_r6_full.sh wrote its logs
timeout -k 10 500 python bench.py --full > $o/bench.log 2>&1 || { tail -20 $o/bench.log; exit 1; }
tail -1 $o/bench.log | cut -c1-300
