#!/bin/bash
# parent, branch, parent, ... in fresh processes on one otherwise idle card: bash profiles/dev/ab_lm_loop.sh [runs per side] [out.jsonl]
# ${OLD:-ab_old}: a copy of the parent commit's wildcat-slam_amd/, include/ and bench.py with its libraries built.
# Then: python profiles/dev/ab_lm_loop.py summarize out.jsonl > profiles/lm_loop_ab.json
set -u -o pipefail
N=${1:-6}
OUT=${2:-lm_loop_ab.jsonl}
: > "$OUT"
for rep in $(seq "$N"); do
  for side in parent branch; do
    tree=.
    [ $side = parent ] && tree=${OLD:-ab_old}
    line=$(timeout -k 10 240 python profiles/dev/ab_lm_loop.py run $tree | grep '^{' | tail -1) || { echo "run $rep ($side) failed" >&2; exit 1; }
    echo "{\"side\": \"$side\", ${line#\{}" | tee -a "$OUT"
  done
done
