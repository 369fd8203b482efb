#!/bin/bash
# round 3: subtree-fused elimination (front_tree_kernel) — parity, then ms/step
set -e
out=${1:-runs/r03}; mkdir -p "$out"
timeout -k 10 900 python -m pytest tests/test_gpu_parity.py tests/test_gpu_fullsize.py tests/test_gpu_boundary.py -x -q > "$out/tree_tests.log" 2>&1 || { tail -30 "$out/tree_tests.log"; exit 1; }
tail -3 "$out/tree_tests.log"
for wl in pose3_100k pose2_100k bal1723; do
  timeout -k 10 300 python bench.py --workload $wl --full --no-cpu-baseline --no-secondary > "$out/${wl}_tree.json" 2> "$out/${wl}_tree.err"
done
