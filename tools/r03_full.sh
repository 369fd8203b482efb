#!/bin/bash
# the whole GPU suite, then the three benches
out=${1:-runs/r03}; mkdir -p "$out"
timeout -k 10 1000 python -m pytest tests -m gpu -x -q > "$out/full_tests.log" 2>&1; echo "rc $?" >> "$out/full_tests.log"
tail -5 "$out/full_tests.log"
grep -q "rc 0" "$out/full_tests.log" || exit 1
for wl in pose3_100k pose2_100k bal1723; do
  timeout -k 10 300 python bench.py --workload $wl --full --no-cpu-baseline --no-secondary > "$out/${wl}_tree.json" 2> "$out/${wl}_tree.err"
done
python tools/bench_summary.py "$out"/*_tree.json | grep -v "^      "
