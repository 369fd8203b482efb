#!/bin/bash
# round 3: the reference's METIS ordering through the HIP path — parity tests, then ms/step beside the library's ND
set -e
out=${1:-runs/r03}; mkdir -p "$out"
python -m pytest tests/test_gpu_fullsize.py -x -q -k "metis" > "$out/metis_tests.log" 2>&1
for wl in bal1723 pose3_100k pose2_100k; do
  python bench.py --workload $wl --full --no-cpu-baseline --no-secondary > "$out/${wl}_lib.json" 2> "$out/${wl}_lib.err"
  python bench.py --workload $wl --ordering metis --full --no-cpu-baseline --no-secondary > "$out/${wl}_metis.json" 2> "$out/${wl}_metis.err"
done
python bench.py --full > "$out/default.json" 2> "$out/default.err"
tail -3 "$out/metis_tests.log"
