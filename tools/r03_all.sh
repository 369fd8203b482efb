#!/bin/bash
# round 3: the three workloads with the library's ordering and with the reference's METIS ordering
out=${1:-runs/r03}; mkdir -p "$out"
for wl in pose3_100k pose2_100k bal1723; do
  for ord in lib metis; do
    extra=""; [ $ord = metis ] && extra="--ordering metis"
    timeout -k 10 300 python bench.py --workload $wl --full --no-cpu-baseline --no-secondary $extra > "$out/${wl}_${ord}_now.json" 2> "$out/${wl}_${ord}_now.err" || tail -3 "$out/${wl}_${ord}_now.err"
  done
done
python tools/bench_summary.py "$out"/*_now.json | grep -v "^      "
