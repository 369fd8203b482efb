#!/usr/bin/env python3
"""Where the time of gsx_lago_initialize goes, beside the LM iteration of the same graph on the same build.

    python tools/lago_probe.py [--poses 100000] [--reps 5] [--warmup 2] [--mst] [--out FILE.json]

Runs lago on the synthetic pose2 graph of bench.py (datasets.synth_manhattan_pose2, seed 42; the reader-style prior is on
its first pose) and prints one JSON line: per stage the median over the repetitions of the times the library keeps for its
last call (gsx_lago_timings: HIP events on the internal handles' streams for the device stages, a host clock for the two
analyses), the wall time of the whole call (a host clock around a call that ends synchronised), and ms per LM trial of the
same graph measured as bench.py measures it.  Every shape is warmed up first; a tracing profiler must not be attached
(end-to-end numbers).
Without a GPU the tool only builds the graph and its tree (--host-only does the same where there is one)."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gtsam_petercdev_amd import _abi as A, _lib, datasets  # noqa: E402


def timed_runs(call, reps, warmup):
    for _ in range(warmup):
        call()
    wall, stages = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append(1e3 * (time.perf_counter() - t0))
        stages.append(_lib.lago_timings())
    out = {k: statistics.median(s[k] for s in stages) for k in stages[0]}
    out["whole_call_wall_ms"] = statistics.median(wall)
    out["whole_call_wall_ms_min_max"] = [min(wall), max(wall)]
    return out


def lm_ms_per_trial(arr, steps, warmup, lam=1e-5):
    be = _lib.product_backend(arr)
    be.set_ordering(be.compute_ordering(A.ORDER_ND))
    be.set_profiling(-1)
    for _ in range(warmup):
        be.lm_trial(True, lam, False)
    be.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        be.lm_trial(True, lam, False)
    be.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    be.close()
    return ms


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mst", action="store_true", help="findMinimumSpanningTree instead of the odometric path")
    ap.add_argument("--lm-steps", type=int, default=20)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    arr = datasets.synth_manhattan_pose2(args.poses, seed=42)
    odometric = not args.mst
    t0 = time.perf_counter()
    s = _lib.lago_structure(arr, odometric)
    out = {"workload": f"pose2_{args.poses}", "tree": "odometric" if odometric else "mst", "n_poses": arr.n_vars,
           "n_factors": arr.n_factors, "n_edges": int(s["edge_from"].size), "n_tree_edges": int(s["tree_ids"].size),
           "n_chords": int(s["chord_ids"].size), "max_depth": s["max_depth"],
           "rounds": int(math.ceil(math.log2(s["max_depth"] + 1))), "structure_host_ms": 1e3 * (time.perf_counter() - t0)}
    if args.host_only or _lib.device_count() == 0:
        out["device"] = None
        print(json.dumps(out))
        return out
    out["lago"] = timed_runs(lambda: _lib.lago_initialize(arr, odometric), args.reps, args.warmup)
    out["lm_ms_per_trial"] = lm_ms_per_trial(arr, args.lm_steps, 3)
    init = _lib.lago_initialize(arr, odometric)
    be = _lib.product_backend(arr)
    out["error_of_the_graphs_own_values"] = be.error()
    be.set_values(init)
    out["error_after_lago"] = be.error()
    be.close()
    assert np.all(np.isfinite(init))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return out


if __name__ == "__main__":
    main()
