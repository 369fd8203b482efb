#!/usr/bin/env python3
"""Where the time of the translation-averaging stage goes: the batched MFAS kernel over a sweep of (directions, nodes), and
one TranslationRecovery run.

    python tools/translation_probe.py [--dirs 1,48,1024] [--nodes 64,1000,8192] [--reps 5] [--warmup 2] [--out FILE.json]

Random graphs of average degree 6 with noisy directions (seed 42).  Prints one JSON line: per (D, n) the median over the
repetitions of the stage times the library keeps for its last call (gsx_mfas_timings: HIP events for the two kernels, a host
clock for the adjacency and for the whole call) and the wall time of the whole call; then the wall time of one
gsx_translation_recovery on a 200-node graph with its LM iteration count.  Every shape is warmed up first; a tracing profiler
must not be attached (end-to-end numbers).  Without a GPU the tool only builds the inputs."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gtsam_petercdev_amd import _abi as A, _lib  # noqa: E402


def random_edges(n, rng, noise=0.02):
    pos = rng.uniform(-10, 10, (n, 3))
    pairs = {(i, (i + 1) % n) if i < (i + 1) % n else ((i + 1) % n, i) for i in range(n)}
    while len(pairs) < 3 * n:
        a, b = (int(x) for x in rng.integers(0, n, 2))
        if a != b:
            pairs.add((a, b) if a < b else (b, a))
    pairs = sorted(pairs)
    d = np.array([pos[b] - pos[a] for a, b in pairs])
    d = d / np.linalg.norm(d, axis=1, keepdims=True) + rng.normal(0, noise, (len(pairs), 3))
    return pos, np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs]), d / np.linalg.norm(d, axis=1, keepdims=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--dirs", default="1,48,1024")
    ap.add_argument("--nodes", default="64,1000,8192")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    args = ap.parse_args(argv)
    rng = np.random.default_rng(42)
    have_gpu = _lib.device_count() > 0
    out = dict(tool="translation_probe", gpu=have_gpu, mfas=[], mfas_timing_names=list(_lib.MFAS_TIMING_NAMES))
    for n in (int(x) for x in args.nodes.split(",")):
        _, k1, k2, dirs = random_edges(n, rng)
        for D in (int(x) for x in args.dirs.split(",")):
            proj = rng.normal(0, 1, (D, 3))
            proj /= np.linalg.norm(proj, axis=1, keepdims=True)
            row = dict(n_dirs=D, n_nodes=n, n_edges=int(k1.size))
            if have_gpu:
                call = lambda: _lib.mfas_outlier_weights(k1, k2, edge_dirs=dirs, proj_dirs=proj, want_weights=False)
                for _ in range(args.warmup):
                    call()
                wall, stages = [], []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    call()
                    wall.append(1e3 * (time.perf_counter() - t0))
                    stages.append(_lib.mfas_timings())
                row.update({k: statistics.median(s[k] for s in stages) for k in stages[0]})
                row["whole_call_wall_ms"] = statistics.median(wall)
            out["mfas"].append(row)
    pos, k1, k2, dirs = random_edges(200, rng, noise=0.005)
    unit = [(int(a), int(b), z, A.NOISE_ISOTROPIC, [0.01]) for a, b, z in zip(k1, k2, dirs)]
    rec = dict(n_nodes=200, n_edges=len(unit))
    if have_gpu:
        wall = []
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            _, r = _lib.translation_recovery(unit)
            if i >= args.warmup:
                wall.append(1e3 * (time.perf_counter() - t0))
        rec.update(whole_call_wall_ms=statistics.median(wall), lm_iterations=r["iterations"], final_error=r["final_error"])
    out["recovery"] = rec
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
