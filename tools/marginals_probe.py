"""Time the all-variables marginal pass (gsx_marginal_covariances) against the per-variable loop it replaces, on the bench
shapes as bench.py builds them.

  (a) one gsx_marginal_covariances(NULL) after a warm call, factorization resident: median of --reps calls;
  (b) gsx_marginal_covariance on --keys seeded keys, extrapolated by n_vars / keys.

Appends one JSON record per workload to --out (default runs/all_marginals_probe.json): both times, the bytes of the
covariance arena and the per-kernel times of one profiled pass (gsx_set_profiling(1) / gsx_kernel_time).

  python tools/marginals_probe.py --workload pose3_100k
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ["all_marginals", "marg_prep", "marg_kt", "marg_sf", "marg_ff", "marg_emit", "marg_leaf"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", required=True, choices=["bal1723", "bal49", "pose3_100k", "pose2_100k"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--keys", type=int, default=200)
    ap.add_argument("--one-pass-only", action="store_true", help="one warm pass and nothing else (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "runs", "all_marginals_probe.json"))
    args = ap.parse_args()
    import bench
    from gtsam_petercdev_amd import _abi as A, _lib
    arrays, order_name = bench.make_problem(args.workload, 42)
    be = _lib.product_backend(arrays)
    kind = {"schur_nd": A.ORDER_SCHUR_ND, "nd": A.ORDER_ND}[order_name]
    be.set_ordering(be.compute_ordering(kind))
    be.linearize()
    parent, fronts = be.get_tree()
    cls = be.front_classes()
    dims = arrays.var_dims.astype(np.int64)
    arena = 0
    for f, (fv, sv) in enumerate(fronts):
        if (int(cls[f]) & 3) != 0:
            F, m = int(dims[fv].sum()), int(dims[fv].sum() + dims[sv].sum())
            arena += 8 * m * (m + F)
    rec = {"workload": args.workload, "n_vars": arrays.n_vars, "n_fronts": len(fronts),
           "tangent_size": int(dims.sum()), "covariance_arena_bytes": arena}
    print(json.dumps(rec), flush=True)
    t0 = time.perf_counter()
    blocks = be.marginal_covariances()      # warm: factorization, arena, work lists
    rec["first_call_s"] = time.perf_counter() - t0
    print(f"first call {rec['first_call_s']:.3f} s", flush=True)
    if args.one_pass_only:
        be.marginal_covariances()
        return
    n_out = be.marginal_blocks_size()
    out = np.zeros(n_out)
    import ctypes as C
    fn = be._fn("marginal_covariances")
    ptr = out.ctypes.data_as(C.POINTER(C.c_double))
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        st = fn(be._h, None, C.c_int32(0), ptr, C.c_int64(n_out))
        ts.append(time.perf_counter() - t0)
        assert st == 0
    rec["all_variables_s_median"] = float(np.median(ts))
    rec["all_variables_s_all"] = ts
    print(f"(a) all variables: median {rec['all_variables_s_median'] * 1e3:.2f} ms", flush=True)
    rng = np.random.default_rng(7)
    keys = [int(k) for k in rng.choice(arrays.var_keys, size=min(args.keys, arrays.n_vars), replace=False)]
    be.marginal_covariance(keys[0])
    t0 = time.perf_counter()
    worst = 0.0
    per = {}
    for k in keys:
        per[k] = be.marginal_covariance(k)
    t_loop = time.perf_counter() - t0
    for k in keys:
        worst = max(worst, float(np.max(np.abs(per[k] - blocks[k])) / np.max(np.abs(per[k]))))
    rec["per_variable_s_per_key"] = t_loop / len(keys)
    rec["per_variable_s_extrapolated"] = t_loop / len(keys) * arrays.n_vars
    rec["per_variable_keys"] = len(keys)
    rec["worst_relative_difference"] = worst
    print(f"(b) per variable: {t_loop / len(keys) * 1e3:.3f} ms a key, {rec['per_variable_s_extrapolated']:.2f} s for all; "
          f"worst difference {worst:.2e}", flush=True)
    be.set_profiling(1)
    be.reset_stats()
    be.marginal_covariances()
    rec["kernel_ms"] = {}
    for name in KERNELS:
        avg, n = be.kernel_time(name)
        rec["kernel_ms"][name] = {"launches": int(n), "total_ms": float(avg) * int(n)}
    be.set_profiling(-1)
    print(json.dumps(rec["kernel_ms"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    recs = []
    if os.path.exists(args.out):
        with open(args.out) as fh:
            recs = json.load(fh)
    recs = [r for r in recs if r["workload"] != args.workload] + [rec]
    with open(args.out, "w") as fh:
        json.dump(recs, fh, indent=1)


if __name__ == "__main__":
    main()
