"""ms per PCG iteration and PCG iterations per LM step on bal1723 and pose3_100k (needs a GPU; nothing here has been run
on one yet).  Usage: python tools/pcg_probe.py [--workload bal1723|pose3_100k] [--epsilon 1e-3] [--steps 3]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gtsam_petercdev_amd import _abi as A, _lib, datasets  # noqa: E402


def problem(name, seed=42):
    if name == "bal1723":
        return datasets.synth_bal_arrays(1723, 156502, 678718, seed=seed, long_range=0.3), A.ORDER_SCHUR_ND, True
    return datasets.synth_manhattan_pose3(100000, seed=seed), A.ORDER_ND, False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default=None, choices=["bal1723", "pose3_100k"])
    ap.add_argument("--epsilon", type=float, default=1e-3)
    ap.add_argument("--steps", type=int, default=3)
    args = ap.parse_args()
    assert _lib.device_count() > 0, "needs a GPU"
    for name in ([args.workload] if args.workload else ["bal1723", "pose3_100k"]):
        arr, order, diag = problem(name)
        gb = _lib.product_backend(arr)
        gb.set_ordering(gb.compute_ordering(order))
        gb.linearize()
        prm = _lib.pcg_params_default()
        prm.epsilon_rel, prm.epsilon_abs = args.epsilon, 0.0
        gb.solve_pcg(1e-4, diag, params=prm, want_delta=False)          # warm-up: tables, allocation
        t0 = time.perf_counter()
        _, st = gb.solve_pcg(1e-4, diag, params=prm, want_delta=False)
        dt = time.perf_counter() - t0
        gb.set_linear_solver(A.SOLVER_PCG, prm)
        p = A.lm_params_ceres() if diag else A.lm_params_legacy()
        p.max_iterations = args.steps
        r = gb.lm_optimize(p)
        print(json.dumps(dict(workload=name, epsilon_rel=args.epsilon, pcg_iterations=st["iterations"],
                              converged=st["converged"], ms_per_pcg_iteration=1e3 * dt / max(st["iterations"], 1),
                              lm_trials=len(r["trace_accepted"]),
                              pcg_iterations_per_lm_trial=r["pcg_iterations"] / max(len(r["trace_accepted"]), 1),
                              final_error=r["final_error"])))
        gb.close()


if __name__ == "__main__":
    main()
