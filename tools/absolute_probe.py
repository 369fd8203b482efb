"""Times of the absolute-measurement factor kernels on a seeded vehicle log: a Pose3 chain of --poses poses with one
BetweenFactor, one GPSFactor and one Pose3AttitudeFactor per pose.  Reports

  * the gsx_kernel_time of "linearize" and "error" (HIP events, profiling level 0, averaged over --reps calls) on the graph
    of the GPS and attitude factors ALONE, where each phase is one launch: linearize_absolute_kernel, and
    error_absolute_kernel with its final reduction;
  * the same two phase times on the whole chain (the between kernels and the absolute ones);
  * the wall time of an LM trial (gsx_lm_optimize over --iterations iterations, divided by the trials of its trace) on the
    whole chain, and on the same chain with the absolute factors replaced by one prior on the first pose.

Prints one JSON line.  --host-only builds the graphs and stops (no device needed).

usage: python tools/absolute_probe.py [--poses 100000] [--seed 42] [--reps 20] [--iterations 10] [--host-only]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gtsam_petercdev_amd import _abi as A, _lib  # noqa: E402

DOWN = np.array([0.0, 0.0, -1.0])


def expmap(w):
    th = np.linalg.norm(w, axis=-1)[..., None, None]
    W = np.zeros(w.shape[:-1] + (3, 3))
    W[..., 0, 1], W[..., 0, 2], W[..., 1, 0] = -w[..., 2], w[..., 1], w[..., 2]
    W[..., 1, 2], W[..., 2, 0], W[..., 2, 1] = -w[..., 0], -w[..., 1], w[..., 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.where(th > 1e-8, np.sin(th) / th, 1.0)
        b = np.where(th > 1e-8, (1 - np.cos(th)) / (th * th), 0.5)
    return np.eye(3) + a * W + b * (W @ W)


def chain(n, seed):
    """(truth states n x 12, initial states, per-pose between / GPS / attitude measurements)."""
    rng = np.random.default_rng(seed)
    dR = expmap(rng.normal(0, 0.05, (n, 3)))
    Rs, ts = np.zeros((n, 3, 3)), np.zeros((n, 3))
    Rs[0] = np.eye(3)
    for i in range(1, n):
        Rs[i] = Rs[i - 1] @ dR[i]
        ts[i] = ts[i - 1] + Rs[i - 1] @ np.array([1.0, 0.0, 0.0])
    pack = lambda R_, t_: np.concatenate([R_.reshape(len(R_), 9), t_], axis=1)
    truth = pack(Rs, ts)
    between = pack(np.swapaxes(Rs[:-1], 1, 2) @ Rs[1:] @ expmap(rng.normal(0, 0.005, (n - 1, 3))),
                   np.einsum("nji,nj->ni", Rs[:-1], ts[1:] - ts[:-1]) + rng.normal(0, 0.02, (n - 1, 3)))
    gps = ts + rng.normal(0, 0.5, (n, 3))
    b = np.einsum("nji,j->ni", Rs, DOWN) + rng.normal(0, 0.01, (n, 3))
    att = np.concatenate([np.tile(DOWN, (n, 1)), b / np.linalg.norm(b, axis=1)[:, None]], axis=1)
    initial = pack(Rs @ expmap(rng.normal(0, 0.02, (n, 3))), ts + rng.normal(0, 0.2, (n, 3)))
    return truth, initial, between, gps, att


def arrays(n, initial, parts):
    """parts: [(factor type, rows, keys n_f x k, measurements n_f x m, sigma)] in graph order."""
    f_type, f_rows, key_ptr, fvars, meas_ptr, meas, noise = [], [], [0], [], [0], [], []
    for ftype, rows, keys, z, sigma in parts:
        nf, k, m = len(keys), keys.shape[1], z.shape[1]
        f_type += [ftype] * nf
        f_rows += [rows] * nf
        key_ptr += (key_ptr[-1] + k * np.arange(1, nf + 1)).tolist()
        fvars.append(keys.reshape(-1))
        meas_ptr += (meas_ptr[-1] + m * np.arange(1, nf + 1)).tolist()
        meas.append(z.reshape(-1))
        noise += [sigma] * nf
    nf = len(f_type)
    return A.ProblemArrays(var_keys=np.arange(n, dtype=np.uint64), var_types=[A.VAR_POSE3] * n, var_dims=[6] * n, f_type=f_type,
                           f_rows=f_rows, f_key_ptr=key_ptr, f_vars=np.concatenate(fvars), f_meas_ptr=meas_ptr,
                           meas=np.concatenate(meas), f_noise_kind=[A.NOISE_ISOTROPIC] * nf, f_noise_ptr=list(range(nf + 1)),
                           noise=np.array(noise), values=initial.reshape(-1))


def graphs(n, seed):
    truth, initial, between, gps, att = chain(n, seed)
    idx = np.arange(n)[:, None]
    bet = (A.F_BETWEEN, 6, np.concatenate([idx[:-1], idx[1:]], axis=1), between, 0.05)
    absolute = [(A.F_GPS, 3, idx, gps, 0.5), (A.F_ATTITUDE, 2, idx, att, 0.05)]
    prior = (A.F_PRIOR, 6, idx[:1], truth[:1], 0.01)
    return {"absolute_only": arrays(n, initial, absolute), "chain": arrays(n, initial, [bet] + absolute),
            "chain_one_prior": arrays(n, initial, [bet, prior])}


def phase_times(arr, reps):
    be = _lib.ProductBackend(arr)
    be.linearize(); be.error()      # (the first calls pay the module load)
    be.set_profiling(0)
    be.reset_stats()
    for _ in range(reps):
        be.linearize()
        be.error()
    be.synchronize()
    out = {"linearize_ms": be.kernel_time("linearize")[0], "error_ms": be.kernel_time("error")[0]}
    be.close()
    return out


def lm_trial_ms(arr, iterations):
    be = _lib.ProductBackend(arr)
    be.set_ordering(be.compute_ordering(A.ORDER_ND))
    p = A.lm_params_legacy()
    p.max_iterations, p.relative_error_tol, p.absolute_error_tol = 2, 0.0, 0.0
    be.lm_optimize(p)               # warm-up
    be.set_values(arr.values)
    p.max_iterations = iterations
    be.synchronize()
    t0 = time.perf_counter()
    res = be.lm_optimize(p)
    dt = time.perf_counter() - t0
    be.close()
    trials = len(res["trace_error"])
    return {"lm_trial_ms": 1e3 * dt / max(trials, 1), "trials": trials, "initial_error": res["initial_error"],
            "final_error": res["final_error"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args()
    g = graphs(a.poses, a.seed)
    rec = dict(n_poses=a.poses, factors={k: int(v.n_factors) for k, v in g.items()}, device=None)
    if not a.host_only:
        rec["device"] = _lib.device_count() > 0
        rec["absolute_only"] = phase_times(g["absolute_only"], a.reps)
        rec["chain"] = dict(phase_times(g["chain"], a.reps), **lm_trial_ms(g["chain"], a.iterations))
        rec["chain_one_prior"] = dict(phase_times(g["chain_one_prior"], a.reps), **lm_trial_ms(g["chain_one_prior"], a.iterations))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
