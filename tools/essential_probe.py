#!/usr/bin/env python3
"""Kernel time of the epipolar linearize and error kernels on a synthetic two-view problem: by default 100 000
correspondences spread over 1 000 EssentialMatrix variables, one graph per factor form, so that the linearize phase is the
form's one launch and the error phase its one launch plus the final reduction (gsx_kernel_time over --reps calls, HIP events).

    python tools/essential_probe.py [--essentials 1000] [--correspondences 100000] [--reps 20] [--host-only]

Prints one JSON line; profiles/essential_kernels.json keeps a recorded run."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gtsam_petercdev_amd import _abi as A, _lib  # noqa: E402

F_E, F_DEPTH, F_CALIB, F_CONSTRAINT = A.F_ESSENTIAL, A.F_ESSENTIAL_DEPTH, A.F_ESSENTIAL_CALIB, A.F_ESSENTIAL_CONSTRAINT


def rotations(rng, n, scale):
    w = rng.normal(0, scale, (n, 3))
    th = np.linalg.norm(w, axis=1)[:, None, None]
    W = np.zeros((n, 3, 3))
    W[:, 0, 1], W[:, 0, 2], W[:, 1, 0] = -w[:, 2], w[:, 1], w[:, 2]
    W[:, 1, 2], W[:, 2, 0], W[:, 2, 1] = -w[:, 0], -w[:, 1], w[:, 0]
    return np.eye(3) + (np.sin(th) / th) * W + ((1 - np.cos(th)) / (th * th)) * (W @ W)


def build(form, n_e, n_c, seed):
    rng = np.random.default_rng(seed)
    Rs = rotations(rng, n_e, 0.3)
    t = rng.normal(size=(n_e, 3))
    t /= np.linalg.norm(t, axis=1)[:, None]
    E = np.concatenate([Rs.reshape(n_e, 9), t], axis=1)
    owner = np.arange(n_c) % n_e
    P1 = np.stack([rng.uniform(-1, 1, n_c), rng.uniform(-1, 1, n_c), rng.uniform(3, 8, n_c)], axis=1)
    P2 = np.einsum("nji,nj->ni", Rs[owner], P1 - t[owner])
    pA, pB = P1[:, :2] / P1[:, 2:], P2[:, :2] / P2[:, 2:] + rng.normal(0, 1e-3, (n_c, 2))
    one = np.ones((n_c, 1))
    types, dims, states = [A.VAR_ESSENTIAL] * n_e, [5] * n_e, [E.reshape(-1)]
    if form == "essential":
        keys, m, z = owner[:, None], 1, np.concatenate([pA, one, pB, one], axis=1)
        ftype = F_E
    elif form in ("depth", "depth_rotated"):
        types += [A.VAR_VECTOR] * n_c
        dims += [1] * n_c
        states.append(1.0 / P1[:, 2])
        keys, m, z = np.stack([owner, n_e + np.arange(n_c)], axis=1), 2, np.concatenate([pA, one, pB, one], axis=1)
        if form == "depth_rotated":
            z = np.concatenate([z, np.tile(np.eye(3).reshape(1, 9), (n_c, 1))], axis=1)
        ftype = F_DEPTH
    elif form == "calib":
        K = np.array([500.0, 500.0, 0.0, 320.0, 240.0])
        types += [A.VAR_VECTOR] * n_e
        dims += [5] * n_e
        states.append(np.tile(K, n_e))
        keys, m = np.stack([owner, n_e + owner], axis=1), 1
        z = np.concatenate([500 * pA + K[3:], 500 * pB + K[3:]], axis=1)
        ftype = F_CALIB
    else:   # constraint: n_e poses, n_c edges between random pairs, measured from the poses themselves
        types, dims = [A.VAR_POSE3] * n_e, [6] * n_e
        pos = rng.normal(0, 5, (n_e, 3))
        states = [np.concatenate([Rs.reshape(n_e, 9), pos], axis=1).reshape(-1)]
        i = rng.integers(0, n_e, n_c)
        j = (i + 1 + rng.integers(0, n_e - 1, n_c)) % n_e
        th = np.einsum("nji,nj->ni", Rs[i], pos[j] - pos[i])
        z = np.concatenate([(np.swapaxes(Rs[i], 1, 2) @ Rs[j]).reshape(n_c, 9), th / np.linalg.norm(th, axis=1)[:, None]], axis=1)
        keys, m, ftype = np.stack([i, j], axis=1), 5, F_CONSTRAINT
    k, nm = keys.shape[1], z.shape[1]
    return A.ProblemArrays(var_keys=np.arange(len(types), dtype=np.uint64), var_types=types, var_dims=dims, f_type=[ftype] * n_c,
                           f_rows=[m] * n_c, f_key_ptr=(k * np.arange(n_c + 1)).tolist(), f_vars=keys.reshape(-1),
                           f_meas_ptr=(nm * np.arange(n_c + 1)).tolist(), meas=z.reshape(-1),
                           f_noise_kind=[A.NOISE_ISOTROPIC] * n_c, f_noise_ptr=list(range(n_c + 1)), noise=np.full(n_c, 0.01),
                           values=np.concatenate(states))


def phase_times(arr, reps):
    be = _lib.ProductBackend(arr)
    be.linearize(); be.error()      # (the first calls pay the module load)
    be.set_profiling(0)
    be.reset_stats()
    for _ in range(reps):
        be.linearize()
        be.error()
    be.synchronize()
    out = {"linearize_us": 1e3 * be.kernel_time("linearize")[0], "error_us": 1e3 * be.kernel_time("error")[0]}
    be.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--essentials", type=int, default=1000)
    ap.add_argument("--correspondences", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args()
    rec = dict(essentials=a.essentials, correspondences=a.correspondences, reps=a.reps, device=None)
    for form in ("essential", "depth", "depth_rotated", "calib", "constraint"):
        arr = build(form, a.essentials, a.correspondences, a.seed)
        rec[form] = {"factors": int(arr.n_factors)}
        if not a.host_only:
            rec["device"] = _lib.device_count() > 0
            t = phase_times(arr, a.reps)
            t["linearize_ns_per_factor"] = 1e3 * t["linearize_us"] / arr.n_factors
            rec[form].update(t)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
