"""Times of the smart projection factor kernels on a seeded graph: --poses camera poses on a circle, --factors smart factors
whose track lengths are drawn from 2 .. 8, pixels with 0.5 px of noise, two pose priors.  Reports the phase times of
gsx_linearize and gsx_error (HIP events, profiling level 0) averaged over --reps calls, each at values moved by more than
the re-triangulation threshold (so every call triangulates) and once more with unmoved values (the cache answers).  Prints
one JSON line.  No time has been measured with it yet.  --host-only builds the graph and stops (no device needed).

usage: python tools/smart_probe.py [--poses 2000] [--factors 100000] [--seed 42] [--reps 10] [--epi] [--host-only]"""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gtsam_petercdev_amd import _abi as A, _lib  # noqa: E402

K = np.array([520.0, 510.0, 0.0, 320.0, 240.0])


def graph(n_poses, n_factors, seed, epi):
    rng = np.random.default_rng(seed)
    poses = np.zeros((n_poses, 12))
    for i in range(n_poses):   # on a circle of radius 30, looking at the centre
        a = 2 * math.pi * i / n_poses
        z = -np.array([math.cos(a), math.sin(a), 0.0])
        x = np.array([-math.sin(a), math.cos(a), 0.0])
        poses[i, :9] = np.stack([x, np.cross(z, x), z], axis=1).reshape(9)
        poses[i, 9:] = [30 * math.cos(a), 30 * math.sin(a), 0.0]
    f_rows, key_ptr, fvars, meas_ptr, meas = [], [0], [], [0], []
    for _ in range(n_factors):
        nk = int(rng.integers(2, 9))
        first = int(rng.integers(0, n_poses))
        views = [(first + j) % n_poses for j in range(nk)]
        p = rng.uniform(-8, 8, 3)
        px = []
        for v in views:
            q = poses[v, :9].reshape(3, 3).T @ (p - poses[v, 9:])
            px += [K[0] * q[0] / q[2] + K[3] + 0.5 * rng.standard_normal(), K[1] * q[1] / q[2] + K[4] + 0.5 * rng.standard_normal()]
        m = np.concatenate([K, [1.0, float(epi), -1.0, -1.0, 1e-5, 1.0], px])
        f_rows.append(2 * nk - 3)
        fvars += views
        key_ptr.append(len(fvars))
        meas.append(m)
        meas_ptr.append(meas_ptr[-1] + m.size)
    nptr = list(range(n_factors + 1))
    for v in (0, 1):
        f_rows.append(6); fvars.append(v); key_ptr.append(len(fvars)); meas.append(poses[v]); meas_ptr.append(meas_ptr[-1] + 12)
        nptr.append(nptr[-1] + 1)
    return A.ProblemArrays(var_keys=np.arange(n_poses, dtype=np.uint64), var_types=[A.VAR_POSE3] * n_poses, var_dims=[6] * n_poses,
                           f_type=[A.F_SMART_PROJECTION] * n_factors + [A.F_PRIOR] * 2, f_rows=f_rows, f_key_ptr=key_ptr,
                           f_vars=fvars, f_meas_ptr=meas_ptr, meas=np.concatenate(meas),
                           f_noise_kind=[A.NOISE_ISOTROPIC] * (n_factors + 2), f_noise_ptr=nptr,
                           noise=np.concatenate([np.ones(n_factors), [0.1, 0.1]]), values=poses.reshape(-1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=2000)
    ap.add_argument("--factors", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--epi", action="store_true")
    ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args()
    arr = graph(a.poses, a.factors, a.seed, a.epi)
    rec = dict(n_poses=a.poses, n_factors=a.factors, mean_length=float(np.diff(arr.f_key_ptr)[:a.factors].mean()), epi=a.epi,
               jacobian_doubles=int(arr.jacobian_offsets()[-1]), device=None)
    if not a.host_only:
        be = _lib.ProductBackend(arr)
        be.linearize(); be.error()   # (the first calls pay the module load)
        be.set_profiling(0)
        rng = np.random.default_rng(a.seed + 1)
        for label, moved in (("retriangulating", True), ("cached", False)):
            be.reset_stats()
            n_retri = 0
            for _ in range(a.reps):
                if moved:
                    v = arr.values.reshape(-1, 12).copy()
                    v[:, 9:] += 1e-3 * rng.standard_normal((a.poses, 3))
                    be.set_values(v.reshape(-1))
                be.linearize()
                n_retri += be.stats()["n_smart_retriangulated"]
                be.error()
            s = be.stats()
            rec[label] = dict(ms_linearize=s["ms_linearize"] / max(s["n_linearize"], 1), ms_error=s["ms_error"] / max(s["n_error"], 1),
                              retriangulated_per_linearize=n_retri / a.reps, n_smart_invalid=s["n_smart_invalid"])
        rec["device"] = 0
        be.close()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
