#!/usr/bin/env python3
"""linearize / error phase time (gsx_kernel_time) of a >= 100k-factor stereo graph — the VO fixture of tests/golden replicated
13 times — against the same structure built with GSX_F_PROJECTION factors (profiles/stereo_vs_projection_linearize.json).

    python tools/stereo_probe.py [out.json]"""
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from gtsam_petercdev_amd import _abi as A, _lib

G = os.path.join(ROOT, "tests", "golden")
K = np.loadtxt(os.path.join(G, "VO_calibration.txt")).reshape(-1)[:6]
poses = np.loadtxt(os.path.join(G, "VO_camera_poses_large.txt")).reshape(-1, 17)
fac = np.loadtxt(os.path.join(G, "VO_stereo_factors_large.txt.gz")).reshape(-1, 8)
REP = 13
pose_state = {}
for row in poses:
    m = row[1:].reshape(4, 4)
    pose_state[int(row[0])] = np.concatenate([m[:3, :3].reshape(9), m[:3, 3]])
lm_state = {}
for x, l, uL, uR, v, X, Y, Z in fac:
    if int(l) not in lm_state:
        s = pose_state[int(x)]
        lm_state[int(l)] = s[:9].reshape(3, 3) @ np.array([X, Y, Z]) + s[9:]
pk, lk = sorted(pose_state), sorted(lm_state)
npz, nl = len(pk), len(lk)
keys, types, dims, vals = [], [], [], []
for r in range(REP):
    for p in pk:
        keys.append((ord('x') << 56) | (r * 1000 + p))
        types.append(A.VAR_POSE3)
        dims.append(6)
        vals.append(pose_state[p])
for r in range(REP):
    for l in lk:
        keys.append((ord('z') << 56) | (r * 100000 + l))
        types.append(A.VAR_VECTOR)
        dims.append(3)
        vals.append(lm_state[l])
pi = {p: i for i, p in enumerate(pk)}
li = {l: i for i, l in enumerate(lk)}

def build(stereo):
    nf = len(fac) * REP
    f_vars = np.zeros((nf, 2), np.int32)
    nm = 9 if stereo else 7
    meas = np.zeros((nf, nm))
    i = 0
    for r in range(REP):
        for x, l, uL, uR, v, *_ in fac:
            f_vars[i] = (r * npz + pi[int(x)], REP * npz + r * nl + li[int(l)])
            meas[i] = [uL, uR, v, *K] if stereo else [uL, v, *K[:5]]
            i += 1
    m = 3 if stereo else 2
    arr = A.ProblemArrays(var_keys=np.array(keys, dtype=np.uint64), var_types=types, var_dims=dims,
                          f_type=np.full(nf, A.F_STEREO if stereo else A.F_PROJECTION), f_rows=np.full(nf, m),
                          f_key_ptr=np.arange(nf + 1) * 2, f_vars=f_vars.reshape(-1), f_meas_ptr=np.arange(nf + 1) * nm,
                          meas=meas.reshape(-1), f_noise_kind=np.full(nf, A.NOISE_ISOTROPIC), f_noise_ptr=np.arange(nf + 1),
                          noise=np.ones(nf), values=np.concatenate(vals))
    for r in range(REP):
        arr = arr.with_factor(A.F_PRIOR, [r * npz], 6, pose_state[pk[0]], A.NOISE_ISOTROPIC, [0.01])
    return arr

out = {"replicas": REP, "device": "MI355X"}
for name, stereo in (("stereo", True), ("projection", False)):
    arr = build(stereo)
    be = _lib.ProductBackend(arr)
    be.set_ordering(be.compute_ordering(A.ORDER_SCHUR_ND))
    be.set_profiling(0)
    for _ in range(5):
        be.linearize()
        be.error()
    be.synchronize()
    be.reset_stats()
    for _ in range(50):
        be.linearize()
        be.error()
    be.synchronize()
    lin, nlin = be.kernel_time("linearize")
    err, nerr = be.kernel_time("error")
    out[name] = {"n_factors": int(arr.n_factors), "jacobian_bytes": int(be.jacobian_size * 8),
                 "linearize_ms": lin, "linearize_launches": nlin, "error_ms": err, "error_launches": nerr}
    print(name, out[name], flush=True)
    be.close()
out["linearize_ratio"] = out["stereo"]["linearize_ms"] / out["projection"]["linearize_ms"]
out["error_ratio"] = out["stereo"]["error_ms"] / out["projection"]["error_ms"]
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
print(json.dumps(out))
