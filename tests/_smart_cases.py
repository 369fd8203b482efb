"""Seeded smart-projection cases shared by tests/test_host_smart_factor.py and tests/test_gpu_smart_factor.py, their
references (float64 and 50 digits, computed once and cached) and the bounds the device is held to.  Test infrastructure only.

Bounds.  The device block is compared through its augmented Hessian D = [A b]'[A b] with the 50-digit H of the reference's
route.  First rule: |D - H|_F <= 10 |H64 - H|_F, H64 the float64 restatement.  Where that is the larger
one, a backward bound takes its place, derived from the operation count and never from a device figure:
  * a column of [F b] costs at most 40 rounded operations (projection, calibration, the 2 x 6 chain, the sensor adjoint,
    whitening), a reflector applied to a column of 16 rows 2 x 16 + 2 more, three of them 102, forming a reflector from E
    about 60, and an entry of [A b]'[A b] a sum of 13 products: k = 40 + 102 + 60 + 13 = 215 operations stand behind an
    entry, so gamma = k u / (1 - k u) with u = 2^-53;
  * Householder QR is backward stable: the computed Q_2 spans the exact left null space of E + dE, |dE|_F <= gamma |E|_F, and
    the projector onto that null space moves by at most |dE|_2 / sigma_min(E) = gamma cond_2(E);
  * hence |D - H|_F <= gamma (1 + cond_2(E)) |[F b]|_F^2.
The point the block is taken at is the factor's own triangulation; its forward error is common to every backward-stable
triangulation and is what the float64 restatement's distance measures, which is why the first rule comes first.
The error is a sum of 2 nk squares of about 25 operations each, taken at the factor's own point p: to first order
|e - e_ref| <= gamma_e e_ref + |E'b| |dp|, gamma_e from k = 25 + 2 nk, |E'b| the slope of the error in the point (it does not
vanish: the DLT point is not the minimizer) and |dp| the forward bound of the linear stage of tests/_triangulation_cases.py,
gamma_t sigma_1 / (sigma_3 - sigma_4) (1 + |p|^2), which a refinement does not amplify (refined_bound there).  The test takes
the larger of that and 10 |e64 - e_ref|."""
from __future__ import annotations

import math

import numpy as np

from . import _smart_restatement as R
from . import _triangulation_cases as TC
from gtsam_petercdev_amd import _abi as A

U = 2.0 ** -53
K_CAL = np.array([520.0, 510.0, 0.3, 320.0, 240.0])
TRACK_LENGTHS = (2, 3, 7, 8)
FACTOR_COUNTS = (1, 63, 64, 65, 257)
N_POSES = 8


def gamma(k):
    return k * U / (1 - k * U)


def rot_ypr(y, p, r):
    cy, sy, cp, sp, cr, sr = math.cos(y), math.sin(y), math.cos(p), math.sin(p), math.cos(r), math.sin(r)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return Rz @ Ry @ Rx


def state(Rm, t):
    return np.concatenate([np.asarray(Rm, float).reshape(9), np.asarray(t, float)])


def compose(a, b):
    Ra, Rb = a[:9].reshape(3, 3), b[:9].reshape(3, 3)
    return state(Ra @ Rb, a[9:] + Ra @ b[9:])


def inverse(a):
    Ra = a[:9].reshape(3, 3)
    return state(Ra.T, -Ra.T @ a[9:])


def expmap_small(pose, xi):
    """pose (+) xi with a first-order rotation re-orthonormalized by QR: a seeded perturbation, not a retraction under test"""
    w, v = np.asarray(xi[:3], float), np.asarray(xi[3:], float)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    Q, Rr = np.linalg.qr(np.eye(3) + W + W @ W / 2)
    Q = Q * np.sign(np.diag(Rr))
    return compose(pose, state(Q, v))


SENSOR = (rot_ypr(0.02, -0.03, 0.01), np.array([0.05, -0.02, 0.1]))
SENSOR_STATE = state(*SENSOR)


def camera_poses(seed=7):
    """8 camera poses on an arc, looking roughly along +x from around the origin (the reference's level_pose family)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(N_POSES):
        Rm = rot_ypr(-math.pi / 2 + 0.06 * (i - 3.5) + 0.01 * rng.standard_normal(), 0.01 * rng.standard_normal(),
                     -math.pi / 2 + 0.01 * rng.standard_normal())
        out.append(state(Rm, [0.1 * rng.standard_normal(), 0.6 * (i - 3.5), 1.0 + 0.3 * rng.standard_normal()]))
    return out


def project(cam_pose, K, p):
    Rm, t = cam_pose[:9].reshape(3, 3), cam_pose[9:]
    q = Rm.T @ (np.asarray(p, float) - t)
    u, v = q[0] / q[2], q[1] / q[2]
    return np.array([K[0] * u + K[2] * v + K[3], K[1] * v + K[4]])


def make_spec(views, landmark, cam_poses, sigma=1.0, sensor=False, epi=False, pixel_noise=0.5, seed=0, **kw):
    """the factor that sees `landmark` from the cameras cam_poses[views]; with a sensor the BODY poses are
    camera (+) sensor^-1, so that the cameras stay where they are (body_poses_for)"""
    rng = np.random.default_rng(1000 + seed)
    px = np.array([project(cam_poses[v], K_CAL, landmark) + pixel_noise * rng.standard_normal(2) for v in views])
    return R.Spec(K=K_CAL, pixels=px, sigma=sigma, enable_epi=epi, sensor=SENSOR if sensor else None, views=list(views), **kw)


def body_poses(cam_poses, sensor):
    return [compose(c, inverse(SENSOR_STATE)) for c in cam_poses] if sensor else list(cam_poses)


def landmarks(n, seed=11):
    rng = np.random.default_rng(seed)
    return [np.array([6.0 + 2.0 * rng.random(), 1.5 * rng.standard_normal(), 1.0 + 0.8 * rng.standard_normal()])
            for _ in range(n)]


def track_cases():
    """nk in TRACK_LENGTHS x sigma in (1, 0.1) x sensor x enable_epi: (name, spec, body poses of the whole pose list)"""
    cams = camera_poses()
    lms = landmarks(64)
    out, k = [], 0
    for nk in TRACK_LENGTHS:
        for sigma in (1.0, 0.1):
            for sensor in (False, True):
                for epi in (False, True):
                    # (3 j mod 8 is distinct for j < 3: short tracks see spread-out cameras, in an order that is not ascending)
                    views = list(range(nk)) if nk >= 7 else [(k + 3 * j) % N_POSES for j in range(nk)]
                    spec = make_spec(views, lms[k], cams, sigma=sigma, sensor=sensor, epi=epi, seed=k)
                    out.append((f"nk{nk}-s{sigma}-sensor{int(sensor)}-epi{int(epi)}", spec, body_poses(cams, sensor)))
                    k += 1
    return out


def invalid_cases():
    """ordinary data on which triangulateSafe finds no valid point: (name, spec, poses, expected status)"""
    cams = camera_poses()
    lm = np.array([6.5, 0.3, 1.2])
    same = [cams[0], cams[0].copy()] + cams[2:]
    behind = np.array([-6.0, 0.2, 1.0])
    out = [("identical_poses", make_spec([0, 1], lm, same, pixel_noise=0.0), same, R.DEGENERATE)]
    # a point behind the cameras projects to pixels whose rays meet behind them: BEHIND_CAMERA
    sp = make_spec([0, 3, 6], behind, cams, pixel_noise=0.0, rank_tol=1e-9)
    out.append(("behind_camera", sp, cams, 2))
    out.append(("far_point", make_spec([0, 2, 5], lm, cams, landmark_distance_threshold=2.0), cams, 4))
    sp = make_spec([1, 4, 7], lm, cams, pixel_noise=0.0, outlier_threshold=1.0)
    sp.pixels[0] += np.array([10.0, 10.0])
    out.append(("outlier", sp, cams, 3))
    return out


# ---- lowering (independent of graph.py) -----------------------------------------------------------------------------------
def meas_of(spec):
    head = list(spec.K) + [spec.rank_tol, float(spec.enable_epi), spec.landmark_distance_threshold, spec.outlier_threshold,
                           spec.retriangulation_threshold, 1.0]
    if spec.sensor is not None:
        head += list(state(*spec.sensor))
    return np.concatenate([np.array(head, float), np.asarray(spec.pixels, float).reshape(-1)])


def graph_arrays(specs, poses, prior_on=(0, 1), prior_sigma=0.1, keys=None):
    """the smart factors `specs` on the POSE3 variables `poses` (keys 0 .. n-1), then a pose prior AT the current value on
    each variable of prior_on (its Jacobian is then the identity over sigma and its right-hand side zero)"""
    n = len(poses)
    f_type, f_rows, key_ptr, fvars, meas_ptr, meas, nkind, nptr, noise = [], [], [0], [], [0], [], [], [0], []
    for s in specs:
        f_type.append(A.F_SMART_PROJECTION)
        f_rows.append(2 * s.nk - 3)
        fvars += list(s.views)
        key_ptr.append(len(fvars))
        m = meas_of(s)
        meas.append(m)
        meas_ptr.append(meas_ptr[-1] + m.size)
        if s.sigma == 1.0:
            nkind.append(A.NOISE_UNIT)
        else:
            nkind.append(A.NOISE_ISOTROPIC)
            noise.append(s.sigma)
        nptr.append(len(noise))
    for v in prior_on:
        f_type.append(A.F_PRIOR)
        f_rows.append(6)
        fvars.append(v)
        key_ptr.append(len(fvars))
        meas.append(np.asarray(poses[v], float))
        meas_ptr.append(meas_ptr[-1] + 12)
        nkind.append(A.NOISE_ISOTROPIC)
        noise.append(prior_sigma)
        nptr.append(len(noise))
    return A.ProblemArrays(var_keys=np.arange(n, dtype=np.uint64) if keys is None else keys, var_types=[A.VAR_POSE3] * n,
                           var_dims=[6] * n, f_type=f_type, f_rows=f_rows, f_key_ptr=key_ptr, f_vars=fvars,
                           f_meas_ptr=meas_ptr, meas=np.concatenate(meas), f_noise_kind=nkind, f_noise_ptr=nptr,
                           noise=np.array(noise, float), values=np.concatenate([np.asarray(p, float) for p in poses]))


def mixed_graph(n_factors):
    """n_factors smart factors of mixed track lengths on the 8 camera poses: the sensor-free cases of track_cases() in a
    stride that mixes lengths, sigmas and the refinement inside every wave (the sensor cases need other body poses)"""
    pool = [(n, s) for n, s, _ in track_cases() if s.sensor is None]
    cams = camera_poses()
    specs = [pool[(5 * i) % len(pool)][1] for i in range(n_factors)]
    return specs, cams


# ---- references, computed once -------------------------------------------------------------------------------------------------
_REF = {}


def reference(spec, poses, X):
    """linearize then error on a fresh factor at `poses` (the pose list the factor's views index): dict(status, point, H,
    fb2, condE, error, decisions)"""
    key = (id(spec), X.name, hash(np.concatenate(poses).tobytes()))
    if key not in _REF:
        f = R.SmartFactor(spec, X)
        own = [poses[v] for v in spec.views]
        H, fb2, cond = f.hessian(own)
        dp = 0.0
        if f.status == R.VALID:
            s = [float(v) for v in f.tri.sigma]
            x = np.array([float(v) for v in f.tri.linear_point])
            dp = TC.gamma(spec.nk) * s[0] / (s[2] - s[3]) * (1 + x.dot(x))
        _REF[key] = dict(status=f.status, point=f.point_float(), H=H, fb2=fb2, condE=cond, grad=float(f.grad_norm), dp=dp,
                         error=f.error(own), decisions=list(f.decisions), spec=spec)
    return _REF[key]


def frob(M):
    return math.sqrt(float(sum(x * x for x in np.asarray(M, dtype=object).reshape(-1))))


def hessian_bound(spec, poses):
    """(bound, d64, backward): the distance the device's augmented Hessian may have from the 50-digit one"""
    r64, rmp = reference(spec, poses, R.FLOAT), reference(spec, poses, R.MP)
    d64 = frob(np.asarray(r64["H"], dtype=object) - rmp["H"])
    backward = gamma(215) * (1.0 + float(rmp["condE"])) * float(rmp["fb2"])
    return max(10.0 * d64, backward), d64, backward


def error_bound(spec, poses):
    r64, rmp = reference(spec, poses, R.FLOAT), reference(spec, poses, R.MP)
    d64 = abs(float(r64["error"] - rmp["error"]))
    return max(10.0 * d64, gamma(25 + 2 * spec.nk) * float(rmp["error"]) + rmp["grad"] * rmp["dp"]), d64


def _extended(M):
    """a matrix of mpmath (or float) numbers in extended precision: the double nearest to x plus the double nearest to the rest"""
    out = np.zeros(np.shape(M), dtype=np.longdouble)
    for idx, x in np.ndenumerate(np.asarray(M, dtype=object)):
        hi = float(x)
        out[idx] = np.longdouble(hi) + np.longdouble(float(x - hi))
    return out


def hessian_distance(block, m, ncols, ref):
    """|[A b]'[A b] - H|_F for a column-major m x ncols block and a reference dict: the product and the difference are taken
    in extended precision (64-bit significands), so that the comparison adds nothing at the scale of the bounds"""
    if "H_ext" not in ref:
        ref["H_ext"] = _extended(ref["H"])
    Ab = np.asarray(block, dtype=np.longdouble).reshape(ncols, m).T
    D = Ab.T @ Ab - ref["H_ext"]
    return float(np.sqrt(np.sum(D * D)))
