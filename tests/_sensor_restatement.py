"""Numpy restatement of the factor forms that carry a sensor-in-body pose and of the self-calibration camera factor, written
from the reference's source lines, not from the device code:

  GSX_F_PROJECTION with 19 measurement doubles   GenericProjectionFactor, the if(body_P_sensor_) branch
                                                 (gtsam/slam/ProjectionFactor.h:138-166)
  GSX_F_STEREO with 21                           GenericStereoFactor, the same branch (gtsam/slam/StereoFactor.h:126-154)
  GSX_F_RANGE with 13 (Pose3) / 4 (Pose2)        RangeFactorWithTransform (gtsam/sam/RangeFactor.h:104-150)
  GSX_F_SFM2                                     GeneralSFMFactor2<Cal3_S2> (gtsam/slam/GeneralSFMFactor.h:208-278)

and, because the graphs of tests/test_gpu_sensor_factors.py mix them with those, of the plain GSX_F_PROJECTION, GSX_F_SFM
and GSX_F_BEARINGRANGE (and a prior on a camera) that tests/_factor_restatement.py leaves to the CPU oracle.  Everything
else is tests/_factor_restatement.py's: its Lie groups, its plain range / stereo measurements, its whitening, [A b], graph error and dense system, handed this module's
`evaluate` (which falls through to its `evaluate` for the plain forms).

A sensor form evaluates the plain measurement at pose.compose(body_P_sensor) and multiplies the pose Jacobian from the
right by H0 = D compose / D pose = AdjointMap(body_P_sensor^-1) (Lie-group compose, gtsam/base/Lie.h; Pose3.cpp:61-75,
Pose2.cpp:127-135, 202-204); the second key's Jacobian is the plain one at the composed pose.

WRONG: names of terms to get deliberately wrong — tests/test_host_sensor_factors.py sizes its derivative bound by what
these do: "adjoint_translation" drops the [t]x R block of the adjoint, "dcal_skew" the skew column of Dcal."""
import functools
import math

import numpy as np

from gtsam_petercdev_amd import _abi as A
from tests import _factor_restatement as R

F_SFM2 = A.F_SFM2
PLAIN_LEN = {A.F_PROJECTION: 7, A.F_STEREO: 9, A.F_RANGE: 1}
WRONG = set()


# ---- compose with the sensor pose ------------------------------------------------------------------------------------
def pose3_compose(pose, sensor):
    """(pose * sensor as a state, H0 = AdjointMap(sensor^-1)); Pose3 operator* = (R1 R2, t1 + R1 t2)."""
    Rp, tp = R.pose3_of(pose)
    Rs, ts = R.pose3_of(sensor)
    H0 = R.pose3_adjoint(Rs.T, -Rs.T @ ts)         # Pose3::inverse (Pose3.cpp:61-64), AdjointMap (:69-75)
    if "adjoint_translation" in WRONG:
        H0[3:, :3] = 0.0
    return R.pose3_state(Rp @ Rs, tp + Rp @ ts), H0


def pose2_compose(pose, sensor):
    """(pose * sensor as (x, y, theta), H0 = AdjointMap(sensor^-1)); Pose2 operator* = (r1 r2, t1 + r1 t2), Pose2::inverse
    (Pose2.cpp:202-204) = (r^-1, r^-1 (-t)), AdjointMap of (x, y, c, s) = [c -s y; s c -x; 0 0 1] (:127-135)."""
    t = np.asarray(pose[:2], float) + R.rot2(pose[2]) @ np.asarray(sensor[:2], float)
    ti = R.rot2(sensor[2]).T @ (-np.asarray(sensor[:2], float))
    c, s = math.cos(-sensor[2]), math.sin(-sensor[2])
    H0 = np.array([[c, -s, ti[1]], [s, c, -ti[0]], [0.0, 0.0, 1.0]])
    if "adjoint_translation" in WRONG:
        H0[:2, 2] = 0.0
    return np.array([t[0], t[1], pose[2] + sensor[2]]), H0


# ---- pinhole cameras -------------------------------------------------------------------------------------------------
def pinhole_pn(pose, point):
    """PinholeBase::project2 (gtsam/geometry/CalibratedCamera.cpp:116-135): q = R' (p - t), cheirality q.z <= 0 (:122),
    pn = q.xy / q.z; Dpose (:27-34), Dpoint (:37-46).  None behind the camera."""
    Rm, t = R.pose3_of(pose)
    q = Rm.T @ (np.asarray(point[:3], float) - t)
    if q[2] <= 0:
        return None
    d = 1.0 / q[2]
    u, v = q[0] * d, q[1] * d
    Dpose = np.array([[u * v, -1 - u * u, v, -d, 0.0, d * u], [1 + v * v, -u * v, -u, 0.0, -d, d * v]])
    Rt = Rm.T
    Dpoint = d * np.array([Rt[0] - u * Rt[2], Rt[1] - v * Rt[2]])
    return np.array([u, v]), Dpose, Dpoint


def s2_project(pose, point, K):
    """PinholeCamera<Cal3_S2>::project = Cal3_S2::uncalibrate (gtsam/geometry/Cal3_S2.cpp:54-62) of project2: (u, v) =
    (fx x + s y + u0, fy y + v0), Dcal = [x 0 y 1 0; 0 y 0 0 1], Dp = [fx s; 0 fy].  K = (fx, fy, s, u0, v0).
    (pi, Dpose 2x6, Dpoint 2x3, Dcal 2x5) or None."""
    res = pinhole_pn(pose, point)
    if res is None:
        return None
    (x, y), Dpose, Dpoint = res
    fx, fy, s, u0, v0 = K
    Dp = np.array([[fx, s], [0.0, fy]])
    Dcal = np.array([[x, 0.0, y, 1.0, 0.0], [0.0, y, 0.0, 0.0, 1.0]])
    if "dcal_skew" in WRONG:
        Dcal[:, 2] = 0.0
    return np.array([fx * x + s * y + u0, fy * y + v0]), Dp @ Dpose, Dp @ Dpoint, Dcal


def bundler_project(cam, point):
    """PinholeCamera<Cal3Bundler>::project2: Cal3Bundler::uncalibrate (gtsam/geometry/Cal3Bundler.cpp:64-90) of project2;
    cam = R9 t3 (f, k1, k2, u0, v0).  (pi, Dcamera 2x9, Dpoint 2x3) or None."""
    res = pinhole_pn(cam[:12], point)
    if res is None:
        return None
    (x, y), Dpose, Dpoint = res
    f, k1, k2, u0, v0 = cam[12:17]
    r = x * x + y * y
    g = 1 + (k1 + k2 * r) * r
    Dcal = np.array([[g * x, f * r * x, f * r * r * x], [g * y, f * r * y, f * r * r * y]])
    a = 2 * (k1 + 2 * k2 * r)
    Dp = np.array([[f * (g + a * x * x), f * a * x * y], [f * a * x * y, f * (g + a * y * y)]])
    return np.array([u0 + f * g * x, v0 + f * g * y]), np.hstack([Dp @ Dpose, Dcal]), Dp @ Dpoint


# ---- factors ---------------------------------------------------------------------------------------------------------
def has_sensor(arr, f):
    ftype, _, z = R.factor_parts(arr, f)
    return ftype in PLAIN_LEN and len(z) > PLAIN_LEN[ftype]


def evaluate(arr, values, f):
    """(e, [H per key], cheirality) of factor f at the packed `values`: the contract of _factor_restatement.evaluate."""
    so = arr.state_offsets()
    ftype, vs, z = R.factor_parts(arr, f)
    st = [values[so[v]:so[v + 1]] for v in vs]
    vt = [int(arr.var_types[v]) for v in vs]
    if ftype == F_SFM2:         # GeneralSFMFactor2::evaluateError (GeneralSFMFactor.h:264-278): zero behind the camera
        res = s2_project(st[0], st[1], st[2])
        if res is None:
            return np.zeros(2), [np.zeros((2, 6)), np.zeros((2, 3)), np.zeros((2, 5))], True
        return res[0] - z[:2], [res[1], res[2], res[3]], False
    if ftype == A.F_SFM:        # GeneralSFMFactor::evaluateError (GeneralSFMFactor.h:127-158): zero behind the camera
        res = bundler_project(st[0], st[1])
        if res is None:
            return np.zeros(2), [np.zeros((2, 9)), np.zeros((2, 3))], True
        return res[0] - z[:2], [res[1], res[2]], False
    if ftype == A.F_BEARINGRANGE:  # BearingRangeFactor (gtsam/sam/BearingRangeFactor.h): the bearing row over the range row
        th, B1, B2 = R.bearing_pose2(st[0], st[1])
        r, R1, R2 = R.range_pose2(st[0], st[1], False)
        return np.array([R.wrap(th - z[0]), r - z[1]]), [np.vstack([B1, R1]), np.vstack([B2, R2])], False
    if ftype == A.F_PRIOR and vt[0] == A.VAR_CAMERA:   # PriorFactor on a PinholeCamera<Cal3Bundler>: the pose's local
        Rx, tx = R.pose3_of(st[0])                     # coordinates, then the difference of (f, k1, k2) (PinholeCamera.h:206-211)
        Rz, tz = R.pose3_of(z)
        loc = np.concatenate([R.pose3_logmap(Rx.T @ Rz, Rx.T @ (tz - tx)), z[12:15] - st[0][12:15]])
        return -loc, [np.eye(9)], False
    sensor = has_sensor(arr, f)
    if ftype == A.F_PROJECTION:  # GenericProjectionFactor::evaluateError (ProjectionFactor.h:138-166): 2 fx behind it
        pose, H0 = pose3_compose(st[0], z[7:19]) if sensor else (st[0], None)
        res = s2_project(pose, st[1], z[2:7])
        if res is None:
            return np.full(2, 2.0 * z[2]), [np.zeros((2, 6)), np.zeros((2, 3))], True
        return res[0] - z[:2], [res[1] @ H0 if sensor else res[1], res[2]], False
    if not sensor:
        return R.evaluate(arr, values, f)
    if ftype == A.F_STEREO:     # GenericStereoFactor::evaluateError (StereoFactor.h:126-154), the body_P_sensor branch
        pose, H0 = pose3_compose(st[0], z[9:21])
        res = R.stereo_project(pose, st[1], z[3:9])
        if res is None:
            return np.full(3, 2.0 * z[3]), [np.zeros((3, 6)), np.zeros((3, 3))], True
        return res[0] - z[:3], [res[1] @ H0, res[2]], False
    assert ftype == A.F_RANGE   # RangeFactorWithTransform::expression (RangeFactor.h:131-138): Range(Compose(a1, S), a2)
    other_is_pose = vt[1] != A.VAR_VECTOR
    if vt[0] == A.VAR_POSE2:
        pose, H0 = pose2_compose(st[0], z[1:4])
        r, H1, H2 = R.range_pose2(pose, st[1], other_is_pose)
    else:
        pose, H0 = pose3_compose(st[0], z[1:13])
        r, H1, H2 = R.range_pose3(pose, st[1], other_is_pose)
    return np.array([r - z[0]]), [(H1 @ H0).reshape(1, -1), H2.reshape(1, -1)], False


linearized = functools.partial(R.linearized, evaluate=evaluate)
jacobians = functools.partial(R.jacobians, evaluate=evaluate)
factor_error = functools.partial(R.factor_error, evaluate=evaluate)
graph_error = functools.partial(R.graph_error, evaluate=evaluate)
dense_system = functools.partial(R.dense_system, evaluate=evaluate)


# ---- graph builders shared by the host and the device tests ---------------------------------------------------------
VARIANTS = ("projection_sensor", "stereo_sensor", "range_pose2_point2_sensor", "range_pose2_pose2_sensor",
            "range_pose3_point3_sensor", "range_pose3_pose3_sensor", "sfm2")
K_S2 = (520.0, 480.0, 1.5, 320.0, 240.0)


def random_sensor3(rng):
    """A sensor pose with a rotation far from the identity (an angle between 1 and 2.5 rad) and an offset of up to 0.5 m."""
    w = rng.normal(0, 1, 3)
    return R.pose3_state(R.so3_expmap(w / np.linalg.norm(w) * rng.uniform(1.0, 2.5)), rng.uniform(-0.5, 0.5, 3))


def random_sensor2(rng):
    return np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(1.0, 2.5) * rng.choice([-1.0, 1.0])])


def body_of(camera, sensor):
    """The body pose X S^-1 whose composition with `sensor` is `camera` (Pose3 states)."""
    Rc, tc = R.pose3_of(camera)
    Rs, ts = R.pose3_of(sensor)
    Rb = Rc @ Rs.T
    return R.pose3_state(Rb, tc - Rb @ ts)


def random_graph(variant, n_factors, noise, seed):
    """`n_factors` factors of one variant, a different random sensor pose per factor.  Camera variants: the body poses are
    such that the composed camera sees its landmark at a depth of 4 to 9 (no factor in the cheirality branch); the
    measurements are off by 20 px a coordinate, for the reason tests/_factor_restatement.random_graph gives."""
    rng = np.random.default_rng(seed)
    if variant.startswith("range"):
        base = variant[:-len("_sensor")]
        arr = R.random_graph(base, n_factors, noise, seed)
        three_d = "pose3" in base
        meas, ptr = [], [0]
        for f in range(arr.n_factors):
            s = random_sensor3(rng) if three_d else random_sensor2(rng)
            meas += [0.0] + list(s)
            ptr.append(len(meas))
        arr = A.ProblemArrays(var_keys=arr.var_keys, var_types=arr.var_types, var_dims=arr.var_dims, f_type=arr.f_type,
                              f_rows=arr.f_rows, f_key_ptr=arr.f_key_ptr, f_vars=arr.f_vars, f_meas_ptr=ptr,
                              meas=np.array(meas), f_noise_kind=arr.f_noise_kind, f_noise_ptr=arr.f_noise_ptr,
                              noise=arr.noise, values=arr.values)
        for f in range(arr.n_factors):   # the measured range: the true one from the sensor, 0.3 m of noise
            arr.meas[arr.f_meas_ptr[f]] = evaluate(arr, arr.values, f)[0][0] + rng.normal(0, 0.3)
        return arr
    n_l = max(6, n_factors // 3)
    points = [rng.uniform(-8, 8, 3) for _ in range(n_l)]
    var_list, values, factors = [], [], []
    calib = variant == "sfm2"
    for f in range(n_factors):           # a body pose per factor: its camera looks at the landmark from a random side
        j = f % n_l if f < n_l else int(rng.integers(n_l))
        Rc = R.random_rot3(rng, 1.2)
        cam = R.pose3_state(Rc, points[j] - Rc @ np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), rng.uniform(4.0, 9.0)]))
        sensor = random_sensor3(rng)
        var_list.append((f, A.VAR_POSE3, 6))
        values.append(cam if calib else body_of(cam, sensor))
        if variant == "stereo_sensor":
            z = R.stereo_project(cam, points[j], R.STEREO_K)[0] + rng.normal(0, 20.0, 3)
            ftype, m, meas, keys = A.F_STEREO, 3, np.concatenate([z, R.STEREO_K, sensor]), [f, n_factors + j]
        elif variant == "projection_sensor":
            z = s2_project(cam, points[j], K_S2)[0] + rng.normal(0, 20.0, 2)
            ftype, m, meas, keys = A.F_PROJECTION, 2, np.concatenate([z, K_S2, sensor]), [f, n_factors + j]
        else:
            z = s2_project(cam, points[j], K_S2)[0] + rng.normal(0, 20.0, 2)
            ftype, m, meas, keys = F_SFM2, 2, z, [f, n_factors + j, n_factors + n_l]
        kind, params = R.noise_of(rng, noise, m)
        factors.append((ftype, keys, m, meas, kind, params))
    var_list += [(1000000 + j, A.VAR_VECTOR, 3) for j in range(n_l)]
    values += points
    if calib:
        var_list.append((2000000, A.VAR_VECTOR, 5))
        values.append(np.array(K_S2) + np.array([3.0, -2.0, 0.2, 1.0, -1.0]))
    return R.make_arrays(var_list, factors, np.concatenate(values))


def selfcal_graph(n_poses, n_points, seed, obs_of_point=None, sigma=1.0, perturb=0.05):
    """A self-calibration graph in the manner of examples/SelfCalibrationExample.cpp: cameras on a circle looking at the
    origin, points near it, exact measurements with K = (50, 50, 0, 50, 50), GeneralSFMFactor2 between each observing pose,
    point and the one K; priors on the first pose, the first point and K; values perturbed from the truth.
    obs_of_point(j) -> the poses that see point j (default: all)."""
    rng = np.random.default_rng(seed)
    K = np.array([50.0, 50.0, 0.0, 50.0, 50.0])
    poses = []
    for i in range(n_poses):
        th = 2 * math.pi * i / n_poses
        c = np.array([30 * math.cos(th), 30 * math.sin(th), 1.2 + 0.1 * i])
        zc = -c / np.linalg.norm(c)
        xc = np.cross(np.array([0.0, 0.0, 1.0]), zc)
        xc /= np.linalg.norm(xc)
        poses.append(R.pose3_state(np.column_stack([xc, np.cross(zc, xc), zc]), c))
    points = [rng.uniform(-10, 10, 3) for _ in range(n_points)]
    var_list = [(i, A.VAR_POSE3, 6) for i in range(n_poses)] + [(1000 + j, A.VAR_VECTOR, 3) for j in range(n_points)] + \
               [(5000, A.VAR_VECTOR, 5)]
    kv = n_poses + n_points
    factors = [(A.F_PRIOR, [0], 6, poses[0], A.NOISE_DIAGONAL, [0.1] * 3 + [0.3] * 3),
               (A.F_PRIOR, [n_poses], 3, points[0], A.NOISE_ISOTROPIC, [0.1]),
               (A.F_PRIOR, [kv], 5, K, A.NOISE_DIAGONAL, [500.0, 500.0, 0.1, 100.0, 100.0])]
    for j in range(n_points):
        for i in (obs_of_point(j) if obs_of_point else range(n_poses)):
            z = s2_project(poses[i], points[j], K)[0]
            factors.append((F_SFM2, [i, n_poses + j, kv], 2, z, A.NOISE_ISOTROPIC, [sigma]))
    vals = [R.retract(A.VAR_POSE3, p, perturb * rng.normal(0, 1, 6)) for p in poses] + \
           [p + perturb * 4 * rng.normal(0, 1, 3) for p in points] + [K + np.array([10.0, 10.0, 0.0, 10.0, 10.0]) * perturb * 4]
    return R.make_arrays(var_list, factors, np.concatenate(vals))
