"""50-digit counterpart of tests/_sensor_restatement.py: the sensor forms of GSX_F_PROJECTION / _STEREO / _RANGE and
GSX_F_SFM2 in the arithmetic, and under the rules, of tests/_mp_restatement.py (mpmath at DPS digits, branches decided on
float64 as the reference decides them, rounded to float64 at the very end), written from the same reference lines.  The
plain forms fall through to tests/_mp_restatement.evaluate_mp."""
import functools

import mpmath as mp
import numpy as np

from gtsam_petercdev_amd import _abi as A
from tests import _factor_restatement as R
from tests import _mp_restatement as M

PLAIN_LEN = {A.F_PROJECTION: 7, A.F_STEREO: 9, A.F_RANGE: 1}


def matmul(P, Q):
    return [[mp.fsum(P[i][k] * Q[k][j] for k in range(len(Q))) for j in range(len(Q[0]))] for i in range(len(P))]


def pose3_compose_sensor(pose, sensor):
    """(pose * sensor as a state, H0 = AdjointMap(sensor^-1)) — compose's Jacobian in its first argument (gtsam/base/Lie.h;
    Pose3.cpp:61-75)."""
    S = M.pose3_of(sensor)
    return M.pose3_state(M.pose3_compose(M.pose3_of(pose), S)), M.pose3_adjoint(M.pose3_inverse(S))


def pose2_compose_sensor(pose, sensor):
    """((x, y, c, s) of pose * sensor, H0 = AdjointMap(sensor^-1)) (Pose2.cpp:127-135, 202-204)."""
    S = M.pose2_cs(sensor)
    return M.pose2_compose_cs(M.pose2_cs(pose), S), M.pose2_adjoint_cs(M.pose2_inverse_cs(S))


def range_2d_cs(pose, other, other_is_pose):
    """Pose2::range (Pose2.cpp:271-310) at a pose held as (x, y, c, s)."""
    d = [other[0] - pose[0], other[1] - pose[1]]
    r, D = M.norm_with_derivative(d)
    c, s = pose[2], pose[3]
    H1 = [-D[0] * c - D[1] * s, D[0] * s - D[1] * c, mp.mpf(0)]
    if other_is_pose:
        c2, s2 = mp.cos(other[2]), mp.sin(other[2])
        H2 = [D[0] * c2 + D[1] * s2, -D[0] * s2 + D[1] * c2, mp.mpf(0)]
    else:
        H2 = D
    return r, H1, H2


def s2_project_cal(pose, point, K, want_H=True):
    """PinholeCamera<Cal3_S2>::project with Dcal = [x 0 y 1 0; 0 y 0 0 1] (gtsam/geometry/Cal3_S2.cpp:54-62)."""
    res = M.s2_project(pose, point, K, want_H)
    if res is None or not want_H:
        return res if res is None else (res[0], None, None, None)
    (x, y), _, _ = M.pinhole_pn(M.pose3_of(M.vec(pose)), M.vec(point), False)
    z, o = mp.mpf(0), mp.mpf(1)
    return res[0], res[1], res[2], [[x, z, y, o, z], [z, y, z, z, o]]


def evaluate_mp(ftype, vt, st, z, want_H=True):
    """(e, [H per key] or None, cheirality) in high precision: tests/_mp_restatement.evaluate_mp, extended."""
    if ftype == A.F_SFM2:       # GeneralSFMFactor2 (gtsam/slam/GeneralSFMFactor.h:264-278): zero behind the camera
        st, z = [M.vec(s) for s in st], M.vec(z)
        res = s2_project_cal(st[0], st[1], st[2], want_H)
        if res is None:
            return [mp.mpf(0)] * 2, [M.zeros(2, 6), M.zeros(2, 3), M.zeros(2, 5)], True
        return M.sub(res[0], z), [res[1], res[2], res[3]], False
    if ftype not in PLAIN_LEN or len(z) == PLAIN_LEN[ftype]:
        return M.evaluate_mp(ftype, vt, st, z, want_H)
    st, z = [M.vec(s) for s in st], M.vec(z)
    n = PLAIN_LEN[ftype]
    if ftype == A.F_RANGE and vt[0] == A.VAR_POSE2:   # RangeFactorWithTransform (gtsam/sam/RangeFactor.h:131-138)
        pose, H0 = pose2_compose_sensor(st[0], z[1:4])
        r, H1, H2 = range_2d_cs(pose, st[1], vt[1] != A.VAR_VECTOR)
        return [r - z[0]], [matmul([H1], H0), [H2]], False
    pose, H0 = pose3_compose_sensor(st[0], z[n:n + 12])
    if ftype == A.F_RANGE:
        r, H1, H2 = M.range_3d(pose, st[1], vt[1] != A.VAR_VECTOR)
        return [r - z[0]], [matmul([H1], H0), [H2]], False
    if ftype == A.F_PROJECTION:  # ProjectionFactor.h:138-166, the if(body_P_sensor_) branch: *H1 = *H1 * H0
        res, m = M.s2_project(pose, st[1], z[2:7], want_H), 2
    else:                        # StereoFactor.h:126-154, the same branch
        res, m = M.stereo_project(pose, st[1], z[3:9], want_H), 3
    if res is None:
        return [2 * z[m]] * m, [M.zeros(m, 6), M.zeros(m, 3)], True
    return M.sub(res[0], z[:m]), [matmul(res[1], H0) if want_H else None, res[2]], False


def evaluate(arr, values, f):
    e, Hs, cheir = evaluate_mp(*M.factor_inputs(arr, values, f))
    return M.to_f64(e), [np.array([[float(x) for x in row] for row in H], dtype=float) for H in Hs], cheir


def true_jacobians(arr, values, f, step="1e-20"):
    """Central differences of the 50-digit error in the variables' tangent spaces (tests/_mp_restatement.true_jacobians on
    this module's evaluate_mp)."""
    ftype, vt, st, z = M.factor_inputs(arr, values, f)
    h = mp.mpf(step)
    _, vs, _ = R.factor_parts(arr, f)
    out = []
    for k, v in enumerate(vs):
        d = int(arr.var_dims[v])
        cols = []
        for j in range(d):
            es = []
            for sgn in (1, -1):
                dx = [mp.mpf(0)] * d
                dx[j] = sgn * h
                moved = list(st)
                moved[k] = M.retract_mp(vt[k], st[k], dx)
                es.append(evaluate_mp(ftype, vt, moved, z, want_H=False)[0])
            cols.append([(a - b) / (2 * h) for a, b in zip(*es)])
        out.append(np.array([[float(cols[j][i]) for j in range(d)] for i in range(len(cols[0]))], dtype=float))
    return out


linearized = functools.partial(R.linearized, evaluate=evaluate)
jacobians = functools.partial(R.jacobians, evaluate=evaluate)
factor_error = functools.partial(R.factor_error, evaluate=evaluate)
graph_error = functools.partial(R.graph_error, evaluate=evaluate)
dense_system = functools.partial(R.dense_system, evaluate=evaluate)
