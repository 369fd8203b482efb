"""50-digit restatement of every factor, error and retract the device computes, written from the reference's source lines
(cited as file:line, paths relative to the reference tree) and NOT from csrc/device_geometry.h or oracle/geometry.h: the
judge tests/test_gpu_kernel_edges.py holds the kernels against, itself pinned by tests/test_host_restatement.py with the
reference's known answers, the closed-form exponential / logarithm and true derivatives.

Rules.  The arithmetic is mpmath at DPS digits.  A BRANCH is taken as the reference takes it, on float64: the quantity that
decides is rounded to float64 (a trace is summed in float64 from the rounded entries, as Eigen sums it) and compared with the
reference's constant; only the arithmetic inside the branch is high precision.  Results are rounded to float64 at the very
end (`evaluate`, `retract`, `local`).  Vectors are lists of mpf, 3x3 matrices lists of rows; a Pose3 is (R, t), a Pose2
(x, y, theta), a camera (R, t, [f, k1, k2, u0, v0]).

Whitening, the robust losses, [A b], the graph error and the dense system are those of tests/_factor_restatement.py, handed
this module's `evaluate`."""
import functools

import mpmath as mp
import numpy as np

from gtsam_petercdev_amd import _abi as A
from tests import _factor_restatement as R

DPS = 50
mp.mp.dps = DPS
PI = mp.pi


def vec(x):
    return [mp.mpf(float(a)) if not isinstance(a, mp.mpf) else a for a in x]


def mat3(x):
    return [vec(row) for row in np.asarray(x, dtype=object).reshape(3, 3).tolist()]


def eye3():
    return [[mp.mpf(int(i == j)) for j in range(3)] for i in range(3)]


def mm(P, Q):
    return [[mp.fsum(P[i][k] * Q[k][j] for k in range(len(Q))) for j in range(len(Q[0]))] for i in range(len(P))]


def mv(P, v):
    return [mp.fsum(P[i][k] * v[k] for k in range(len(v))) for i in range(len(P))]


def tr3(P):
    return [[P[j][i] for j in range(3)] for i in range(3)]


def add(a, b):
    return [x + y for x, y in zip(a, b)]


def sub(a, b):
    return [x - y for x, y in zip(a, b)]


def scal(s, a):
    return [s * x for x in a]


def dot(a, b):
    return mp.fsum(x * y for x, y in zip(a, b))


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def skew(w):
    """skewSymmetric (gtsam/base/Matrix.h)."""
    z = mp.mpf(0)
    return [[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]]


def lin(*terms):
    """sum of coefficient * 3x3 matrix."""
    return [[mp.fsum(c * M[i][j] for c, M in terms) for j in range(3)] for i in range(3)]


# ---- SO(3) -----------------------------------------------------------------------------------------------------------
def dexp_functor(w, near_zero=None):
    """so3::ExpmapFunctor / DexpFunctor (gtsam/geometry/SO3.cpp:61-112): (A, B, C, nearZero).  nearZero is the caller's
    flag or theta2 <= epsilon (:62-63); the Taylor forms are second order (:73-74, :107)."""
    theta2 = dot(w, w)
    near = bool(near_zero) or float(theta2) <= np.finfo(float).eps
    if not near:
        theta = mp.sqrt(theta2)
        a = mp.sin(theta) / theta                              # :66
        s2 = mp.sin(theta / 2)
        b = 2 * s2 * s2 / theta2                               # :67-70
        c = (1 - a) / theta2                                   # :100
    else:
        a = 1 - theta2 / 6                                     # :73
        b = mp.mpf(1) / 2 - theta2 / 24                        # :74
        c = mp.mpf(1) / 6 - theta2 / 120                       # :107
    return a, b, c, near


def so3_expmap(w, near_zero=None):
    """ExpmapFunctor::expmap (SO3.cpp:95): I + A W + B W W."""
    a, b, _, _ = dexp_functor(w, near_zero)
    W = skew(w)
    return lin((1, eye3()), (a, W), (b, mm(W, W)))


def trace64(Rm):
    """R.trace() as float64 arithmetic sees it: the branch variable of SO3::Logmap."""
    return (float(Rm[0][0]) + float(Rm[1][1])) + float(Rm[2][2])


def so3_logmap_branch(Rm):
    """'pi' + the index of the largest diagonal entry (SO3.cpp:316-356), 'normal' (:360-363) or 'taylor' (:364-369)."""
    tr = trace64(Rm)
    if tr + 1.0 < 1e-3:
        d = [float(Rm[i][i]) for i in range(3)]
        if d[2] > d[1] and d[2] > d[0]:
            return "pi2"
        return "pi1" if d[1] > d[0] else "pi0"
    return "normal" if tr - 3.0 < -1e-6 else "taylor"


def so3_logmap(Rm):
    """SO3::Logmap (gtsam/geometry/SO3.cpp:299-375), every branch.  Near pi (:316-356) with a the largest diagonal entry
    and (a, b, c) cyclic: W = R_cb - R_bc, Q1 = 2 + 2 R_aa, Q2 = R_ab + R_ba, Q3 = R_ca + R_ac, omega_a, omega_b, omega_c =
    sgn(W) (pi - 2 |W| / |(Q1, Q2, Q3, W)|) / (2 sqrt(Q1)) (Q1, Q2, Q3) — the three written-out cases of the source
    (:317-329 a = 3; :330-342 a = 2; :343-355 a = 1), sgn(0) = +1 (:326)."""
    branch = so3_logmap_branch(Rm)
    if branch.startswith("pi"):
        a = int(branch[2])
        b, c = (a + 1) % 3, (a + 2) % 3
        W = Rm[c][b] - Rm[b][c]
        Q1 = 2 + 2 * Rm[a][a]
        Q2 = Rm[a][b] + Rm[b][a]
        Q3 = Rm[c][a] + Rm[a][c]
        norm = mp.sqrt(Q1 * Q1 + Q2 * Q2 + Q3 * Q3 + W * W)
        sgn = -1 if W < 0 else 1
        magn = PI - (2 * sgn * W) / norm
        scale = sgn * magn / (2 * mp.sqrt(Q1))
        om = [None] * 3
        om[a], om[b], om[c] = scale * Q1, scale * Q2, scale * Q3
        return om
    tr = Rm[0][0] + Rm[1][1] + Rm[2][2]
    if branch == "normal":
        theta = mp.acos((tr - 1) / 2)                          # :362
        magn = theta / (2 * mp.sin(theta))                     # :363
    else:
        t3 = tr - 3
        magn = mp.mpf(1) / 2 - t3 / 12 + t3 * t3 / 60          # :368
    return [magn * (Rm[2][1] - Rm[1][2]), magn * (Rm[0][2] - Rm[2][0]), magn * (Rm[1][0] - Rm[0][1])]   # :370


# ---- SE(3) -----------------------------------------------------------------------------------------------------------
def pose3_of(s):
    s = vec(s)
    return [s[0:3], s[3:6], s[6:9]], s[9:12]


def pose3_state(p):
    return [x for row in p[0] for x in row] + list(p[1])


def pose3_compose(p, q):
    """Pose3 operator* (gtsam/geometry/Pose3.h): (R1 R2, t1 + R1 t2)."""
    return mm(p[0], q[0]), add(p[1], mv(p[0], q[1]))


def pose3_inverse(p):
    """Pose3::inverse (gtsam/geometry/Pose3.cpp:61-64): (R', R' (-t))."""
    Rt = tr3(p[0])
    return Rt, mv(Rt, scal(-1, p[1]))


def pose3_between(p, q):
    return pose3_compose(pose3_inverse(p), q)


def pose3_adjoint(p):
    """Pose3::AdjointMap (Pose3.cpp:69-75): [R 0; [t]x R, R]."""
    Rm, t = p
    TR = mm(skew(t), Rm)
    z = mp.mpf(0)
    return [list(Rm[i]) + [z, z, z] for i in range(3)] + [list(TR[i]) + list(Rm[i]) for i in range(3)]


def pose3_expmap(xi):
    """Pose3::Expmap (Pose3.cpp:184-222): nearZero = w.w <= 1e-5 (:189) handed to the functor; t = applyLeftJacobian(v) =
    v + B w x v + C w x (w x v) (SO3.cpp:165-174, :114-139)."""
    xi = vec(xi)
    w, v = xi[:3], xi[3:]
    near = float(dot(w, w)) <= 1e-5
    _, b, c, _ = dexp_functor(w, near)
    wv = cross(w, v)
    return so3_expmap(w, near), add(add(v, scal(b, wv)), scal(c, cross(w, wv)))


def pose3_logmap(p):
    """Pose3::Logmap (Pose3.cpp:225-245)."""
    w = so3_logmap(p[0])
    T = p[1]
    t = mp.sqrt(dot(w, w))
    if float(t) < 1e-10:                                       # :230
        return w + list(T)
    W = skew(scal(1 / t, w))                                   # :235
    WT = mv(W, T)
    u = add(sub(T, scal(t / 2, WT)), scal(1 - t / (2 * mp.tan(t / 2)), mv(W, WT)))   # :238-240
    return w + u


# ---- SE(2) -----------------------------------------------------------------------------------------------------------
def rot2_normalize(c, s):
    """Rot2::normalize (gtsam/geometry/Rot2.cpp:56-64)."""
    scale = c * c + s * s
    if abs(float(scale) - 1.0) > 1e-10:
        k = 1 / mp.sqrt(scale)
        c, s = c * k, s * k
    return c, s


def pose2_cs(p):
    """(x, y, c, s) of a Pose2 state: Rot2::fromAngle (Rot2.h)."""
    return p[0], p[1], mp.cos(p[2]), mp.sin(p[2])


def pose2_compose_cs(a, b):
    """Pose2 operator* (gtsam/geometry/Pose2.h): (r1 * r2, t1 + r1 * t2); Rot2 operator* = fromCosSin(c1 c2 - s1 s2,
    s1 c2 + c1 s2) (Rot2.h), which normalizes (Rot2.cpp:27-30)."""
    c, s = rot2_normalize(a[2] * b[2] - a[3] * b[3], a[3] * b[2] + a[2] * b[3])
    return a[0] + a[2] * b[0] - a[3] * b[1], a[1] + a[3] * b[0] + a[2] * b[1], c, s   # Rot2::rotate, Rot2.cpp:100-106


def pose2_inverse_cs(a):
    """Pose2::inverse (gtsam/geometry/Pose2.cpp:202-204): (r^-1, r.unrotate(-t)); unrotate Rot2.cpp:110-116."""
    tx, ty = -a[0], -a[1]
    return a[2] * tx + a[3] * ty, -a[3] * tx + a[2] * ty, a[2], -a[3]


def pose2_chart(a):
    """Pose2::ChartAtOrigin::Local with the default GTSAM_SLOW_BUT_CORRECT_EXPMAP off (Pose2.cpp:112-122):
    (x, y, theta), theta = atan2(s, c) (Rot2.h)."""
    return [a[0], a[1], mp.atan2(a[3], a[2])]


def pose2_between(a, b):
    """Local(a, b) = chart(a^-1 b) of two (x, y, theta) states."""
    return pose2_chart(pose2_compose_cs(pose2_inverse_cs(pose2_cs(vec(a))), pose2_cs(vec(b))))


def pose2_adjoint_cs(a):
    """Pose2::AdjointMap (Pose2.cpp:127-135)."""
    return [[a[2], -a[3], a[1]], [a[3], a[2], -a[0]], [mp.mpf(0), mp.mpf(0), mp.mpf(1)]]


# ---- charts of the variable types ------------------------------------------------------------------------------------
def retract_mp(vtype, state, d):
    """traits<T>::Retract in high precision, state in / state out.  VECTOR: x + d.  POSE2: x * (dx, dy, dtheta)
    (Pose2::ChartAtOrigin::Retract, Pose2.cpp:100-110), the angle read back through atan2 as a Rot2 hands it out.  POSE3:
    x * Expmap(d) (Pose3.cpp:248-250, GTSAM_POSE3_EXPMAP).  CAMERA: PinholeCamera::retract (PinholeCamera.h:197-203) =
    pose 6 + Cal3Bundler::retract (f + d6, k1 + d7, k2 + d8; u0, v0 carried: Cal3Bundler.h:134-136)."""
    state, d = vec(state), vec(d)
    if vtype == A.VAR_VECTOR:
        return add(state, d)
    if vtype == A.VAR_POSE2:
        return pose2_chart(pose2_compose_cs(pose2_cs(state), pose2_cs(d)))
    out = pose3_state(pose3_compose(pose3_of(state), pose3_expmap(d[:6])))
    if vtype == A.VAR_CAMERA:
        out += [state[12] + d[6], state[13] + d[7], state[14] + d[8], state[15], state[16]]
    return out


def local_mp(vtype, x, y):
    """traits<T>::Local(x, y) = chart(x^-1 y); CAMERA: PinholeCamera::localCoordinates (PinholeCamera.h:206-211) with
    Cal3Bundler::localCoordinates = the difference of (f, k1, k2) (Cal3Bundler.h:139-141)."""
    x, y = vec(x), vec(y)
    if vtype == A.VAR_VECTOR:
        return sub(y, x)
    if vtype == A.VAR_POSE2:
        return pose2_between(x, y)
    out = pose3_logmap(pose3_between(pose3_of(x), pose3_of(y)))
    if vtype == A.VAR_CAMERA:
        out += [y[12] - x[12], y[13] - x[13], y[14] - x[14]]
    return out


def to_f64(x):
    return np.array([float(a) for a in x], dtype=float)


def retract(vtype, state, d):
    return to_f64(retract_mp(vtype, state, d))


def local(vtype, x, y):
    return to_f64(local_mp(vtype, x, y))


def retract_values(arr, values, delta):
    """Values::retract (gtsam/nonlinear/Values.cpp:53-64) of the packed values by the packed tangent vector."""
    so, to = arr.state_offsets(), arr.tangent_offsets()
    return np.concatenate([retract(int(arr.var_types[v]), values[so[v]:so[v + 1]], delta[to[v]:to[v + 1]])
                           for v in range(arr.n_vars)])


# ---- cameras ---------------------------------------------------------------------------------------------------------
def pinhole_pn(pose, point, want_H):
    """PinholeBase::project2 (gtsam/geometry/CalibratedCamera.cpp:116-135): q = R' (p - t) (Pose3::transformTo), cheirality
    q.z <= 0 (:122), pn = q.xy / q.z (:88-94); Dpose (:27-34), Dpoint (:37-46, Rt = R').  None behind the camera."""
    Rm, t = pose
    q = mv(tr3(Rm), sub(point, t))
    if float(q[2]) <= 0:
        return None
    d = 1 / q[2]
    u, v = q[0] * d, q[1] * d
    if not want_H:
        return (u, v), None, None
    z = mp.mpf(0)
    Dpose = [[u * v, -1 - u * u, v, -d, z, d * u], [1 + v * v, -u * v, -u, z, -d, d * v]]
    Rt = tr3(Rm)
    Dpoint = [[d * (Rt[0][j] - u * Rt[2][j]) for j in range(3)], [d * (Rt[1][j] - v * Rt[2][j]) for j in range(3)]]
    return (u, v), Dpose, Dpoint


def sfm_project(cam, point, want_H=True):
    """PinholeCamera<Cal3Bundler>::project2 = Cal3Bundler::uncalibrate (gtsam/geometry/Cal3Bundler.cpp:64-90) of
    PinholeBase::project2; Dcamera = [Dpi_pn Dpn_pose, Dcal] (2 x 9), Dpoint = Dpi_pn Dpn_point.  cam: 17 state doubles."""
    cam, point = vec(cam), vec(point)
    res = pinhole_pn(pose3_of(cam[:12]), point, want_H)
    if res is None:
        return None
    (x, y), Dpose, Dpoint = res
    f, k1, k2, u0, v0 = cam[12:17]
    r = x * x + y * y                                          # :70
    g = 1 + (k1 + k2 * r) * r                                  # :71
    pi = [u0 + f * g * x, v0 + f * g * y]                      # :72, :89
    if not want_H:
        return pi, None, None
    Dcal = [[g * x, f * r * x, f * r * r * x], [g * y, f * r * y, f * r * r * y]]          # :78-79
    a = 2 * (k1 + 2 * k2 * r)                                  # :83
    Dp = [[f * (g + a * x * x), f * a * x * y], [f * a * x * y, f * (g + a * y * y)]]       # :84-86
    H1 = [[Dp[i][0] * Dpose[0][j] + Dp[i][1] * Dpose[1][j] for j in range(6)] + Dcal[i] for i in range(2)]
    H2 = [[Dp[i][0] * Dpoint[0][j] + Dp[i][1] * Dpoint[1][j] for j in range(3)] for i in range(2)]
    return pi, H1, H2


def s2_project(pose, point, K, want_H=True):
    """PinholePose<Cal3_S2>::project2: Cal3_S2::uncalibrate (gtsam/geometry/Cal3_S2.cpp:44-50) (u, v) = (fx x + s y + u0,
    fy y + v0), Dp = [fx s; 0 fy], of PinholeBase::project2.  K = (fx, fy, s, u0, v0)."""
    pose, point, K = vec(pose), vec(point), vec(K)
    res = pinhole_pn(pose3_of(pose), point, want_H)
    if res is None:
        return None
    (x, y), Dpose, Dpoint = res
    fx, fy, s, u0, v0 = K
    pi = [fx * x + s * y + u0, fy * y + v0]
    if not want_H:
        return pi, None, None
    H1 = [[fx * Dpose[0][j] + s * Dpose[1][j] for j in range(6)], [fy * Dpose[1][j] for j in range(6)]]
    H2 = [[fx * Dpoint[0][j] + s * Dpoint[1][j] for j in range(3)], [fy * Dpoint[1][j] for j in range(3)]]
    return pi, H1, H2


def stereo_project(pose, point, K, want_H=True):
    """StereoCamera::project2 (gtsam/geometry/StereoCamera.cpp:37-79); K = (fx, fy, s, u0, v0, b), s unused as there."""
    pose, point, K = vec(pose), vec(point), vec(K)
    Rm, t = pose3_of(pose)
    q = mv(tr3(Rm), sub(point, t))
    if float(q[2]) <= 0:
        return None
    fx, fy, _s, u0, v0, b = K
    x, y = q[0], q[1]
    d = 1 / q[2]
    dfx, dfy = d * fx, d * fy
    uL, uR, v = dfx * x, dfx * (x - b), dfy * y
    out = [u0 + uL, u0 + uR, v0 + v]
    if not want_H:
        return out, None, None
    v1 = v / fy
    v2 = fx * v1
    dx = d * x
    z = mp.mpf(0)
    H1 = [[uL * v1, -fx - dx * uL, v2, -dfx, z, d * uL], [uR * v1, -fx - dx * uR, v2, -dfx, z, d * uR],
          [fy + v * v1, -dx * v, -x * dfy, z, -dfy, d * v]]
    H2 = [[d * (fx * Rm[j][0] - Rm[j][2] * uL) for j in range(3)], [d * (fx * Rm[j][0] - Rm[j][2] * uR) for j in range(3)],
          [d * (fy * Rm[j][1] - Rm[j][2] * v) for j in range(3)]]
    return out, H1, H2


# ---- planar and spatial measurements ---------------------------------------------------------------------------------
def norm_with_derivative(p):
    """norm2 / norm3 (gtsam/geometry/Point2.cpp:27-36, Point3.cpp:41-50): the row of ones at r <= 1e-10."""
    r = mp.sqrt(dot(p, p))
    return r, ([x / r for x in p] if abs(float(r)) > 1e-10 else [mp.mpf(1)] * len(p))


def bearing_2d(pose, point):
    """Pose2::bearing (gtsam/geometry/Pose2.cpp:246-257) on Pose2::transformTo (:208-215) and Rot2::relativeBearing
    (Rot2.cpp:119-130, the n <= 1e-5 guard): (angle, H pose 1x3, H point 1x2)."""
    c, s = mp.cos(pose[2]), mp.sin(pose[2])
    dx, dy = point[0] - pose[0], point[1] - pose[1]
    qx, qy = c * dx + s * dy, -s * dx + c * dy
    d2 = qx * qx + qy * qy
    if abs(float(mp.sqrt(d2))) > 1e-5:
        theta, D = mp.atan2(qy, qx), [-qy / d2, qx / d2]
    else:
        theta, D = mp.mpf(0), [mp.mpf(0), mp.mpf(0)]
    # D q / D pose = [-1 0 q.y; 0 -1 -q.x] (:213, Rot2.cpp:113), D q / D point = R' (Rot2.cpp:114)
    H1 = [-D[0], -D[1], D[0] * qy - D[1] * qx]
    H2 = [D[0] * c - D[1] * s, D[0] * s + D[1] * c]
    return theta, H1, H2


def range_2d(pose, other, other_is_pose):
    """Pose2::range (Pose2.cpp:271-310)."""
    d = [other[0] - pose[0], other[1] - pose[1]]
    r, D = norm_with_derivative(d)
    c, s = mp.cos(pose[2]), mp.sin(pose[2])
    H1 = [-D[0] * c - D[1] * s, D[0] * s - D[1] * c, mp.mpf(0)]
    if other_is_pose:
        c2, s2 = mp.cos(other[2]), mp.sin(other[2])
        H2 = [D[0] * c2 + D[1] * s2, -D[0] * s2 + D[1] * c2, mp.mpf(0)]
    else:
        H2 = D
    return r, H1, H2


def range_3d(pose, other, other_is_pose):
    """Pose3::range (gtsam/geometry/Pose3.cpp:408-431) on Pose3::transformTo (:380-397)."""
    Rm, t = pose3_of(pose)
    point = other[9:12] if other_is_pose else other[:3]
    q = mv(tr3(Rm), sub(point, t))
    r, D = norm_with_derivative(q)
    Sq = skew(q)
    H1 = [mp.fsum(D[i] * Sq[i][j] for i in range(3)) for j in range(3)] + [-x for x in D]
    Dpoint = [mp.fsum(D[i] * Rm[j][i] for i in range(3)) for j in range(3)]       # D_r_local R'
    if other_is_pose:
        R2, _ = pose3_of(other)
        H2 = [mp.mpf(0)] * 3 + [mp.fsum(Dpoint[i] * R2[i][j] for i in range(3)) for j in range(3)]
    else:
        H2 = Dpoint
    return r, H1, H2


def wrap(a):
    """Rot2 Local: the angle of fromAngle(a) read back through atan2."""
    return mp.atan2(mp.sin(a), mp.cos(a))


# ---- factors -----------------------------------------------------------------------------------------------------------
def identity(n):
    return [[mp.mpf(int(i == j)) for j in range(n)] for i in range(n)]


def zeros(m, n):
    return [[mp.mpf(0)] * n for _ in range(m)]


def neg(M):
    return [[-x for x in row] for row in M]


def evaluate_mp(ftype, vt, st, z, want_H=True):
    """(e, [H per key] or None, cheirality) of one factor in high precision: the UNWHITENED evaluateError.  vt: the
    variable types, st: their states, z: the factor's measurement doubles."""
    st, z = [vec(s) for s in st], vec(z)
    if ftype == A.F_PRIOR:      # PriorFactor (gtsam/nonlinear/PriorFactor.h:98-102): e = -Local(x, prior), H = I
        loc = local_mp(vt[0], st[0], z)
        return [-x for x in loc], [identity(len(loc))], False
    if ftype == A.F_BETWEEN:    # BetweenFactor (gtsam/slam/BetweenFactor.h:111-124): e = Local(z, x1^-1 x2), H1 =
        if vt[0] == A.VAR_VECTOR:   # -Ad(h^-1), H2 = I (traits::Between; no Logmap derivative by default)
            n = len(st[0])
            return sub(sub(st[1], st[0]), z), [neg(identity(n)), identity(n)], False
        if vt[0] == A.VAR_POSE2:
            h = pose2_compose_cs(pose2_inverse_cs(pose2_cs(st[0])), pose2_cs(st[1]))
            e = pose2_chart(pose2_compose_cs(pose2_inverse_cs(pose2_cs(z)), h))
            return e, [neg(pose2_adjoint_cs(pose2_inverse_cs(h))), identity(3)], False
        h = pose3_between(pose3_of(st[0]), pose3_of(st[1]))
        e = pose3_logmap(pose3_between(pose3_of(z), h))
        return e, [neg(pose3_adjoint(pose3_inverse(h))), identity(6)], False
    if ftype == A.F_SFM:        # GeneralSFMFactor (gtsam/slam/GeneralSFMFactor.h:127-158): h(x) - z; cheirality: zeros
        res = sfm_project(st[0], st[1], want_H)
        if res is None:
            return [mp.mpf(0)] * 2, [zeros(2, 9), zeros(2, 3)], True
        return sub(res[0], z), [res[1], res[2]], False
    if ftype == A.F_PROJECTION:  # GenericProjectionFactor (gtsam/slam/ProjectionFactor.h:138-166): cheirality 2 fx
        res = s2_project(st[0], st[1], z[2:7], want_H)
        if res is None:
            return [2 * z[2]] * 2, [zeros(2, 6), zeros(2, 3)], True
        return sub(res[0], z[:2]), [res[1], res[2]], False
    if ftype == A.F_BEARINGRANGE:  # BearingRangeFactor (gtsam/sam/BearingRangeFactor.h): e = Local(z, h(x))
        th, B1, B2 = bearing_2d(st[0], st[1])
        r, R1, R2 = range_2d(st[0], st[1], False)
        return [wrap(th - z[0]), r - z[1]], [[B1, R1], [B2, R2]], False
    if ftype == A.F_RANGE:      # RangeFactor (gtsam/sam/RangeFactor.h): e = range - z
        other_is_pose = vt[1] != A.VAR_VECTOR
        r, H1, H2 = (range_2d if vt[0] == A.VAR_POSE2 else range_3d)(st[0], st[1], other_is_pose)
        return [r - z[0]], [[H1], [H2]], False
    if ftype == A.F_BEARING:    # BearingFactor (gtsam/sam/BearingFactor.h)
        th, H1, H2 = bearing_2d(st[0], st[1])
        return [wrap(th - z[0])], [[H1], [H2]], False
    if ftype == A.F_STEREO:     # GenericStereoFactor (gtsam/slam/StereoFactor.h:126-154): cheirality 2 fx
        res = stereo_project(st[0], st[1], z[3:9], want_H)
        if res is None:
            return [2 * z[3]] * 3, [zeros(3, 6), zeros(3, 3)], True
        return sub(res[0], z[:3]), [res[1], res[2]], False
    raise NotImplementedError(f"factor type {ftype}")


def factor_inputs(arr, values, f):
    so = arr.state_offsets()
    ftype, vs, z = R.factor_parts(arr, f)
    return ftype, [int(arr.var_types[v]) for v in vs], [values[so[v]:so[v + 1]] for v in vs], z


def evaluate(arr, values, f):
    """The contract of tests/_factor_restatement.evaluate — (e, [H per key], cheirality), float64 — for all nine factor
    types but GSX_F_LINEAR, evaluated at DPS digits and rounded at the end."""
    e, Hs, cheir = evaluate_mp(*factor_inputs(arr, values, f))
    return to_f64(e), [np.array([[float(x) for x in row] for row in H], dtype=float) for H in Hs], cheir


def true_jacobians(arr, values, f, step="1e-20"):
    """Central differences of the high-precision error in the variables' tangent spaces, taken in high precision: step h,
    truncation O(h^2) = 1e-40, rounding 10^-DPS / h = 1e-30.  One m x d float64 matrix per key."""
    ftype, vt, st, z = factor_inputs(arr, values, f)
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
                moved[k] = retract_mp(vt[k], st[k], dx)
                es.append(evaluate_mp(ftype, vt, moved, z, want_H=False)[0])
            cols.append([(a - b) / (2 * h) for a, b in zip(*es)])
        out.append(np.array([[float(cols[j][i]) for j in range(d)] for i in range(len(cols[0]))], dtype=float))
    return out


# the shared whitening / [A b] / error machinery of tests/_factor_restatement.py on this module's evaluate
linearized = functools.partial(R.linearized, evaluate=evaluate)
jacobians = functools.partial(R.jacobians, evaluate=evaluate)
factor_error = functools.partial(R.factor_error, evaluate=evaluate)
graph_error = functools.partial(R.graph_error, evaluate=evaluate)
dense_system = functools.partial(R.dense_system, evaluate=evaluate)
