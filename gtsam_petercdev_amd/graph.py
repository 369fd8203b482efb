"""Host-side mirror of the reference's interface for the hot path.

Same names, argument meaning and error behaviour as the reference classes so
that the parity tests read like the reference's own tests
(tests/testNonlinearOptimizer.cpp, tests/testGeneralSFMFactorB.cpp, ...):

  NonlinearFactorGraph / Values / Ordering          gtsam/nonlinear, gtsam/inference
  PriorFactor / BetweenFactor / GeneralSFMFactor    gtsam/nonlinear/PriorFactor.h,
                                                    gtsam/slam/BetweenFactor.h,
                                                    gtsam/slam/GeneralSFMFactor.h
  noiseModel.{Unit,Isotropic,Diagonal,Gaussian}     gtsam/linear/NoiseModel.cpp
  LevenbergMarquardtParams / ...Optimizer           gtsam/nonlinear/LevenbergMarquardt*.h
  GaussNewtonOptimizer                              gtsam/nonlinear/GaussNewtonOptimizer.cpp
  GaussianFactorGraph / JacobianFactor              gtsam/linear

These classes only *describe* a problem (they lower it to the flat arrays of
include/gsx.h); every number on the hot path is computed behind the C-ABI.
The backend is pluggable only so that tests can push the identical description
through the CPU oracle; the default is the HIP library and it fails loudly when
that is missing.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Iterable, List, Optional, Sequence

import numpy as np

from . import _abi as A

Key = int


# ---- Symbol (gtsam/inference/Symbol.cpp:29-47) --------------------------------
def symbol(c: str, j: int) -> Key:
    return (ord(c) << 56) | int(j)


def X(j):
    return symbol("x", j)


def L(j):
    return symbol("l", j)


def P(j):
    return symbol("p", j)


def C(j):
    return symbol("c", j)


# ---- geometry value types (host-side construction of Values only) -----------------
class Pose2:
    type_code = A.VAR_POSE2
    dim = 3

    def __init__(self, x=0.0, y=0.0, theta=0.0):
        self.x_, self.y_, self.theta_ = float(x), float(y), float(theta)

    def state(self):
        return np.array([self.x_, self.y_, self.theta_])

    @staticmethod
    def from_state(s):
        return Pose2(s[0], s[1], s[2])

    def x(self):
        return self.x_

    def y(self):
        return self.y_

    def theta(self):
        return self.theta_

    def equals(self, o, tol=1e-9):
        dth = math.atan2(math.sin(self.theta_ - o.theta_), math.cos(self.theta_ - o.theta_))
        return abs(self.x_ - o.x_) < tol and abs(self.y_ - o.y_) < tol and abs(dth) < tol

    def __repr__(self):
        return f"Pose2({self.x_}, {self.y_}, {self.theta_})"


def _skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0.0]])


class Rot3:
    type_code = A.VAR_ROT3
    dim = 3

    def __init__(self, R=None):
        self.R = np.eye(3) if R is None else np.asarray(R, dtype=float).reshape(3, 3)

    def state(self):
        return self.R.reshape(9)

    @staticmethod
    def ClosestTo(M):
        """Rot3::ClosestTo (gtsam/geometry/SO3.cpp:202-208) on the device (gsx_closest_rotations)."""
        from . import _lib
        return Rot3(_lib.closest_rotations(np.asarray(M, dtype=float).reshape(1, 3, 3))[0])

    @staticmethod
    def Rodrigues(wx, wy=None, wz=None):
        """Rot3::Rodrigues -> SO3::Expmap (gtsam/geometry/SO3.cpp:61-96)."""
        w = np.array([wx, wy, wz], dtype=float) if wy is not None else np.asarray(wx, dtype=float)
        th2 = float(w @ w)
        W = _skew(w)
        if th2 <= np.finfo(float).eps:
            a, b = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
        else:
            th = math.sqrt(th2)
            a = math.sin(th) / th
            s2 = math.sin(th / 2.0)
            b = 2.0 * s2 * s2 / th2
        return Rot3(np.eye(3) + a * W + b * (W @ W))

    Expmap = Rodrigues

    @staticmethod
    def Quaternion(w, x, y, z):
        """Rot3::Quaternion(w,x,y,z) (Eigen quaternion -> matrix)."""
        n = math.sqrt(w * w + x * x + y * y + z * z)
        w, x, y, z = w / n, x / n, y / n, z / n
        return Rot3([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])

    @staticmethod
    def RzRyRx(x, y, z):
        """Rot3::RzRyRx(x,y,z) = Rz(z) Ry(y) Rx(x) (gtsam/geometry/Rot3M.cpp)."""
        cx, sx, cy, sy, cz, sz = math.cos(x), math.sin(x), math.cos(y), math.sin(y), math.cos(z), math.sin(z)
        Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        return Rot3(Rz @ Ry @ Rx)

    Ypr = staticmethod(lambda y, p, r: Rot3.RzRyRx(r, p, y))

    def matrix(self):
        return self.R

    @staticmethod
    def from_state(s):
        return Rot3(np.asarray(s[:9]).reshape(3, 3))

    def inverse(self):
        return Rot3(self.R.T)

    def compose(self, o):
        return Rot3(self.R @ o.R)

    def between(self, o):
        return Rot3(self.R.T @ o.R)

    def rotate(self, p):
        return self.R @ _vec3(p)

    def unrotate(self, p):
        return self.R.T @ _vec3(p)

    def equals(self, o, tol=1e-9):
        return np.allclose(self.R, o.R, atol=tol)


def _vec3(p):
    """A Point3, or a Unit3's unit vector."""
    return np.asarray(p.point3() if hasattr(p, "point3") else p, dtype=float).reshape(3)


class Pose3:
    type_code = A.VAR_POSE3
    dim = 6

    def __init__(self, R: Optional[Rot3] = None, t=None):
        self.R_ = R if R is not None else Rot3()
        self.t_ = np.zeros(3) if t is None else np.asarray(t, dtype=float).reshape(3)

    def state(self):
        return np.concatenate([self.R_.R.reshape(9), self.t_])

    @staticmethod
    def from_state(s):
        return Pose3(Rot3(np.asarray(s[:9]).reshape(3, 3)), s[9:12])

    def rotation(self):
        return self.R_

    def translation(self):
        return self.t_

    def compose(self, o):
        return Pose3(Rot3(self.R_.R @ o.R_.R), self.t_ + self.R_.R @ o.t_)

    def inverse(self):
        return Pose3(Rot3(self.R_.R.T), -self.R_.R.T @ self.t_)

    def between(self, o):
        return self.inverse().compose(o)

    def transformFrom(self, point):
        """Pose3::transformFrom (gtsam/geometry/Pose3.cpp:356-369): R p + t."""
        return self.R_.R @ np.asarray(point, dtype=float).reshape(3) + self.t_

    def transformTo(self, point):
        """Pose3::transformTo (gtsam/geometry/Pose3.cpp:380-397): R' (p - t)."""
        return self.R_.R.T @ (np.asarray(point, dtype=float).reshape(3) - self.t_)

    def equals(self, o, tol=1e-9):
        return np.allclose(self.R_.R, o.R_.R, atol=tol) and np.allclose(self.t_, o.t_, atol=tol)


class Cal3Bundler:
    def __init__(self, f=1.0, k1=0.0, k2=0.0, u0=0.0, v0=0.0):
        self.f, self.k1, self.k2, self.u0, self.v0 = map(float, (f, k1, k2, u0, v0))

    def vector(self):
        return np.array([self.f, self.k1, self.k2, self.u0, self.v0])


class PinholeCameraCal3Bundler:
    """SfmCamera = PinholeCamera<Cal3Bundler> (gtsam/geometry/PinholeCamera.h)."""
    type_code = A.VAR_CAMERA
    dim = 9

    def __init__(self, pose: Pose3, K: Cal3Bundler):
        self.pose_, self.K_ = pose, K

    def state(self):
        return np.concatenate([self.pose_.state(), self.K_.vector()])

    @staticmethod
    def from_state(s):
        return PinholeCameraCal3Bundler(Pose3.from_state(s[:12]), Cal3Bundler(*s[12:17]))

    def pose(self):
        return self.pose_

    def calibration(self):
        return self.K_


class _Vector:
    type_code = A.VAR_VECTOR

    def __init__(self, v):
        self.v = np.atleast_1d(np.asarray(v, dtype=float))
        self.dim = int(self.v.size)

    def state(self):
        return self.v


def Point2(x, y):
    return np.array([x, y], dtype=float)


def Point3(x, y, z):
    return np.array([x, y, z], dtype=float)


def _wrap_value(v):
    if isinstance(v, Cal3_S2):  # a calibration as a variable: its 5-vector
        return _Vector(v.vector())
    return v if hasattr(v, "type_code") else _Vector(v)


def _unwrap(type_code, s):
    if type_code == A.VAR_POSE2:
        return Pose2.from_state(s)
    if type_code == A.VAR_POSE3:
        return Pose3.from_state(s)
    if type_code == A.VAR_CAMERA:
        return PinholeCameraCal3Bundler.from_state(s)
    if type_code == A.VAR_ROT3:
        return Rot3.from_state(s)
    if type_code == A.VAR_UNIT3:
        return Unit3.from_state(s)
    if type_code == A.VAR_ESSENTIAL:
        return EssentialMatrix.from_state(s)
    return np.array(s)


# ---- noise models (gtsam/linear/NoiseModel.cpp) -------------------------------------
class _Noise:
    def __init__(self, kind, dim, params=()):
        self.kind, self.dim_ = kind, int(dim)
        self.params = np.asarray(params, dtype=float).reshape(-1)

    def dim(self):
        return self.dim_

    def isUnit(self):
        return self.kind == A.NOISE_UNIT


class noiseModel:
    class Unit:
        @staticmethod
        def Create(dim):
            return _Noise(A.NOISE_UNIT, dim)

    class Isotropic:
        @staticmethod
        def Sigma(dim, sigma, smart=True):
            # NoiseModel.cpp:625-634: sigma == 1 -> Unit
            if smart and abs(sigma - 1.0) < 1e-9:
                return noiseModel.Unit.Create(dim)
            return _Noise(A.NOISE_ISOTROPIC, dim, [sigma])

        @staticmethod
        def Variance(dim, variance, smart=True):
            return noiseModel.Isotropic.Sigma(dim, math.sqrt(variance), smart)

        @staticmethod
        def Precision(dim, precision, smart=True):
            # a zero precision is an infinite sigma, as Variance(dim, 1 / precision) gives there (NoiseModel.h:577-579)
            return noiseModel.Isotropic.Sigma(dim, 1.0 / math.sqrt(precision) if precision != 0 else math.inf, smart)

    class Diagonal:
        @staticmethod
        def Sigmas(sigmas, smart=True):
            s = np.asarray(sigmas, dtype=float).reshape(-1)
            # NoiseModel.cpp:292-309: a (near-)zero sigma makes the model Constrained; all sigmas equal -> Isotropic
            if smart and s.size > 0 and np.any(s < 1e-8):
                return noiseModel.Constrained.MixedSigmas(s)
            if smart and s.size > 0 and np.all(np.abs(s - s[0]) < 1e-9):
                return noiseModel.Isotropic.Sigma(s.size, float(s[0]), True)
            return _Noise(A.NOISE_DIAGONAL, s.size, s)

        @staticmethod
        def Variances(variances, smart=True):
            return noiseModel.Diagonal.Sigmas(np.sqrt(np.asarray(variances, dtype=float)), smart)

        @staticmethod
        def Precisions(precisions, smart=True):
            return noiseModel.Diagonal.Sigmas(1.0 / np.sqrt(np.asarray(precisions, dtype=float)), smart)

    class Constrained:
        """noiseModel::Constrained (gtsam/linear/NoiseModel.h:389-500): rows with sigma == 0 are hard constraints (eliminated
        by constraint pivots instead of Cholesky, NoiseModel.cpp:503-620); mu weighs their violation in the error functions."""

        @staticmethod
        def MixedSigmas(*args):
            if len(args) == 1:
                sigmas = np.asarray(args[0], dtype=float).reshape(-1)
                mu = np.full(sigmas.size, 1000.0)
            else:
                sigmas = np.asarray(args[1], dtype=float).reshape(-1)
                mu = np.broadcast_to(np.asarray(args[0], dtype=float), sigmas.shape).astype(float)
            return _Noise(A.NOISE_CONSTRAINED, sigmas.size, np.concatenate([sigmas, mu]))

        @staticmethod
        def All(dim, mu=1000.0):
            return noiseModel.Constrained.MixedSigmas(mu, np.zeros(int(dim)))

    class Gaussian:
        @staticmethod
        def SqrtInformation(R, smart=True):
            R = np.asarray(R, dtype=float)
            m = R.shape[0]
            if smart and np.count_nonzero(R - np.diag(np.diagonal(R))) == 0:
                return noiseModel.Diagonal.Sigmas(1.0 / np.diagonal(R), True)  # NoiseModel.cpp:84-96
            return _Noise(A.NOISE_GAUSSIAN, m, np.triu(R).reshape(-1))

        @staticmethod
        def Information(M, smart=True):
            M = np.asarray(M, dtype=float)
            if smart and np.count_nonzero(M - np.diag(np.diagonal(M))) == 0:
                return noiseModel.Diagonal.Precisions(np.diagonal(M), True)  # NoiseModel.cpp:98-112
            Lc = np.linalg.cholesky(M)  # LLT(information).matrixU() = L'
            return _Noise(A.NOISE_GAUSSIAN, M.shape[0], Lc.T.reshape(-1))

        @staticmethod
        def Covariance(S, smart=True):
            return noiseModel.Gaussian.Information(np.linalg.inv(np.asarray(S, dtype=float)), smart)

    class mEstimator:
        """gtsam/linear/LossFunctions.h: robust M-estimators (Block reweighting)."""

        class _M:
            def __init__(self, code, k):
                self.code, self.k = code, float(k)

        class Huber:
            @staticmethod
            def Create(k=1.345):
                return noiseModel.mEstimator._M(A.NOISE_ROBUST_HUBER, k)

        class Tukey:
            @staticmethod
            def Create(c=4.6851):
                return noiseModel.mEstimator._M(A.NOISE_ROBUST_TUKEY, c)

        class Cauchy:
            @staticmethod
            def Create(k=0.1):
                return noiseModel.mEstimator._M(A.NOISE_ROBUST_CAUCHY, k)

    class Robust:
        @staticmethod
        def Create(robust, noise):
            """noiseModel::Robust::Create(mEstimator, baseNoise) — gtsam/linear/NoiseModel.cpp:740-743."""
            return _Noise(noise.kind | robust.code, noise.dim(), np.concatenate([noise.params, [robust.k]]))


# ---- factors ---------------------------------------------------------------------------
class _Factor:
    def __init__(self, ftype, keys, rows, meas, noise: Optional[_Noise]):
        self.ftype, self.keys_, self.rows = ftype, [int(k) for k in keys], int(rows)
        self.meas = np.asarray(meas, dtype=float).reshape(-1)
        self.noise = noise if noise is not None else noiseModel.Unit.Create(rows)
        if self.noise.dim() != self.rows:
            raise ValueError("noise model dimension does not match factor dimension")

    def keys(self):
        return list(self.keys_)


def PriorFactor(key, prior, model=None):
    """PriorFactor<T>(key, prior, model) — gtsam/nonlinear/PriorFactor.h."""
    v = _wrap_value(prior)
    f = _Factor(A.F_PRIOR, [key], v.dim, v.state(), model)
    f.value_type = v.type_code
    return f


def BetweenFactor(key1, key2, measured, model=None):
    """BetweenFactor<T>(key1, key2, measured, model) — gtsam/slam/BetweenFactor.h."""
    v = _wrap_value(measured)
    if v.type_code == A.VAR_CAMERA:
        raise ValueError("BetweenFactor<camera> is not on the supported path")
    if v.type_code in (A.VAR_UNIT3, A.VAR_ESSENTIAL):
        raise ValueError("BetweenFactor on a Unit3 or an EssentialMatrix: neither is a group")
    f = _Factor(A.F_BETWEEN, [key1, key2], v.dim, v.state(), model)
    f.value_type = v.type_code
    return f


BetweenFactorPose2 = BetweenFactorPose3 = BetweenFactorRot3 = BetweenFactorPoint2 = BetweenFactorPoint3 = BetweenFactor
PriorFactorPose2 = PriorFactorPose3 = PriorFactorRot3 = PriorFactorUnit3 = PriorFactorEssentialMatrix = PriorFactorPoint2 = PriorFactorPoint3 = PriorFactor


def GeneralSFMFactor(measured, model, cameraKey, landmarkKey):
    """GeneralSFMFactor<SfmCamera,Point3>(measured, model, cameraKey, landmarkKey)."""
    return _Factor(A.F_SFM, [cameraKey, landmarkKey], 2, measured, model)


GeneralSFMFactorCal3Bundler = GeneralSFMFactor


class Cal3_S2:
    """gtsam/geometry/Cal3_S2.h: (fx, fy, s, u0, v0), or (fov degrees, w, h) — Cal3_S2.cpp:28-41.  As a VALUE (the
    calibration variable of GeneralSFMFactor2, a PriorFactor<Cal3_S2>) it is the 5-vector: Cal3_S2 retracts by vector
    addition (Cal3_S2.h: retract / localCoordinates): Values.insert and PriorFactor take it as that vector."""

    def __init__(self, *args):
        if len(args) == 3:
            fov, w, h = args
            a = fov * math.pi / 360.0  # fov/2 in radians
            f = w / (2.0 * math.tan(a))
            self.v = np.array([f, f, 0.0, w / 2.0, h / 2.0])
        elif len(args) == 5:
            self.v = np.asarray(args, dtype=float)
        else:
            self.v = np.array([1.0, 1.0, 0.0, 0.0, 0.0])

    def fx(self):
        return float(self.v[0])

    def vector(self):
        return self.v.copy()


def _sensor_state(body_P_sensor, cls):
    if not isinstance(body_P_sensor, cls):
        raise ValueError(f"body_P_sensor must be a {cls.__name__}")
    return body_P_sensor.state()


def GenericProjectionFactor(measured, model, poseKey, pointKey, K: "Cal3_S2", body_P_sensor: Optional["Pose3"] = None):
    """GenericProjectionFactor<Pose3, Point3, Cal3_S2>(measured, model, poseKey, pointKey, K[, body_P_sensor]) —
    gtsam/slam/ProjectionFactor.h (default cheirality flags).  With body_P_sensor the camera sits at
    pose.compose(body_P_sensor) (:138-166)."""
    meas = [np.asarray(measured, dtype=float).reshape(2), K.vector()]
    if body_P_sensor is not None:
        meas.append(_sensor_state(body_P_sensor, Pose3))
    return _Factor(A.F_PROJECTION, [poseKey, pointKey], 2, np.concatenate(meas), model)


GenericProjectionFactorCal3_S2 = GenericProjectionFactor


def BearingRangeFactor(poseKey, pointKey, bearing, range_, model):
    """BearingRangeFactor<Pose2, Point2>(poseKey, pointKey, Rot2 bearing, double range, model) — gtsam/sam/
    BearingRangeFactor.h; `bearing` is the angle in radians (Rot2::fromAngle)."""
    return _Factor(A.F_BEARINGRANGE, [poseKey, pointKey], 2, [float(bearing), float(range_)], model)


BearingRangeFactor2D = BearingRangeFactor


def BearingFactor(poseKey, pointKey, measured, model):
    """BearingFactor<Pose2, Point2>(poseKey, pointKey, Rot2 measured, model) — gtsam/sam/BearingFactor.h; `measured` is
    the angle in radians (Rot2::fromAngle)."""
    return _Factor(A.F_BEARING, [poseKey, pointKey], 1, [float(measured)], model)


BearingFactor2D = BearingFactor


def RangeFactor(key1, key2, measured, model):
    """RangeFactor<A1, A2>(key1, key2, measured, model) — gtsam/sam/RangeFactor.h.  The variant — (Pose2, Point2),
    (Pose2, Pose2), (Pose3, Point3) or (Pose3, Pose3) — is the one of the two variables in the Values the graph is lowered
    with; any other pair is refused there (NonlinearFactorGraph.to_arrays)."""
    return _Factor(A.F_RANGE, [key1, key2], 1, [float(measured)], model)


RangeFactor2D = RangeFactorPose2 = RangeFactor3D = RangeFactorPose3 = RangeFactor


def RangeFactorWithTransform(key1, key2, measured, model, body_T_sensor):
    """RangeFactorWithTransform<A1, A2>(key1, key2, measured, model, body_T_sensor) — gtsam/sam/RangeFactor.h:104-150: the
    range from key1's pose composed with body_T_sensor (a Pose2 or a Pose3: the type of key1's variable, checked when the
    graph is lowered)."""
    if not isinstance(body_T_sensor, (Pose2, Pose3)):
        raise ValueError("body_T_sensor must be a Pose2 or a Pose3")
    f = _Factor(A.F_RANGE, [key1, key2], 1, np.concatenate([[float(measured)], body_T_sensor.state()]), model)
    f.sensor_type = body_T_sensor.type_code
    return f


RangeFactorWithTransform2D = RangeFactorWithTransformPose2 = RangeFactorWithTransform
RangeFactorWithTransform3D = RangeFactorWithTransformPose3 = RangeFactorWithTransform


def GeneralSFMFactor2(measured, model, poseKey, landmarkKey, calibKey):
    """GeneralSFMFactor2<Cal3_S2>(measured, model, poseKey, landmarkKey, calibKey) — gtsam/slam/GeneralSFMFactor.h:208-278:
    the calibration is the third variable (a Cal3_S2, held as its 5-vector)."""
    return _Factor(A.F_SFM2, [poseKey, landmarkKey, calibKey], 2, np.asarray(measured, dtype=float).reshape(2), model)


GeneralSFMFactor2Cal3_S2 = GeneralSFMFactor2


class Unit3:
    """gtsam/geometry/Unit3.h: a point on the unit sphere.  The constructor normalises (Unit3.h:70-79) and leaves (0, 0, 0)
    alone — it is what TranslationRecovery compares zero-translation edges against (TranslationRecovery.cpp:55).  As a
    VALUE it is the variable GSX_VAR_UNIT3: state the unit vector, tangent 2 in basis()."""

    type_code = A.VAR_UNIT3
    dim = 2

    def __init__(self, *args):
        if len(args) == 0:
            p = np.array([1.0, 0.0, 0.0])
        elif len(args) == 1:
            p = args[0].p.copy() if isinstance(args[0], Unit3) else np.asarray(args[0], dtype=float).reshape(3).copy()
        else:
            p = np.array([float(a) for a in args]).reshape(3)
        n = math.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
        self.p = p / n if n > 0 else p

    def point3(self):
        return self.p.copy()

    unitVector = point3

    def state(self):
        return self.p

    @staticmethod
    def from_state(s):
        u = Unit3()
        u.p = np.array(s[:3], dtype=float)   # as stored: nothing is normalised again
        return u

    def basis(self):
        """Unit3::basis (Unit3.cpp:72-81, 128-138): 3 x 2."""
        n = self.p
        m = np.abs(n)
        axis = np.zeros(3)
        axis[0 if (m[0] <= m[1] and m[0] <= m[2]) else (1 if (m[1] <= m[0] and m[1] <= m[2]) else 2)] = 1.0
        b1 = np.cross(n, axis)
        b1 = b1 / math.sqrt(b1 @ b1)
        return np.stack([b1, np.cross(n, b1)], axis=1)

    def retract(self, v):
        """Unit3::retract (Unit3.cpp:255-282)."""
        xi = self.basis() @ np.asarray(v, dtype=float).reshape(2)
        theta = math.sqrt(xi @ xi)
        st = 1.0 if theta < np.finfo(float).eps else math.sin(theta) / theta
        return Unit3(math.cos(theta) * self.p + st * xi)

    def localCoordinates(self, other: "Unit3"):
        """Unit3::localCoordinates (Unit3.cpp:285-303)."""
        x = float(self.p @ other.p)
        z = 1.0 - x * x
        if z < np.finfo(float).eps:
            if x <= 0:
                return np.array([math.pi, 0.0])
            y = 1.0 - (x - 1.0) / 3.0
        else:
            y = math.acos(x) / math.sqrt(z)
        return self.basis().T @ (y * (other.p - x * self.p))

    def dot(self, q: "Unit3") -> float:
        return float(self.p[0] * q.p[0] + self.p[1] * q.p[1] + self.p[2] * q.p[2])

    def equals(self, q: "Unit3", tol=1e-9) -> bool:
        return bool(np.all(np.abs(self.p - q.p) <= tol))

    def __repr__(self):
        return f"Unit3({self.p[0]:.6g}, {self.p[1]:.6g}, {self.p[2]:.6g})"


def _so3_logmap(R):
    """SO3::Logmap (gtsam/geometry/SO3.cpp:299-375)."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr + 1.0 < 1e-3:
        k = 2 if (R[2, 2] > R[1, 1] and R[2, 2] > R[0, 0]) else (1 if R[1, 1] > R[0, 0] else 0)
        i, j = (k + 1) % 3, (k + 2) % 3
        W = R[j, i] - R[i, j]
        Q1, Q2, Q3 = 2.0 + 2.0 * R[k, k], R[k, i] + R[i, k], R[j, k] + R[k, j]
        norm = math.sqrt(Q1 * Q1 + Q2 * Q2 + Q3 * Q3 + W * W)
        sgn = -1.0 if W < 0 else 1.0
        scale = sgn * 0.5 / math.sqrt(Q1) * (math.pi - (2 * sgn * W) / norm)
        w = np.zeros(3)
        w[k], w[i], w[j] = scale * Q1, scale * Q2, scale * Q3
        return w
    tr_3 = tr - 3.0
    if tr_3 < -1e-6:
        theta = math.acos((tr - 1.0) / 2.0)
        mag = theta / (2.0 * math.sin(theta))
    else:
        mag = 0.5 - tr_3 / 12.0 + tr_3 * tr_3 / 60.0
    return mag * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])


class EssentialMatrix:
    """gtsam/geometry/EssentialMatrix.h: a rotation aRb and a direction aTb; E = [t]x R.  As a VALUE it is the variable
    GSX_VAR_ESSENTIAL: state R row-major (9), then the direction (3); tangent omega (3), then the direction's 2."""

    type_code = A.VAR_ESSENTIAL
    dim = 5

    def __init__(self, aRb: Optional[Rot3] = None, aTb: Optional[Unit3] = None):
        self.R_ = aRb if aRb is not None else Rot3()
        self.t_ = aTb if aTb is not None else Unit3(1.0, 0.0, 0.0)

    @staticmethod
    def FromPose3(aPb: "Pose3"):
        """EssentialMatrix::FromPose3 (EssentialMatrix.cpp:27-45)."""
        return EssentialMatrix(aPb.rotation(), Unit3(aPb.translation()))

    @staticmethod
    def FromRotationAndDirection(aRb, aTb):
        return EssentialMatrix(aRb, aTb)

    @staticmethod
    def Homogeneous(p):
        p = np.asarray(p, dtype=float).reshape(2)
        return np.array([p[0], p[1], 1.0])

    @staticmethod
    def from_state(s):
        return EssentialMatrix(Rot3.from_state(s[:9]), Unit3.from_state(s[9:12]))

    def state(self):
        return np.concatenate([self.R_.R.reshape(9), self.t_.p])

    def rotation(self):
        return self.R_

    def direction(self):
        return self.t_

    def matrix(self):
        return _skew(self.t_.p) @ self.R_.R

    def retract(self, xi):
        """EssentialMatrix.h:92-94: (R Expmap(xi[:3]), t.retract(xi[3:]))."""
        xi = np.asarray(xi, dtype=float).reshape(5)
        return EssentialMatrix(self.R_.compose(Rot3.Expmap(xi[:3])), self.t_.retract(xi[3:]))

    def localCoordinates(self, other: "EssentialMatrix"):
        """EssentialMatrix.h:97-103."""
        return np.concatenate([_so3_logmap(self.R_.R.T @ other.R_.R), self.t_.localCoordinates(other.t_)])

    def rotate(self, cRb: Rot3):
        """EssentialMatrix::rotate (EssentialMatrix.cpp:73-101): E in the camera frame."""
        return EssentialMatrix(Rot3(cRb.R @ self.R_.R @ cRb.R.T), Unit3(cRb.R @ self.t_.p))

    def error(self, vA, vB):
        """EssentialMatrix::error (EssentialMatrix.cpp:104-114): vA' E vB."""
        return float(np.asarray(vA, dtype=float) @ self.matrix() @ np.asarray(vB, dtype=float))

    def equals(self, o, tol=1e-8):
        return self.R_.equals(o.R_, tol) and self.t_.equals(o.t_, tol)

    def __repr__(self):
        return f"EssentialMatrix(R={self.R_.R.tolist()}, t={self.t_})"


def _direction(w_aZb) -> np.ndarray:
    return w_aZb.point3() if isinstance(w_aZb, Unit3) else Unit3(w_aZb).point3()


def TranslationFactor(a, b, w_aZb, model=None):
    """TranslationFactor(a, b, w_aZb, noiseModel) — gtsam/sfm/TranslationFactor.h:41-78: normalize(Tb - Ta) - w_aZb."""
    return _Factor(A.F_TRANSLATION, [a, b], 3, _direction(w_aZb), model)


def BilinearAngleTranslationFactor(a, b, scaleKey, w_aZb, model=None):
    """BilinearAngleTranslationFactor(a, b, scale_key, w_aZb, noiseModel) — TranslationFactor.h:104-149 (BATA):
    |s| (Tb - Ta) - w_aZb with the scale a Vector1 variable."""
    return _Factor(A.F_BILINEAR_TRANSLATION, [a, b, scaleKey], 3, _direction(w_aZb), model)


# ---- absolute-measurement factors (gtsam/navigation, gtsam/slam/Pose*Prior.h): the reference's argument orders ----------
def GPSFactor(key, gpsIn, model):
    """GPSFactor(key, gpsIn, model) — gtsam/navigation/GPSFactor.h: e = translation - gpsIn."""
    return _Factor(A.F_GPS, [key], 3, _vec3(gpsIn), model)


def GPSFactorArm(key, gpsIn, leverArm, model):
    """GPSFactorArm(key, gpsIn, leverArm, model): e = translation + R leverArm - gpsIn."""
    return _Factor(A.F_GPS, [key], 3, np.concatenate([_vec3(gpsIn), _vec3(leverArm)]), model)


def GPSFactorArmCalib(key1, key2, gpsIn, model):
    """GPSFactorArmCalib(poseKey, leverArmKey, gpsIn, model): the lever arm is the Point3 variable key2."""
    return _Factor(A.F_GPS, [key1, key2], 3, _vec3(gpsIn), model)


def PoseTranslationPrior2D(key, measured, model):
    """PoseTranslationPrior<Pose2>(key, translation | pose, model) — gtsam/slam/PoseTranslationPrior.h."""
    t = np.array([measured.x(), measured.y()]) if isinstance(measured, Pose2) else np.asarray(measured, dtype=float).reshape(2)
    return _Factor(A.F_POSE_TRANSLATION_PRIOR, [key], 2, t, model)


def PoseTranslationPrior3D(key, measured, model):
    """PoseTranslationPrior<Pose3>(key, translation | pose, model)."""
    t = measured.translation() if isinstance(measured, Pose3) else _vec3(measured)
    return _Factor(A.F_POSE_TRANSLATION_PRIOR, [key], 3, t, model)


def PoseRotationPrior2D(key, measured, model):
    """PoseRotationPrior<Pose2>(key, rotation angle | pose, model) — gtsam/slam/PoseRotationPrior.h."""
    th = measured.theta() if isinstance(measured, Pose2) else float(measured)
    return _Factor(A.F_POSE_ROTATION_PRIOR, [key], 1, [th], model)


def PoseRotationPrior3D(key, measured, model):
    """PoseRotationPrior<Pose3>(key, Rot3 | pose, model)."""
    R = measured.rotation() if isinstance(measured, Pose3) else measured
    return _Factor(A.F_POSE_ROTATION_PRIOR, [key], 3, R.state(), model)


def _unit3_vector(u):
    return (u if isinstance(u, Unit3) else Unit3(u)).point3()


def Rot3AttitudeFactor(key, nRef, model, bMeasured=None):
    """Rot3AttitudeFactor(key, nRef, model, bMeasured = Unit3(0, 0, 1)) — gtsam/navigation/AttitudeFactor.h:96-100."""
    b = _unit3_vector(bMeasured if bMeasured is not None else Unit3(0.0, 0.0, 1.0))
    f = _Factor(A.F_ATTITUDE, [key], 2, np.concatenate([_unit3_vector(nRef), b]), model)
    f.value_type = A.VAR_ROT3
    return f


def Pose3AttitudeFactor(key, nRef, model, bMeasured=None):
    """Pose3AttitudeFactor(key, nRef, model, bMeasured = Unit3(0, 0, 1)) — AttitudeFactor.h:178-182."""
    f = Rot3AttitudeFactor(key, nRef, model, bMeasured)
    f.value_type = A.VAR_POSE3
    return f


def MagFactor1(key, measured, scale, direction, bias, model):
    """MagFactor1(key, measured, scale, direction, bias, model) — gtsam/navigation/MagFactor.h:105-110: nM = scale * direction
    (a Unit3)."""
    return _Factor(A.F_MAG, [key], 3, np.concatenate([_vec3(measured), float(scale) * _unit3_vector(direction), _vec3(bias)]),
                   model)


def _mag_pose(key, measured, scale, direction, bias, model, body_P_sensor, n):
    # MagPoseFactor's constructor (gtsam/navigation/MagPoseFactor.h:74-85): z and bias rotated into the body frame,
    # nM = scale * direction.normalized()
    z, d, b = (np.asarray(v, dtype=float).reshape(n) for v in (measured, direction, bias))
    if body_P_sensor is not None:
        if n == 3:
            R = body_P_sensor.rotation().matrix()
        else:
            c, s = math.cos(body_P_sensor.theta()), math.sin(body_P_sensor.theta())
            R = np.array([[c, -s], [s, c]])
        z, b = R @ z, R @ b
    return _Factor(A.F_MAG, [key], n, np.concatenate([z, float(scale) * (d / np.linalg.norm(d)), b]), model)


def MagPoseFactorPose2(pose_key, measured, scale, direction, bias, model, body_P_sensor=None):
    """MagPoseFactor<Pose2>(pose_key, measured, scale, direction, bias, model, body_P_sensor)."""
    return _mag_pose(pose_key, measured, scale, direction, bias, model, body_P_sensor, 2)


def MagPoseFactorPose3(pose_key, measured, scale, direction, bias, model, body_P_sensor=None):
    """MagPoseFactor<Pose3>(pose_key, measured, scale, direction, bias, model, body_P_sensor)."""
    return _mag_pose(pose_key, measured, scale, direction, bias, model, body_P_sensor, 3)


# ---- two-view geometry (gtsam/slam/EssentialMatrixFactor.h, EssentialMatrixConstraint.h): the reference's argument orders -
def _calibrate_s2(K: "Cal3_S2", p):
    """Cal3_S2::calibrate (gtsam/geometry/Cal3_S2.cpp:53-69)."""
    fx, fy, s, u0, v0 = K.vector()
    p = np.asarray(p, dtype=float).reshape(2)
    y = (p[1] - v0) / fy
    return np.array([((p[0] - u0) - s * y) / fx, y])


def EssentialMatrixFactor(key, pA, pB, model, K: Optional["Cal3_S2"] = None):
    """EssentialMatrixFactor(key, pA, pB, model[, K]) — :52-78: the points in calibrated coordinates, or in pixels with K
    (used in the constructor only).  e = vA' E vB."""
    if K is not None:
        pA, pB = _calibrate_s2(K, pA), _calibrate_s2(K, pB)
    return _Factor(A.F_ESSENTIAL, [key], 1, np.concatenate([EssentialMatrix.Homogeneous(pA), EssentialMatrix.Homogeneous(pB)]),
                   model)


def EssentialMatrixFactor2(key1, key2, pA, pB, model, K: Optional["Cal3_S2"] = None):
    """EssentialMatrixFactor2(key1, key2, pA, pB, model[, K]) — :133-158: key2 is the inverse depth (a double, held as a
    1-vector); f = 1, or (fx + fy) / 2 with K."""
    f = 1.0
    if K is not None:
        pA, pB = _calibrate_s2(K, pA), _calibrate_s2(K, pB)
        f = 0.5 * (K.vector()[0] + K.vector()[1])
    return _Factor(A.F_ESSENTIAL_DEPTH, [key1, key2], 2,
                   np.concatenate([EssentialMatrix.Homogeneous(pA), np.asarray(pB, dtype=float).reshape(2), [f]]), model)


def EssentialMatrixFactor3(key1, key2, pA, pB, cRb: Rot3, model, K: Optional["Cal3_S2"] = None):
    """EssentialMatrixFactor3(key1, key2, pA, pB, cRb, model[, K]) — :256-273: E is rotated into the camera frame first."""
    f = EssentialMatrixFactor2(key1, key2, pA, pB, model, K)
    f.meas = np.concatenate([f.meas, cRb.state()])
    return f


def EssentialMatrixFactor4(keyE, keyK, pA, pB, model=None):
    """EssentialMatrixFactor4<Cal3_S2>(keyE, keyK, pA, pB, model) — :358-360: the points in pixels, the calibration the
    variable keyK (a Cal3_S2, held as its 5-vector)."""
    return _Factor(A.F_ESSENTIAL_CALIB, [keyE, keyK], 1,
                   np.concatenate([np.asarray(pA, dtype=float).reshape(2), np.asarray(pB, dtype=float).reshape(2)]), model)


EssentialMatrixFactor4Cal3_S2 = EssentialMatrixFactor4


def EssentialMatrixConstraint(key1, key2, measuredE: "EssentialMatrix", model):
    """EssentialMatrixConstraint(key1, key2, measuredE, model) — gtsam/slam/EssentialMatrixConstraint.h: between two Pose3."""
    return _Factor(A.F_ESSENTIAL_CONSTRAINT, [key1, key2], 5, measuredE.state(), model)


class Cal3_S2Stereo:
    """gtsam/geometry/Cal3_S2Stereo.h: (fx, fy, s, u0, v0, b)."""

    def __init__(self, fx=1.0, fy=1.0, s=0.0, u0=0.0, v0=0.0, b=1.0):
        self.v = np.array([fx, fy, s, u0, v0, b], dtype=float)

    def fx(self):
        return float(self.v[0])

    def baseline(self):
        return float(self.v[5])

    def vector(self):
        return self.v.copy()


class StereoPoint2:
    """gtsam/geometry/StereoPoint2.h: (uL, uR, v)."""

    def __init__(self, uL=0.0, uR=0.0, v=0.0):
        self.v_ = np.array([uL, uR, v], dtype=float)

    def uL(self):
        return float(self.v_[0])

    def uR(self):
        return float(self.v_[1])

    def v(self):
        return float(self.v_[2])

    def vector(self):
        return self.v_.copy()


def GenericStereoFactor(measured, model, poseKey, landmarkKey, K: "Cal3_S2Stereo", body_P_sensor: Optional["Pose3"] = None):
    """GenericStereoFactor<Pose3, Point3>(measured, model, poseKey, landmarkKey, K[, body_P_sensor]) —
    gtsam/slam/StereoFactor.h (default cheirality flags).  With body_P_sensor the stereo camera sits at
    pose.compose(body_P_sensor) (:126-154)."""
    z = measured.vector() if isinstance(measured, StereoPoint2) else np.asarray(measured, dtype=float).reshape(3)
    meas = [z, K.vector()]
    if body_P_sensor is not None:
        meas.append(_sensor_state(body_P_sensor, Pose3))
    return _Factor(A.F_STEREO, [poseKey, landmarkKey], 3, np.concatenate(meas), model)


GenericStereoFactor3D = GenericStereoFactor


def JacobianFactor(*args):
    """JacobianFactor(key1, A1, [key2, A2, ...], b[, model]) — gtsam/linear/JacobianFactor.h.
    A diagonal/isotropic model is folded in by the backend (whitening)."""
    args = list(args)
    model = args.pop() if isinstance(args[-1], _Noise) else None
    b = np.asarray(args.pop(), dtype=float).reshape(-1)
    keys, blocks = [], []
    for i in range(0, len(args), 2):
        keys.append(int(args[i]))
        blocks.append(np.asarray(args[i + 1], dtype=float).reshape(b.size, -1))
    Ab = np.concatenate(blocks + [b.reshape(-1, 1)], axis=1)
    f = _Factor(A.F_LINEAR, keys, b.size, Ab.reshape(-1, order="F"), model)
    f.block_dims = [blk.shape[1] for blk in blocks]
    return f


# ---- containers ----------------------------------------------------------------------------
class Values:
    def __init__(self, other: Optional["Values"] = None):
        self._v: Dict[Key, object] = dict(other._v) if other is not None else {}

    def insert(self, key, value):
        if int(key) in self._v:
            raise KeyError(f"ValuesKeyAlreadyExists: {key}")
        self._v[int(key)] = _wrap_value(value)

    def update(self, key, value):
        self._v[int(key)] = _wrap_value(value)

    def exists(self, key):
        return int(key) in self._v

    def keys(self):
        return sorted(self._v)

    def size(self):
        return len(self._v)

    def at(self, key):
        if int(key) not in self._v:
            raise KeyError(f"ValuesKeyDoesNotExist: {key}")
        v = self._v[int(key)]
        return v.v.copy() if isinstance(v, _Vector) else v

    atPose2 = atPose3 = atRot3 = atUnit3 = atEssentialMatrix = atPoint2 = atPoint3 = atVector = at

    def dims(self):
        return {k: self._v[k].dim for k in self.keys()}

    def pack(self):
        ks = self.keys()
        return (np.concatenate([self._v[k].state() for k in ks]) if ks else np.zeros(0))

    @staticmethod
    def unpack(keys, types, dims, packed):
        out, off = Values(), 0
        for k, t, d in zip(keys, types, dims):
            sd = A.STATE_DIM.get(int(t), int(d))
            out._v[int(k)] = _wrap_value(_unwrap(int(t), packed[off:off + sd]))
            off += sd
        return out


class Ordering(list):
    """gtsam/inference/Ordering.h — a list of keys in elimination order."""

    def push_back(self, k):
        self.append(int(k))


class NonlinearFactorGraph:
    def __init__(self):
        self.factors: List[Optional[_Factor]] = []

    def add(self, f):
        self.factors.append(f)

    push_back = emplace_shared = add

    def addPrior(self, key, prior, model=None):
        self.add(PriorFactor(key, prior, model))

    def size(self):
        return len(self.factors)

    def keys(self):
        return sorted({k for f in self.factors if f is not None for k in f.keys_})

    # -- lowering to include/gsx.h arrays -----------------------------------------
    def to_arrays(self, values: Optional[Values] = None, var_dims: Optional[Dict[Key, int]] = None) -> A.ProblemArrays:
        facs = [f for f in self.factors if f is not None]  # null factors are skipped (NonlinearFactorGraph.cpp:239-278)
        if values is not None:
            keys = values.keys()
            types = [values._v[k].type_code for k in keys]
            dims = [values._v[k].dim for k in keys]
        else:  # linear graph: dims from the Jacobian blocks
            dd: Dict[Key, int] = dict(var_dims or {})
            for f in facs:
                for k, d in zip(f.keys_, getattr(f, "block_dims", [])):
                    dd[k] = d
            keys = sorted(dd)
            types = [A.VAR_VECTOR] * len(keys)
            dims = [dd[k] for k in keys]
        index = {k: i for i, k in enumerate(keys)}
        key_ptr, meas_ptr, noise_ptr = [0], [0], [0]
        fvars: List[int] = []
        meas: List[np.ndarray] = []
        noise: List[np.ndarray] = []
        for f in facs:
            for k in f.keys_:
                if k not in index:
                    raise KeyError(f"ValuesKeyDoesNotExist: {k}")
                fvars.append(index[k])
            if f.ftype == A.F_RANGE and values is not None:  # the variant is the one of the two variables' types
                (t1, d1), (t2, d2) = [(types[index[k]], dims[index[k]]) for k in f.keys_]
                if t1 not in (A.VAR_POSE2, A.VAR_POSE3) or not (
                        t2 == t1 or (t2 == A.VAR_VECTOR and d2 == (2 if t1 == A.VAR_POSE2 else 3))):
                    raise ValueError(f"RangeFactor between variables {f.keys_}: not (Pose2 | Pose3) to a point of its space "
                                     "or to a pose of its kind")
                if getattr(f, "sensor_type", t1) != t1:
                    raise ValueError(f"RangeFactorWithTransform on variables {f.keys_}: body_T_sensor is not of the first "
                                     "variable's type")
            key_ptr.append(len(fvars))
            meas.append(f.meas)
            meas_ptr.append(meas_ptr[-1] + f.meas.size)
            noise.append(f.noise.params)
            noise_ptr.append(noise_ptr[-1] + f.noise.params.size)
        cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0)
        return A.ProblemArrays(
            var_keys=np.array(keys, dtype=np.uint64), var_types=types, var_dims=dims,
            f_type=[f.ftype for f in facs], f_rows=[f.rows for f in facs],
            f_key_ptr=key_ptr, f_vars=fvars, f_meas_ptr=meas_ptr, meas=cat(meas),
            f_noise_kind=[f.noise.kind for f in facs], f_noise_ptr=noise_ptr, noise=cat(noise),
            values=values.pack() if values is not None else None)

    def error(self, values: Values, backend_factory=None) -> float:
        be = _make_backend(self.to_arrays(values), backend_factory)
        try:
            return be.error()
        finally:
            be.close()


class GaussianFactorGraph(NonlinearFactorGraph):
    """Linear graph of JacobianFactors; optimize() = the NonlinearOptimizer::solve seam."""

    def optimize(self, ordering: Optional[Sequence[Key]] = None, backend_factory=None) -> Dict[Key, np.ndarray]:
        arrays = self.to_arrays(None)
        arrays.values = np.zeros(int(arrays.var_dims.sum()))
        be = _make_backend(arrays, backend_factory)
        try:
            be.set_ordering(ordering if ordering is not None else be.compute_ordering(A.ORDER_MINDEGREE))
            be.linearize()
            delta = be.solve(0.0)
        finally:
            be.close()
        off = arrays.tangent_offsets()
        return {int(k): delta[off[i]:off[i + 1]] for i, k in enumerate(arrays.var_keys)}


class InitializePose3:
    """InitializePose3 (gtsam/slam/InitializePose3.h) on the device: chordal relaxation or Riemannian gradient for the
    rotations, then one Gauss-Newton iteration for the poses (include/gsx.h: gsx_initialize_pose3 and its stages)."""

    kAnchorKey = A.ANCHOR_KEY

    @staticmethod
    def buildPose3graph(graph) -> "NonlinearFactorGraph":
        """initialize::buildPoseGraph<Pose3> (InitializePose.h:36-52): the BetweenFactor<Pose3> of the graph, and every
        PriorFactor<Pose3> as a between factor from the anchor key with the prior's noise."""
        out = NonlinearFactorGraph()
        for f in graph.factors:
            if f is None or getattr(f, "value_type", None) != A.VAR_POSE3:
                continue
            if f.ftype == A.F_BETWEEN:
                out.add(f)
            elif f.ftype == A.F_PRIOR:
                out.add(BetweenFactor(A.ANCHOR_KEY, f.keys_[0], Pose3.from_state(f.meas), f.noise))
        return out

    @staticmethod
    def _lower(pose3Graph, given: Optional["Values"] = None):
        """The arrays of include/gsx.h for a graph of buildPose3graph: its keys as POSE3 variables, a between factor from
        the anchor as the prior it came from; and `given` packed in that order (None without one)."""
        keys = sorted({k for f in pose3Graph.factors for k in f.keys_} - {A.ANCHOR_KEY})
        values = Values()
        for k in keys:
            values.insert(k, given.at(k) if given is not None else Pose3())
        g = NonlinearFactorGraph()
        for f in pose3Graph.factors:
            if f.ftype != A.F_BETWEEN or getattr(f, "value_type", None) != A.VAR_POSE3:
                raise ValueError("InitializePose3: not a graph of buildPose3graph")
            if f.keys_[0] == A.ANCHOR_KEY:
                g.add(PriorFactor(f.keys_[1], Pose3.from_state(f.meas), f.noise))
            else:
                g.add(f)
        arr = g.to_arrays(values)
        return arr, keys, (arr.values if given is not None else None)

    @staticmethod
    def _rotations(keys, rot) -> "Values":
        out = Values()
        for k, R in zip(keys, rot):
            out.insert(k, Rot3(R))
        return out

    @staticmethod
    def computeOrientationsChordal(pose3Graph) -> "Values":
        from . import _lib
        arr, keys, _ = InitializePose3._lower(pose3Graph)
        return InitializePose3._rotations(keys, _lib.pose3_orientations_chordal(arr))

    @staticmethod
    def computeOrientationsGradient(pose3Graph, givenGuess, maxIter=10000, setRefFrame=True) -> "Values":
        from . import _lib
        arr, keys, given = InitializePose3._lower(pose3Graph, givenGuess)
        return InitializePose3._rotations(keys, _lib.pose3_orientations_gradient(arr, given, maxIter, setRefFrame)[0])

    @staticmethod
    def initializeOrientations(graph) -> "Values":
        return InitializePose3.computeOrientationsChordal(InitializePose3.buildPose3graph(graph))

    @staticmethod
    def createSymbolicGraph(pose3Graph):
        """(adjEdgesMap: key -> factor indices in graph order, factorId2RotMap: factor index -> measured Rot3)."""
        from . import _lib
        arr, keys, _ = InitializePose3._lower(pose3Graph)
        _, _, adj = _lib.pose3_init_structure(arr)
        names = keys + [A.ANCHOR_KEY]
        adjEdgesMap = {names[i]: lst for i, lst in enumerate(adj) if lst}
        factorId2RotMap = {i: Pose3.from_state(f.meas).rotation() for i, f in enumerate(pose3Graph.factors)}
        return adjEdgesMap, factorId2RotMap

    @staticmethod
    def computePoses(initialRot, posegraph, singleIter=True) -> "Values":
        """initialize::computePoses<Pose3> (InitializePose.h:57-97).  (The reference also appends the anchor's prior to the
        caller's posegraph; this one leaves it as it is.)"""
        from . import _lib
        arr, keys, _ = InitializePose3._lower(posegraph)
        rot = np.stack([np.asarray(initialRot.at(k).matrix(), dtype=float) for k in keys]) if keys else np.zeros((0, 3, 3))
        packed = _lib.pose3_compute_poses(arr, rot, singleIter)
        return Values.unpack(arr.var_keys, arr.var_types, arr.var_dims, packed)

    @staticmethod
    def initialize(graph, givenGuess=None, useGradient=False) -> "Values":
        """InitializePose3::initialize (InitializePose3.cpp:296-319)."""
        from . import _lib
        arr, keys, given = InitializePose3._lower(InitializePose3.buildPose3graph(graph),
                                                  givenGuess if (givenGuess is not None and givenGuess.size() > 0) else None)
        p = _lib.init_pose3_params_default()
        p.use_gradient = int(bool(useGradient))
        packed, _ = _lib.initialize_pose3(arr, given, p)
        return Values.unpack(arr.var_keys, arr.var_types, arr.var_dims, packed)


class lago:
    """namespace lago (gtsam/slam/lago.h) on the device: a spanning tree on the host, then the cumulative orientations, the
    regularized orientation system, the pose system and the composition on the device (include/gsx.h: gsx_lago_*)."""

    kAnchorKey = A.ANCHOR_KEY

    @staticmethod
    def buildPose2graph(graph) -> "NonlinearFactorGraph":
        """initialize::buildPoseGraph<Pose2> (InitializePose.h:36-52): the BetweenFactor<Pose2> of the graph, and every
        PriorFactor<Pose2> as a between factor from the anchor key with the prior's noise."""
        out = NonlinearFactorGraph()
        for f in graph.factors:
            if f is None or getattr(f, "value_type", None) != A.VAR_POSE2:
                continue
            if f.ftype == A.F_BETWEEN:
                out.add(f)
            elif f.ftype == A.F_PRIOR:
                out.add(BetweenFactor(A.ANCHOR_KEY, f.keys_[0], Pose2.from_state(f.meas), f.noise))
        return out

    @staticmethod
    def _lower(pose2Graph, given: Optional["Values"] = None):
        """The arrays of include/gsx.h for a graph of buildPose2graph: its keys as POSE2 variables, a between factor from
        the anchor as the prior it came from; and `given` packed in that order (None without one)."""
        keys = sorted({k for f in pose2Graph.factors for k in f.keys_} - {A.ANCHOR_KEY})
        values = Values()
        for k in keys:
            values.insert(k, given.at(k) if given is not None else Pose2())
        g = NonlinearFactorGraph()
        for f in pose2Graph.factors:
            if f.ftype != A.F_BETWEEN or getattr(f, "value_type", None) != A.VAR_POSE2:
                raise ValueError("lago: not a graph of buildPoseGraph<Pose2>")
            if f.keys_[0] == A.ANCHOR_KEY:
                g.add(PriorFactor(f.keys_[1], Pose2.from_state(f.meas), f.noise))
            else:
                g.add(f)
        arr = g.to_arrays(values)
        return arr, keys, (arr.values if given is not None else None)

    @staticmethod
    def findMinimumSpanningTree(pose2Graph) -> Dict[Key, Key]:
        """lago::findMinimumSpanningTree (lago.cpp:229-260): the PredecessorMap {key: parent key}, the anchor its own."""
        from . import _lib
        arr, keys, _ = lago._lower(pose2Graph)
        names = keys + [A.ANCHOR_KEY]
        parent = _lib.lago_structure(arr, False)["parent"]
        return {names[i]: names[p] for i, p in enumerate(parent) if p >= 0}

    @staticmethod
    def getSymbolicGraph(tree, g):
        """lago::getSymbolicGraph (lago.cpp:101-138) for any PredecessorMap: (spanningTreeIds, chordsIds, deltaThetaMap).
        Ids count every factor of g; a missing key raises KeyError as tree.at does."""
        spanningTreeIds, chordsIds, deltaThetaMap = [], [], {}
        i = 0
        for f in g.factors:
            if f is not None and len(f.keys_) == 2:
                if f.ftype != A.F_BETWEEN or getattr(f, "value_type", None) != A.VAR_POSE2:
                    continue   # (the reference's `continue` skips its id++ as well)
                key1, key2 = f.keys_
                deltaTheta = float(f.meas[2])
                if deltaTheta > math.pi or deltaTheta <= -math.pi:   # measured().theta()
                    deltaTheta = math.atan2(math.sin(deltaTheta), math.cos(deltaTheta))
                if tree[key1] == key2:
                    deltaThetaMap.setdefault(key1, -deltaTheta)
                    spanningTreeIds.append(i)
                elif tree[key2] == key1:
                    deltaThetaMap.setdefault(key2, deltaTheta)
                    spanningTreeIds.append(i)
                else:
                    chordsIds.append(i)
            i += 1
        return spanningTreeIds, chordsIds, deltaThetaMap

    @staticmethod
    def computeThetasToRoot(deltaThetaMap, tree) -> Dict[Key, float]:
        """lago::computeThetasToRoot (lago.cpp:82-98) on the device (gsx_lago_thetas_to_root)."""
        from . import _lib
        keys = sorted(tree)
        index = {k: i for i, k in enumerate(keys)}
        parent = np.array([index[tree[k]] for k in keys], dtype=np.int32)
        delta = np.array([0.0 if tree[k] == k else deltaThetaMap[k] for k in keys])
        theta = _lib.lago_thetas_to_root(parent, delta)
        return {k: float(theta[index[k]]) for k in keys if k in deltaThetaMap or tree[k] == k}

    @staticmethod
    def initializeOrientations(graph, useOdometricPath=True) -> Dict[Key, np.ndarray]:
        """lago::initializeOrientations (lago.cpp:297-305): {key: [theta]}, not wrapped, the anchor's (0) included as in
        the reference's VectorValues."""
        from . import _lib
        arr, keys, _ = lago._lower(lago.buildPose2graph(graph))
        theta = _lib.lago_initialize_orientations(arr, bool(useOdometricPath))
        out = {k: np.array([t]) for k, t in zip(keys, theta)}
        out[A.ANCHOR_KEY] = np.array([0.0])
        return out

    @staticmethod
    def initialize(graph, useOdometricPathOrInitialGuess=True) -> "Values":
        """lago::initialize(graph, useOdometricPath = true) (lago.cpp:375-388) and lago::initialize(graph, initialGuess)
        (:391-409): with a Values the poses keep its x and y and take lago's orientation (odometric tree)."""
        from . import _lib
        pg = lago.buildPose2graph(graph)
        if isinstance(useOdometricPathOrInitialGuess, Values):
            arr, _, given = lago._lower(pg, useOdometricPathOrInitialGuess)
            packed = _lib.lago_initialize_with_guess(arr, given)
        else:
            arr, _, _ = lago._lower(pg)
            packed = _lib.lago_initialize(arr, bool(useOdometricPathOrInitialGuess))
        return Values.unpack(arr.var_keys, arr.var_types, arr.var_dims, packed)


# ---- translation averaging: 1dSfM (gtsam/sfm/MFAS.h, TranslationRecovery.h) on the device: include/gsx.h gsx_mfas_*, gsx_translation_* ----
class _BinaryMeasurement:
    """gtsam/sfm/BinaryMeasurement.h."""

    def __init__(self, key1, key2, measured, model=None):
        self.key1_, self.key2_, self.measured_ = int(key1), int(key2), measured
        self.model_ = model if model is not None else noiseModel.Unit.Create(3)

    def key1(self): return self.key1_
    def key2(self): return self.key2_
    def measured(self): return self.measured_
    def noiseModel(self): return self.model_


class BinaryMeasurementUnit3(_BinaryMeasurement):
    def __init__(self, key1, key2, measured, model=None):
        super().__init__(key1, key2, measured if isinstance(measured, Unit3) else Unit3(measured), model)

    def vector(self):
        return self.measured_.point3()


class BinaryMeasurementPoint3(_BinaryMeasurement):
    def __init__(self, key1, key2, measured, model=None):
        super().__init__(key1, key2, np.asarray(measured, dtype=float).reshape(3).copy(), model)

    def vector(self):
        return self.measured_.copy()


class MFAS:
    """gtsam/sfm/MFAS.h: MFAS(relativeTranslations, projectionDirection) or MFAS(edgeWeights); the D = 1 case of the batched
    device entry (gsx_mfas_outlier_weights).  The ordering is *a* valid MFAS ordering: among several roots the lowest key
    comes first, where the reference takes the first in unordered_map order (include/gsx.h)."""

    def __init__(self, *args):
        if len(args) == 2:
            relativeTranslations, direction = args
            d = direction if isinstance(direction, Unit3) else Unit3(direction)
            self.edgeWeights_ = {}
            for m in relativeTranslations:   # (a repeated pair keeps the last entry: the map assignment of MFAS.cpp:119)
                self.edgeWeights_[(m.key1(), m.key2())] = m.measured().dot(d)
        else:
            self.edgeWeights_ = {(int(a), int(b)): float(w) for (a, b), w in dict(args[0]).items()}

    def _run(self, want_ordering):
        from . import _lib
        pairs = list(self.edgeWeights_)
        w = np.array([[self.edgeWeights_[p] for p in pairs]])
        return pairs, _lib.mfas_outlier_weights([p[0] for p in pairs], [p[1] for p in pairs], weights=w,
                                                want_ordering=want_ordering)

    def computeOrdering(self) -> List[Key]:
        if not self.edgeWeights_:
            return []
        return [int(k) for k in self._run(True)[1]["ordering"][0]]

    def computeOutlierWeights(self) -> Dict[Tuple[Key, Key], float]:
        if not self.edgeWeights_:
            return {}
        pairs, out = self._run(False)
        return {p: float(x) for p, x in zip(pairs, out["weights"][0])}

    @staticmethod
    def outlierWeightsBatch(measurements, directions) -> dict:
        """The batched entry: every measurement projected along every direction (D workgroups in one launch).  Returns
        {"pairs": [(key1, key2)], "weights": (D, E), "mean": (E,)} in the order of `measurements`; mean[e] = sum over d of
        weights[d][e] / D, the average of python/gtsam/examples/TranslationAveragingExample.py:84-87."""
        from . import _lib
        ms = list(measurements)
        dirs = np.array([(d if isinstance(d, Unit3) else Unit3(d)).point3() for d in directions]).reshape(-1, 3)
        out = _lib.mfas_outlier_weights([m.key1() for m in ms], [m.key2() for m in ms],
                                        edge_dirs=np.array([m.measured().point3() for m in ms]).reshape(-1, 3), proj_dirs=dirs)
        return dict(pairs=[(m.key1(), m.key2()) for m in ms], weights=out["weights"], mean=out["mean"])


class TranslationRecovery:
    """gtsam/sfm/TranslationRecovery.h: TranslationRecovery(lmParams) / TranslationRecovery(lmParams,
    use_bilinear_translation_factor).  run() goes through gsx_translation_recovery; buildGraph / addPrior /
    initializeRandomly are the reference's building blocks on this mirror's graph classes (initializeRandomly draws from
    gsx_translation_recovery_problem, so the stream is the library's: std::mt19937(seed), fresh per call)."""

    def __init__(self, lmParams=None, use_bilinear_translation_factor=False, seed=42):
        self.lmParams_ = lmParams if lmParams is not None else LevenbergMarquardtParams()
        self.use_bilinear_translation_factor_ = bool(use_bilinear_translation_factor)
        self.seed_ = int(seed)

    def _params(self) -> A.TranslationParams:
        from . import _lib
        p = _lib.translation_params_default()
        p.lm = self.lmParams_.c_params()
        p.use_bilinear = int(self.use_bilinear_translation_factor_)
        p.seed = self.seed_
        return p

    @staticmethod
    def _edges(ms):
        return [(m.key1(), m.key2(), m.vector(), m.noiseModel().kind, m.noiseModel().params) for m in ms]

    def buildGraph(self, relativeTranslations) -> "NonlinearFactorGraph":
        graph = NonlinearFactorGraph()
        for i, edge in enumerate(relativeTranslations):
            if self.use_bilinear_translation_factor_:
                graph.add(BilinearAngleTranslationFactor(edge.key1(), edge.key2(), symbol("S", i), edge.measured(),
                                                         edge.noiseModel()))
            else:
                graph.add(TranslationFactor(edge.key1(), edge.key2(), edge.measured(), edge.noiseModel()))
        return graph

    def addPrior(self, relativeTranslations, scale, betweenTranslations, graph, priorNoiseModel=None):
        relativeTranslations = list(relativeTranslations)
        if not relativeTranslations:
            return
        edge = relativeTranslations[0]
        prior = priorNoiseModel if priorNoiseModel is not None else noiseModel.Isotropic.Sigma(3, 0.01)
        graph.add(PriorFactor(edge.key1(), Point3(0, 0, 0), prior))
        betweenTranslations = list(betweenTranslations)
        if not betweenTranslations:
            graph.add(PriorFactor(edge.key2(), scale * edge.measured().point3(), edge.noiseModel()))
            return
        for b in betweenTranslations:
            graph.add(BetweenFactor(b.key1(), b.key2(), b.measured(), b.noiseModel()))

    def initializeRandomly(self, relativeTranslations, betweenTranslations=(), initialValues=None) -> "Values":
        from . import _lib
        given = {} if initialValues is None else {k: initialValues.at(k) for k in initialValues.keys()}
        # (the edges as they are: a zero direction merges nodes in run(), not here — keep it from merging by asking for the
        # values of the keys alone: the draws depend on the order of first appearance only)
        rel = [(m.key1(), m.key2(), np.array([1.0, 0.0, 0.0]), A.NOISE_UNIT, ()) for m in relativeTranslations]
        btw = [(m.key1(), m.key2(), np.zeros(3), A.NOISE_UNIT, ()) for m in betweenTranslations]
        arr, _ = _lib.translation_recovery_problem(rel, 1.0, btw, given, self._params())
        return Values.unpack(arr.var_keys, arr.var_types, arr.var_dims, arr.values)

    def run(self, relativeTranslations, scale=1.0, betweenTranslations=(), initialValues=None) -> "Values":
        from . import _lib
        given = {} if initialValues is None else {k: initialValues.at(k) for k in initialValues.keys()}
        result, self.lastResult_ = _lib.translation_recovery(self._edges(relativeTranslations), scale,
                                                             self._edges(betweenTranslations), given, self._params())
        out = Values()
        for k in sorted(result):
            out.insert(k, result[k])
        return out

    @staticmethod
    def SimulateMeasurements(poses: "Values", edges) -> List[BinaryMeasurementUnit3]:
        """TranslationRecovery::SimulateMeasurements (TranslationRecovery.cpp:230-243)."""
        model = noiseModel.Isotropic.Sigma(3, 0.01)
        out = []
        for a, b in edges:
            Ta, Tb = poses.at(a).translation(), poses.at(b).translation()
            out.append(BinaryMeasurementUnit3(a, b, Unit3(np.asarray(Tb) - np.asarray(Ta)), model))
        return out


# ---- triangulation (gtsam/geometry/triangulation.h) on the device: include/gsx.h gsx_triangulate* --------------------------
class TriangulationUnderconstrainedException(RuntimeError):
    """triangulation.h:42-48"""

    def __init__(self):
        super().__init__("Triangulation Underconstrained Exception.")


class TriangulationCheiralityException(RuntimeError):
    """triangulation.h:50-56"""

    def __init__(self):
        super().__init__("Triangulation Cheirality Exception: The resulting landmark is behind one or more cameras.")


class PinholeCameraCal3_S2:
    """PinholeCamera<Cal3_S2> (gtsam/geometry/PinholeCamera.h) as far as triangulation needs it."""

    def __init__(self, pose: Optional[Pose3] = None, K: Optional[Cal3_S2] = None):
        self.pose_, self.K_ = pose if pose is not None else Pose3(), K if K is not None else Cal3_S2()

    def pose(self):
        return self.pose_

    def calibration(self):
        return self.K_

    def project(self, point):
        """PinholeCamera::project: raises ValueError behind the camera (CheiralityException)."""
        q = self.pose_.transformTo(np.asarray(point, dtype=float))
        if q[2] <= 0:
            raise ValueError("CheiralityException: landmark behind camera")
        fx, fy, s, u0, v0 = self.K_.v
        x, y = q[0] / q[2], q[1] / q[2]
        return np.array([fx * x + s * y + u0, fy * y + v0])


class TriangulationParameters:
    """TriangulationParameters (triangulation.h:562-607), the reference's constructor order and defaults."""

    def __init__(self, rankTolerance=1.0, enableEPI=False, landmarkDistanceThreshold=-1.0,
                 dynamicOutlierRejectionThreshold=-1.0, useLOST=False, noiseModel=None):
        self.rankTolerance, self.enableEPI = float(rankTolerance), bool(enableEPI)
        self.landmarkDistanceThreshold = float(landmarkDistanceThreshold)
        self.dynamicOutlierRejectionThreshold = float(dynamicOutlierRejectionThreshold)
        self.useLOST, self.noiseModel = bool(useLOST), noiseModel

    def c_params(self, safe=True) -> A.TriangulationParams:
        return _triangulation_c_params(self.rankTolerance, self.enableEPI, self.noiseModel, self.useLOST,
                                       self.landmarkDistanceThreshold, self.dynamicOutlierRejectionThreshold, safe)


def _triangulation_c_params(rank_tol, optimize, model, useLOST, far=-1.0, outlier=-1.0, safe=False) -> A.TriangulationParams:
    p = A.TriangulationParams()
    p.rank_tol, p.optimize, p.use_lost, p.safe = float(rank_tol), int(bool(optimize)), int(bool(useLOST)), int(bool(safe))
    p.landmark_distance_threshold, p.dynamic_outlier_rejection_threshold = float(far), float(outlier)
    p.noise_kind = -1
    if model is not None:
        if model.dim() != 2:
            raise ValueError("TriangulationFactor must be created with 2-dimensional noise model.")
        if model.params.size > 5:
            raise ValueError("triangulation: noise model not supported")
        p.noise_kind = int(model.kind)
        for i, v in enumerate(model.params):
            p.noise[i] = float(v)
    return p


class TriangulationResult:
    """TriangulationResult (triangulation.h:642-698): an optional point and the reason why it is missing."""
    VALID, DEGENERATE, BEHIND_CAMERA, OUTLIER, FAR_POINT = range(5)
    CALIBRATION_FAILED = 5   # Cal3Bundler::calibrate did not converge (the reference's runtime_error)

    def __init__(self, status, point=None):
        self.status = int(status)
        self.point = None if point is None or self.status != self.VALID else np.array(point, dtype=float)

    def valid(self): return self.status == self.VALID
    def degenerate(self): return self.status == self.DEGENERATE
    def outlier(self): return self.status == self.OUTLIER
    def farPoint(self): return self.status == self.FAR_POINT
    def behindCamera(self): return self.status == self.BEHIND_CAMERA

    def get(self):
        if self.point is None:
            raise RuntimeError("TriangulationResult has no value")
        return self.point

    def __repr__(self):
        return f"point = {self.point}" if self.point is not None else f"no point, status = {self.status}"


def _camera_arrays(cameras_or_poses, sharedCal):
    """(camera_kind, cameras, calibrations) of gsx_triangulate from poses + a shared Cal3_S2 / Cal3Bundler, or a camera set"""
    if sharedCal is not None:
        poses = list(cameras_or_poses)
        if isinstance(sharedCal, Cal3Bundler):
            cams = [np.concatenate([p.state(), sharedCal.vector()]) for p in poses]
            return A.CAMERA_CAL3BUNDLER, np.array(cams).reshape(-1, 17), None
        if not isinstance(sharedCal, Cal3_S2):
            raise ValueError("triangulation: only Cal3_S2 and Cal3Bundler calibrations are supported")
        return A.CAMERA_POSE3_CAL3_S2, np.array([p.state() for p in poses]).reshape(-1, 12), sharedCal.vector().reshape(1, 5)
    cams = list(cameras_or_poses)
    if cams and isinstance(cams[0], PinholeCameraCal3Bundler):
        return A.CAMERA_CAL3BUNDLER, np.array([c.state() for c in cams]).reshape(-1, 17), None
    if any(not isinstance(c, PinholeCameraCal3_S2) for c in cams):
        raise ValueError("triangulation: only PinholeCameraCal3_S2 and PinholeCameraCal3Bundler cameras are supported")
    return (A.CAMERA_POSE3_CAL3_S2, np.array([c.pose().state() for c in cams]).reshape(-1, 12),
            np.array([c.calibration().vector() for c in cams]).reshape(-1, 5))


def _triangulate_one(cameras_or_poses, sharedCal, measurements, params):
    from . import _lib
    kind, cams, cal = _camera_arrays(cameras_or_poses, sharedCal)
    z = np.asarray(measurements, dtype=float).reshape(-1, 2)
    if z.shape[0] != cams.shape[0]:
        raise ValueError("triangulation: one measurement per camera")
    n = cams.shape[0]
    pts, st = _lib.triangulate(kind, cams, cal, np.array([0, n], np.int64), np.arange(n, dtype=np.int32), z, params)
    return pts[0], int(st[0])


def triangulatePoint3(*args, **kw):
    """triangulatePoint3(poses, sharedCal, measurements, rank_tol=1e-9, optimize=False, model=None, useLOST=False)
    (triangulation.h:424-475) and its camera-set form triangulatePoint3(cameras, measurements, rank_tol, ...) (:491-549).
    Raises TriangulationUnderconstrainedException / TriangulationCheiralityException."""
    names = ("rank_tol", "optimize", "model", "useLOST")
    if len(args) >= 2 and isinstance(args[1], (Cal3_S2, Cal3Bundler)):
        cams, cal, meas, rest = args[0], args[1], args[2] if len(args) > 2 else kw.pop("measurements"), args[3:]
    else:
        cams, cal, meas, rest = args[0], None, args[1] if len(args) > 1 else kw.pop("measurements"), args[2:]
    opt = dict(rank_tol=1e-9, optimize=False, model=None, useLOST=False)
    opt.update(dict(zip(names, rest)))
    opt.update(kw)
    p = _triangulation_c_params(opt["rank_tol"], opt["optimize"], opt["model"], opt["useLOST"])
    point, status = _triangulate_one(cams, cal, meas, p)
    if status == A.TRI_DEGENERATE:
        raise TriangulationUnderconstrainedException()
    if status == A.TRI_BEHIND_CAMERA:
        raise TriangulationCheiralityException()
    if status == A.TRI_CALIBRATION_FAILED:
        raise RuntimeError("Cal3Bundler::calibrate fails to converge. need a better initialization")
    return point


def triangulatePoint3Batch(cameras, measurements, rank_tol=1e-9, optimize=False, model=None, useLOST=False):
    """triangulatePoint3 for many measurement sets of ONE camera set in one call on the device: measurements (n, m, 2), one
    row of m pixels per track.  Returns (points (n, 3), statuses (n,) of TriangulationResult); a track that is not VALID has
    NaN in its point — nothing is raised per track."""
    from . import _lib
    kind, cams, cal = _camera_arrays(cameras, None)
    z = np.asarray(measurements, dtype=float)
    if z.ndim != 3 or z.shape[1] != cams.shape[0] or z.shape[2] != 2:
        raise ValueError("triangulatePoint3Batch: measurements must be (n, number of cameras, 2)")
    n, m = z.shape[:2]
    return _lib.triangulate(kind, cams, cal, np.arange(n + 1, dtype=np.int64) * m, np.tile(np.arange(m, dtype=np.int32), n),
                            z.reshape(-1, 2), _triangulation_c_params(rank_tol, optimize, model, useLOST))


def triangulateSafe(cameras, measured, params: TriangulationParameters) -> TriangulationResult:
    """triangulateSafe(cameras, measured, params) (triangulation.h:701-758)."""
    point, status = _triangulate_one(cameras, None, measured, params.c_params(safe=True))
    return TriangulationResult(status, point)


def triangulateLandmarks(graph, values: "Values", params: Optional[TriangulationParameters] = None):
    """Every landmark of the graph's GeneralSFMFactor / GenericProjectionFactor observations triangulated at once from the
    cameras of `values` (gsx_triangulate_landmarks): (Values with the VALID landmarks replaced, {landmark key: status})."""
    from . import _lib
    params = params if params is not None else TriangulationParameters()
    arr = graph.to_arrays(values)
    packed, status = _lib.triangulate_landmarks(arr, None, params.c_params(safe=True))
    lm, _, _ = _lib.triangulation_tracks(arr)
    out = Values.unpack(arr.var_keys, arr.var_types, arr.var_dims, packed)
    return out, {int(arr.var_keys[v]): int(s) for v, s in zip(lm, status)}


# ---- smart projection factors (gtsam/slam/SmartProjectionPoseFactor.h, SmartProjectionFactor.h, SmartFactorParams.h) ---------
HESSIAN, IMPLICIT_SCHUR, JACOBIAN_Q, JACOBIAN_SVD = range(4)            # LinearizationMode
IGNORE_DEGENERACY, ZERO_ON_DEGENERACY, HANDLE_INFINITY = range(3)       # DegeneracyMode


class SmartProjectionParams:
    """SmartProjectionParams (SmartFactorParams.h:40-137) with the reference's defaults: HESSIAN, IGNORE_DEGENERACY,
    rankTol 1, enableEPI false, retriangulationThreshold 1e-5, no distance and no outlier threshold.  The backend offers no
    linearization mode (HESSIAN and JACOBIAN_SVD give the same normal equations at lambda = 0) and takes only
    ZERO_ON_DEGENERACY: a factor with another degeneracy mode raises ValueError when its graph is lowered."""

    def __init__(self, linMode=HESSIAN, degMode=IGNORE_DEGENERACY, throwCheirality=False, verboseCheirality=False,
                 retriangulationTh=1e-5):
        self.linearizationMode, self.degeneracyMode = linMode, degMode
        self.triangulation = TriangulationParameters()   # rankTolerance 1.0, enableEPI false, -1, -1
        self.retriangulationThreshold = float(retriangulationTh)
        self.throwCheirality, self.verboseCheirality = throwCheirality, verboseCheirality

    def setLinearizationMode(self, m): self.linearizationMode = m
    def setDegeneracyMode(self, m): self.degeneracyMode = m
    def setRankTolerance(self, v): self.triangulation.rankTolerance = float(v)
    def setEnableEPI(self, v): self.triangulation.enableEPI = bool(v)
    def setLandmarkDistanceThreshold(self, v): self.triangulation.landmarkDistanceThreshold = float(v)
    def setDynamicOutlierRejectionThreshold(self, v): self.triangulation.dynamicOutlierRejectionThreshold = float(v)
    def setRetriangulationThreshold(self, v): self.retriangulationThreshold = float(v)
    def getLinearizationMode(self): return self.linearizationMode
    def getDegeneracyMode(self): return self.degeneracyMode
    def getTriangulationParameters(self): return self.triangulation
    def getRetriangulationThreshold(self): return self.retriangulationThreshold


class SmartProjectionPose3Factor:
    """SmartProjectionPoseFactor<Cal3_S2>(sharedNoiseModel, K[, body_P_sensor][, params]): one factor per track, lowered to
    GSX_F_SMART_PROJECTION.  Limits of the backend (include/gsx.h): 2 to 8 views, an Isotropic or Unit model of dimension 2,
    ZERO_ON_DEGENERACY only."""
    ftype = A.F_SMART_PROJECTION
    MAX_VIEWS = 8

    def __init__(self, model, K: "Cal3_S2", body_P_sensor: Optional["Pose3"] = None,
                 params: Optional[SmartProjectionParams] = None):
        model = model if model is not None else noiseModel.Unit.Create(2)
        if model.dim() != 2 or model.kind not in (A.NOISE_UNIT, A.NOISE_ISOTROPIC):
            raise ValueError("SmartFactorBase: needs isotropic (an Isotropic or Unit model of dimension 2)")
        self.noise, self.K_ = model, K
        self.sensor_ = None if body_P_sensor is None else _sensor_state(body_P_sensor, Pose3)
        self.params_ = params if params is not None else SmartProjectionParams()
        self.keys_: List[int] = []
        self.measured_: List[np.ndarray] = []
        self._result = TriangulationResult(TriangulationResult.DEGENERATE)   # (the reference's default-constructed result_)

    def add(self, measured, key):
        if int(key) in self.keys_:
            raise ValueError("SmartFactorBase::add: adding duplicate measurement for key.")
        self.measured_.append(np.asarray(measured, dtype=float).reshape(2))
        self.keys_.append(int(key))

    def keys(self): return list(self.keys_)
    def measured(self): return [m.copy() for m in self.measured_]
    def size(self): return len(self.keys_)

    @property
    def rows(self):
        return 2 * len(self.keys_) - 3

    @property
    def meas(self):
        p, t = self.params_, self.params_.triangulation
        if p.degeneracyMode != ZERO_ON_DEGENERACY:
            raise ValueError("SmartProjectionPose3Factor: the backend takes only ZERO_ON_DEGENERACY (IGNORE_DEGENERACY and "
                             "HANDLE_INFINITY need the point at infinity); set params.setDegeneracyMode(ZERO_ON_DEGENERACY)")
        if not 2 <= len(self.keys_) <= self.MAX_VIEWS:
            raise ValueError(f"SmartProjectionPose3Factor: {len(self.keys_)} views; the backend takes 2 to {self.MAX_VIEWS}")
        head = [self.K_.vector(), [t.rankTolerance, float(t.enableEPI), t.landmarkDistanceThreshold,
                                   t.dynamicOutlierRejectionThreshold, p.retriangulationThreshold, float(p.degeneracyMode)]]
        if self.sensor_ is not None:
            head.append(self.sensor_)
        return np.concatenate(head + self.measured_)

    def point(self) -> "TriangulationResult":
        """The result of the last triangulation a backend did for this factor (after an optimizer's optimize() / values() /
        error(), or this factor's own error(values))."""
        return self._result

    def error(self, values: "Values", backend_factory=None) -> float:
        g = NonlinearFactorGraph()
        g.add(self)
        sub = Values()
        for k in self.keys_:
            sub.insert(k, values.at(k))
        be = _make_backend(g.to_arrays(sub), backend_factory)
        try:
            e = be.error()
            _sync_smart_results(g, be)
            return e
        finally:
            be.close()


def _sync_smart_results(graph, backend):
    """SmartProjectionFactor::point(): copy the handle's last triangulations into the graph's smart factors"""
    # (an optimizer accepts any object that lowers itself with to_arrays: only a graph with a factor list can hold smart factors)
    smart = [f for f in getattr(graph, "factors", ()) if f is not None and getattr(f, "ftype", None) == A.F_SMART_PROJECTION]
    if not smart or not hasattr(backend, "smart_points"):
        return
    pts, st = backend.smart_points()
    for f, p, s in zip(smart, pts, st):
        f._result = TriangulationResult(s if s >= 0 else TriangulationResult.DEGENERATE, p)


def _make_backend(arrays, backend_factory):
    if backend_factory is None:
        from ._lib import product_backend
        backend_factory = product_backend
    return backend_factory(arrays)


# ---- optimizers ---------------------------------------------------------------------------------
class DummyPreconditionerParameters:
    """gtsam/linear/Preconditioner.h: the identity."""
    kind = A.PRECOND_DUMMY


class BlockJacobiPreconditionerParameters:
    """gtsam/linear/Preconditioner.h: Cholesky factors of the diagonal blocks of the damped Hessian."""
    kind = A.PRECOND_BLOCK_JACOBI


class PCGSolverParameters:
    """gtsam/linear/PCGSolver.h:36-50 over ConjugateGradientParameters (ConjugateGradientSolver.h:29-96), with its
    setter names.  The subgraph preconditioner is not offered by the backend."""

    def __init__(self, preconditioner=None):
        self.minIterations, self.maxIterations, self.reset = 1, 500, 501
        self.epsilon_rel, self.epsilon_abs = 1e-3, 1e-3
        self.preconditioner = preconditioner if preconditioner is not None else BlockJacobiPreconditionerParameters()

    def setMinIterations(self, v): self.minIterations = int(v)
    def setMaxIterations(self, v): self.maxIterations = int(v)
    def setReset(self, v): self.reset = int(v)
    def setEpsilon(self, v): self.epsilon_rel = float(v)
    def setEpsilon_rel(self, v): self.epsilon_rel = float(v)
    def setEpsilon_abs(self, v): self.epsilon_abs = float(v)
    def setPreconditionerParams(self, p): self.preconditioner = p

    def c_params(self) -> A.PCGParams:
        return A.PCGParams(int(self.maxIterations), int(self.minIterations), int(self.reset), float(self.epsilon_rel),
                           float(self.epsilon_abs), int(self.preconditioner.kind))


def _route_linear_solver(backend, linearSolverType, iterativeParams):
    """NonlinearOptimizerParams::linearSolverType (NonlinearOptimizerParams.h:81-108): "ITERATIVE" with
    PCGSolverParameters goes to gsx_set_linear_solver; the direct kinds all mean the multifrontal Cholesky here."""
    if str(linearSolverType).upper() == "ITERATIVE":
        if not isinstance(iterativeParams, PCGSolverParameters):
            raise ValueError("linearSolverType ITERATIVE needs iterativeParams = PCGSolverParameters (the subgraph "
                             "solver is not offered)")
        backend.set_linear_solver(A.SOLVER_PCG, iterativeParams.c_params())


class GaussNewtonParams:
    """gtsam/nonlinear/GaussNewtonParams.h = NonlinearOptimizerParams (NonlinearOptimizerParams.h:42-108)."""

    def __init__(self):
        self.maxIterations, self.relativeErrorTol, self.absoluteErrorTol, self.errorTol = 100, 1e-5, 1e-5, 0.0
        self.ordering: Optional[Ordering] = None
        self.orderingType = "COLAMD"
        self.linearSolverType = "MULTIFRONTAL_CHOLESKY"
        self.iterativeParams = None


class LevenbergMarquardtParams:
    """gtsam/nonlinear/LevenbergMarquardtParams.h:61-98 + NonlinearOptimizerParams.h:42-108."""
    SILENT, SUMMARY = 0, 1

    def __init__(self):
        self._set(A.lm_params_legacy())
        # the class default lambdaInitial/lambdaFactor etc. ARE the legacy values;
        self.ordering: Optional[Ordering] = None
        self.orderingType = "COLAMD"
        self.linearSolverType = "MULTIFRONTAL_CHOLESKY"   # or "ITERATIVE" with iterativeParams = PCGSolverParameters
        self.iterativeParams = None

    def _set(self, p: A.LMParams):
        self.maxIterations, self.relativeErrorTol = p.max_iterations, p.relative_error_tol
        self.absoluteErrorTol, self.errorTol = p.absolute_error_tol, p.error_tol
        self.lambdaInitial, self.lambdaFactor = p.lambda_initial, p.lambda_factor
        self.lambdaUpperBound, self.lambdaLowerBound = p.lambda_upper_bound, p.lambda_lower_bound
        self.minModelFidelity = p.min_model_fidelity
        self.diagonalDamping = bool(p.diagonal_damping)
        self.useFixedLambdaFactor = bool(p.use_fixed_lambda_factor)
        self.minDiagonal, self.maxDiagonal = p.min_diagonal, p.max_diagonal
        self.verbosityLM = p.verbosity

    @staticmethod
    def LegacyDefaults():
        return LevenbergMarquardtParams()

    @staticmethod
    def CeresDefaults():
        p = LevenbergMarquardtParams()
        p._set(A.lm_params_ceres())
        return p

    def c_params(self) -> A.LMParams:
        return A.LMParams(self.maxIterations, self.relativeErrorTol, self.absoluteErrorTol, self.errorTol,
                          self.lambdaInitial, self.lambdaFactor, self.lambdaUpperBound, self.lambdaLowerBound,
                          self.minModelFidelity, int(self.diagonalDamping), int(self.useFixedLambdaFactor),
                          self.minDiagonal, self.maxDiagonal, int(self.verbosityLM))


class _OptimizerBase:
    def __init__(self, graph, initialValues, ordering, orderingType, backend_factory, ordering_fn):
        self.graph_ = graph
        self.arrays = graph.to_arrays(initialValues)
        self.backend = _make_backend(self.arrays, backend_factory)
        if ordering is None:
            # EnsureHasOrdering (LevenbergMarquardtParams.h:112-117): the reference calls
            # Ordering::Create(orderingType, graph) here.  A caller-supplied ordering_fn lets the
            # tests feed the reference's own CCOLAMD result; otherwise the library's own ordering.
            if ordering_fn is not None:
                ordering = ordering_fn(self.arrays)
            else:
                kind = {"COLAMD": A.ORDER_MINDEGREE, "METIS": A.ORDER_ND, "NATURAL": A.ORDER_NATURAL,
                        "SCHUR": A.ORDER_SCHUR, "SCHUR_ND": A.ORDER_SCHUR_ND}[orderingType]
                ordering = self.backend.compute_ordering(kind)
        self.ordering = Ordering(int(k) for k in ordering)
        self.backend.set_ordering(self.ordering)
        self.result = None

    def values(self) -> Values:
        _sync_smart_results(self.graph_, self.backend)
        return Values.unpack(self.arrays.var_keys, self.arrays.var_types, self.arrays.var_dims,
                             self.backend.get_values())

    def error(self) -> float:
        e = self.backend.error()
        _sync_smart_results(self.graph_, self.backend)
        return e

    def iterations(self) -> int:
        return self.result["iterations"] if self.result else self._iterations


class LevenbergMarquardtOptimizer(_OptimizerBase):
    """LevenbergMarquardtOptimizer(graph, initialValues[, ordering][, params])."""

    def __init__(self, graph, initialValues, *args, backend_factory=None, ordering_fn=None):
        params, ordering = LevenbergMarquardtParams(), None
        for a in args:
            if isinstance(a, LevenbergMarquardtParams):
                params = a
            elif a is not None:
                ordering = a
        if ordering is None:
            ordering = params.ordering
        self.params_ = params
        super().__init__(graph, initialValues, ordering, params.orderingType, backend_factory, ordering_fn)
        _route_linear_solver(self.backend, params.linearSolverType, params.iterativeParams)
        self.backend.lm_reset(params.c_params())
        self._iterations = 0
        self._lambda = params.lambdaInitial

    def optimize(self) -> Values:
        self.result = self.backend.lm_optimize(self.params_.c_params())
        self._lambda = self.result["final_lambda"]
        return self.values()

    def iterate(self):
        err, lam = self.backend.lm_iterate(self.params_.c_params())
        self._iterations += 1
        self._lambda = lam
        return err

    def lambda_(self) -> float:
        return self._lambda


class DoglegOptimizer(_OptimizerBase):
    """gtsam/nonlinear/DoglegOptimizer.h: DoglegParams::deltaInitial = 1.0, NonlinearOptimizerParams defaults."""

    def __init__(self, graph, initialValues, ordering=None, deltaInitial=1.0, maxIterations=100, relativeErrorTol=1e-5,
                 absoluteErrorTol=1e-5, errorTol=0.0, backend_factory=None, ordering_fn=None, orderingType="COLAMD"):
        super().__init__(graph, initialValues, ordering, orderingType, backend_factory, ordering_fn)
        self._p = (deltaInitial, maxIterations, relativeErrorTol, absoluteErrorTol, errorTol)

    def optimize(self) -> Values:
        self.result = self.backend.dogleg_optimize(*self._p)
        return self.values()

    def getDelta(self) -> float:
        return float(self.result["final_lambda"])


class GaussNewtonOptimizer(_OptimizerBase):
    def __init__(self, graph, initialValues, ordering=None, maxIterations=100, relativeErrorTol=1e-5,
                 absoluteErrorTol=1e-5, errorTol=0.0, backend_factory=None, ordering_fn=None, orderingType="COLAMD",
                 params: Optional["GaussNewtonParams"] = None):
        if params is not None:   # GaussNewtonOptimizer(graph, initialValues, params)
            maxIterations, relativeErrorTol = params.maxIterations, params.relativeErrorTol
            absoluteErrorTol, errorTol, orderingType = params.absoluteErrorTol, params.errorTol, params.orderingType
            ordering = ordering if ordering is not None else params.ordering
        super().__init__(graph, initialValues, ordering, orderingType, backend_factory, ordering_fn)
        if params is not None:
            _route_linear_solver(self.backend, params.linearSolverType, params.iterativeParams)
        self._p = (maxIterations, relativeErrorTol, absoluteErrorTol, errorTol)
        self._iterations = 0

    def optimize(self) -> Values:
        self.result = self.backend.gn_optimize(*self._p)
        return self.values()


class JointMarginal:
    """gtsam/nonlinear/Marginals.h:140-190: blocks of a joint covariance by key; keys sorted as the reference returns them."""

    def __init__(self, matrix, keys, dims):
        self._m, self._keys = matrix, list(keys)
        self._off = dict(zip(self._keys, np.concatenate([[0], np.cumsum(dims)[:-1]]).astype(int)))
        self._dim = dict(zip(self._keys, dims))

    def at(self, iVariable, jVariable):
        i, j = self._off[iVariable], self._off[jVariable]
        return self._m[i:i + self._dim[iVariable], j:j + self._dim[jVariable]]

    __call__ = at

    def fullMatrix(self):
        return self._m

    def keys(self):
        return list(self._keys)


class Marginals:
    """gtsam/nonlinear/Marginals.h:32-138 on the device factorization: Marginals(graph, solution).marginalCovariance(key),
    .marginalInformation(key), .jointMarginalCovariance(keys), .jointMarginalInformation(keys).  (The reference's
    CHOLESKY / QR switch has no counterpart: the Bayes tree here is always the Cholesky one.)"""

    def __init__(self, graph, solution, ordering=None, backend_factory=None, orderingType="COLAMD"):
        self.arrays = graph.to_arrays(solution)
        self.backend = _make_backend(self.arrays, backend_factory)
        if ordering is None:
            kind = {"COLAMD": A.ORDER_MINDEGREE, "METIS": A.ORDER_ND, "NATURAL": A.ORDER_NATURAL}[orderingType]
            ordering = self.backend.compute_ordering(kind)
        self.backend.set_ordering([int(k) for k in ordering])
        self.backend.linearize()
        self._blocks = {}

    def marginalCovariance(self, key):
        if int(key) in self._blocks:
            return self._blocks[int(key)].copy()
        return self.backend.marginal_covariance(key)

    def marginalCovariances(self, keys=None) -> dict:
        """The marginal covariance of every listed variable (None: all of them) as {key: d x d}, from one top-down pass
        over the device factorization instead of one query per variable; marginalCovariance(key) serves from the
        result afterwards (a Marginals object stands for one fixed linearization, as the reference's does)."""
        res = self.backend.marginal_covariances(None if keys is None else [int(k) for k in keys])
        self._blocks.update(res)
        return {k: v.copy() for k, v in res.items()}

    def marginalInformation(self, key):
        return np.linalg.inv(self.marginalCovariance(key))

    def jointMarginalCovariance(self, variables) -> JointMarginal:
        keys = sorted(int(k) for k in variables)
        dims = [int(self.arrays.var_dims[int(np.searchsorted(self.arrays.var_keys, np.uint64(k)))]) for k in keys]
        return JointMarginal(self.backend.joint_marginal_covariance(keys), keys, dims)

    def jointMarginalInformation(self, variables) -> JointMarginal:
        j = self.jointMarginalCovariance(variables)
        return JointMarginal(np.linalg.inv(j.fullMatrix()), j.keys(), [j._dim[k] for k in j.keys()])
