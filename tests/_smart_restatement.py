"""Restatement of the reference's smart projection factor (gtsam/slam/SmartProjectionPoseFactor.h, SmartProjectionFactor.h,
SmartFactorBase.h, gtsam/geometry/CameraSet.h SchurComplement, CalibratedCamera.cpp:27-46, Pose3.cpp:61-75,169-171), written
from those lines: once in float64 (FLOAT) and, with the same code on mpmath numbers, at 50 digits (MP).  Test infrastructure:
nothing of the product is imported here.

The route is the reference's own, not the product's: triangulateSafe from tests/_triangulation_restatement.py, F, E and b per
view, Cameras::SchurComplement with the EXPLICIT (E'E)^-1, and the stateful re-triangulation cache of decideIfTriangulate.
Every comparison a branch is taken on is recorded in SmartFactor.decisions as (name, value, threshold, scale)."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from ._triangulation_restatement import (FLOAT, MP, VALID, DEGENERATE, Camera, Params, triangulate, _Cam)  # noqa: F401

NEVER = -1


@dataclass
class Spec:
    """one SmartProjectionPoseFactor<Cal3_S2>: K = (fx, fy, s, u0, v0); sensor = None or (R 3x3, t 3); pixels [nk, 2]"""
    K: np.ndarray
    pixels: np.ndarray
    sigma: float = 1.0
    rank_tol: float = 1.0
    enable_epi: bool = False
    landmark_distance_threshold: float = -1.0
    outlier_threshold: float = -1.0
    retriangulation_threshold: float = 1e-5
    sensor: tuple = None
    views: list = field(default_factory=list)   # indices into the pose list the factor is evaluated on

    @property
    def nk(self):
        return len(self.pixels)


def _obj(a, X):
    return np.array([[X.num(v) for v in row] for row in np.asarray(a, float)], dtype=object)


def _skew(t, X):
    z = X.num(0)
    return np.array([[z, -t[2], t[1]], [t[2], z, -t[0]], [-t[1], t[0], z]], dtype=object)


def _adjoint_inverse(sensor, X):
    """AdjointMap(body_P_sensor^-1) (Pose3.cpp:61-75 on Pose3::inverse): the Jacobian of world_P_body.compose(body_P_sensor)
    with respect to world_P_body"""
    Rs, ts = _obj(np.asarray(sensor[0], float).reshape(3, 3), X), np.array([X.num(v) for v in sensor[1]], dtype=object)
    Ri, ti = Rs.T, -Rs.T.dot(ts)
    A = np.full((6, 6), X.num(0), dtype=object)
    A[:3, :3] = Ri
    A[3:, 3:] = Ri
    A[3:, :3] = _skew(ti, X).dot(Ri)
    return A


def _inv3(M):
    a, b, c, d, e, f, g, h, i = [M[r][q] for r in range(3) for q in range(3)]
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    adj = np.array([[e * i - f * h, c * h - b * i, b * f - c * e], [f * g - d * i, a * i - c * g, c * d - a * f],
                    [d * h - e * g, b * g - a * h, a * e - b * d]], dtype=object)
    return adj / det


class SmartFactor:
    """the factor with its mutable cache (cameraPosesTriangulation_, result_) in the arithmetic X"""

    def __init__(self, spec: Spec, X=FLOAT):
        self.spec, self.X = spec, X
        self.cached = None          # camera poses (R, t) of the last triangulation
        self.status, self.point = NEVER, None
        self.n_triangulations = 0
        self.decisions = []
        self.tri = None
        self.grad_norm = X.num(0)   # |E'b| of the last linearization: the slope of the error in the point

    def _cameras(self, poses):
        s = self.spec
        return [Camera(np.asarray(p[:9], float).reshape(3, 3), np.asarray(p[9:12], float), s.K) for p in poses]

    def _cams(self, poses):
        s = self.spec
        return [_Cam(c, self.X, s.sensor) for c in self._cameras(poses)]

    def _equals(self, a, b, tol):   # Pose3::equals -> fpEqual(a, b, tol, false) on the 12 entries (finite values)
        worst = max(abs(x - y) for x, y in zip(list(a.R.reshape(-1)) + list(a.t), list(b[0].reshape(-1)) + list(b[1])))
        if tol > 0:
            self.decisions.append(("pose_entry", worst, tol, tol))
        return worst <= tol

    def triangulate_safe(self, poses):
        """SmartProjectionFactor::triangulateSafe (:173-184): True when this call re-triangulated"""
        s = self.spec
        cams = self._cams(poses)
        retri = self.cached is None or len(self.cached) != len(cams)
        if not retri:
            for c, old in zip(cams, self.cached):
                if not self._equals(c, old, s.retriangulation_threshold):
                    retri = True
                    break
        if retri:
            self.cached = [(c.R.copy(), c.t.copy()) for c in cams]
            prm = Params(rank_tol=s.rank_tol, optimize=s.enable_epi, use_lost=False, noise=None,
                         landmark_distance_threshold=s.landmark_distance_threshold, outlier_threshold=s.outlier_threshold,
                         safe=True)
            res = triangulate(self._cameras(poses), s.pixels, prm, self.X,
                              None if s.sensor is None else [s.sensor] * s.nk)
            self.decisions += res.decisions
            self.tri = res              # (the linear system and its singular values: the bounds of the cases file)
            self.status = res.status
            self.point = res.point if res.status == VALID else None
            self.n_triangulations += 1
        return retri

    def jacobians(self, poses, point=None):
        """whitened F (list of 2 x 6), E (2 nk x 3), b (2 nk) at the cached point (SmartFactorBase::computeJacobians +
        whitenJacobians); None when a view fails the cheirality test"""
        X, s = self.X, self.spec
        n = X.num
        p = np.array([n(v) for v in (self.point if point is None else point)], dtype=object)
        inv = 1 / n(s.sigma)
        Fs, Es, bs = [], [], []
        adj = None if s.sensor is None else _adjoint_inverse(s.sensor, X)
        for c, z in zip(self._cams(poses), s.pixels):
            q = c.to_camera(p)
            if not q[2] > 0:
                return None
            d = 1 / q[2]
            u, v = q[0] * d, q[1] * d
            pi, Dpi = c.uncalibrate(u, v, True)
            Dpose = np.array([[u * v, -1 - u * u, v, -d, n(0), d * u], [1 + v * v, -u * v, -u, n(0), -d, d * v]], dtype=object)
            F = Dpi.dot(Dpose)
            if adj is not None:
                F = F.dot(adj)
            Dpoint = d * np.array([[n(1), n(0), -u], [n(0), n(1), -v]], dtype=object).dot(c.R.T)
            Fs.append(F * inv)
            Es.append(Dpi.dot(Dpoint) * inv)
            bs.append(np.array([n(z[0]) - pi[0], n(z[1]) - pi[1]], dtype=object) * inv)
        return Fs, np.concatenate(Es, axis=0), np.concatenate(bs)

    def hessian(self, poses):
        """linearize: the augmented Hessian [[G, g], [g', f]] (6 nk + 1 square) of createHessianFactor (:198-237) through
        Cameras::SchurComplement with the explicit point covariance; zeros without a valid point.  Also returns
        (|[F b]|_F^2, cond_2(E)) for the bounds of the cases file (0, 1 without a point)."""
        X, s = self.X, self.spec
        self.triangulate_safe(poses)
        D = 6 * s.nk + 1
        Z = np.full((D, D), X.num(0), dtype=object)
        jac = self.jacobians(poses) if self.status == VALID else None
        if jac is None:
            return Z, X.num(0), X.num(1)
        Fs, E, b = jac
        F = np.full((2 * s.nk, 6 * s.nk), X.num(0), dtype=object)
        for i, Fi in enumerate(Fs):
            F[2 * i:2 * i + 2, 6 * i:6 * i + 6] = Fi
        Fb = np.concatenate([F, b.reshape(-1, 1)], axis=1)
        P = _inv3(E.T.dot(E))
        EtFb = E.T.dot(Fb)
        self.grad_norm = X.sqrt(sum(x * x for x in EtFb[:, -1]))
        H = Fb.T.dot(Fb) - EtFb.T.dot(P).dot(EtFb)
        sv, _ = X.svd([list(r) for r in E])
        return H, sum(x * x for x in Fb.reshape(-1)), sv[0] / sv[2]

    def error(self, poses):
        """totalReprojectionError (:411-430) under ZERO_ON_DEGENERACY"""
        X, s = self.X, self.spec
        self.triangulate_safe(poses)
        if self.status != VALID:
            return X.num(0)
        total = X.num(0)
        p = np.array([X.num(v) for v in self.point], dtype=object)
        for c, z in zip(self._cams(poses), s.pixels):
            pi = c.project(p)
            if pi is None:
                return X.num(0)
            e0, e1 = (pi[0] - X.num(z[0])) / X.num(s.sigma), (pi[1] - X.num(z[1])) / X.num(s.sigma)
            total += e0 * e0 + e1 * e1
        return total / 2

    def point_float(self):
        return np.full(3, np.nan) if self.point is None else np.array([float(v) for v in self.point])
