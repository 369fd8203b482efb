"""Restatement of the reference's triangulation (gtsam/geometry/triangulation.{h,cpp}, gtsam/slam/TriangulationFactor.h,
gtsam/geometry/Cal3Bundler.cpp:64-128, gtsam/base/Matrix.cpp:556-574, gtsam/nonlinear/LevenbergMarquardtOptimizer.cpp:121-270,
NonlinearOptimizer.cpp:62-117,182-231), written from those lines: once in numpy float64 (FLOAT) and, with the same code on
mpmath numbers, at 50 digits (MP), as tests/_mp_restatement.py does for the factors.  Test infrastructure: nothing of the
product is imported here.

The linear algebra is the reference's own choice, not the product's: an SVD of the 2m x 4 matrix A (numpy / mpmath.svd_r),
a column-pivoted Householder QR of the 2m x 3 LOST system.  Every comparison the reference takes a branch on is recorded in
Result.decisions as (name, value, threshold, scale), so that a test can assert that no case sits on a threshold."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import mpmath
import numpy as np

VALID, DEGENERATE, BEHIND_CAMERA, OUTLIER, FAR_POINT, CALIBRATION_FAILED = range(6)
N_UNIT, N_ISOTROPIC, N_DIAGONAL, N_GAUSSIAN = range(4)
HUBER, TUKEY, CAUCHY = 1 << 4, 2 << 4, 3 << 4


class FLOAT:
    name = "float64"
    num = staticmethod(float)
    sqrt = staticmethod(math.sqrt)
    log1p = staticmethod(math.log1p)
    eps = 2.220446049250313e-16

    @staticmethod
    def svd(A):   # singular values (descending) and V
        _, s, vt = np.linalg.svd(np.array(A, dtype=np.float64), full_matrices=True)
        return list(s), vt.T


class MP:
    name = "mp50"
    num = staticmethod(lambda x: mpmath.mpf(x))
    sqrt = staticmethod(mpmath.sqrt)
    log1p = staticmethod(mpmath.log1p)
    eps = mpmath.mpf(2.220446049250313e-16)   # the reference's numeric_limits<double>::epsilon() is a constant of the policy

    @staticmethod
    def svd(A):
        _, s, v = mpmath.svd_r(mpmath.matrix([[x for x in row] for row in A]), full_matrices=True, compute_uv=True)
        n = len(A[0])
        vt = np.array([[v[i, j] for j in range(n)] for i in range(n)], dtype=object)
        return [s[i] for i in range(len(s))], vt.T


mpmath.mp.dps = 50


@dataclass
class Camera:
    """kind 0: Pose3 + Cal3_S2 (K = fx, fy, s, u0, v0); kind 1: PinholeCamera<Cal3Bundler> (K = f, k1, k2, u0, v0)"""
    R: np.ndarray
    t: np.ndarray
    K: np.ndarray
    kind: int = 0

    def state(self):
        return np.concatenate([np.asarray(self.R, float).reshape(9), np.asarray(self.t, float), np.asarray(self.K, float)])


@dataclass
class Params:
    """TriangulationParameters + triangulatePoint3's arguments; noise = None or (kind, params)"""
    rank_tol: float = 1e-9
    optimize: bool = False
    use_lost: bool = False
    noise: tuple = None
    landmark_distance_threshold: float = -1.0
    outlier_threshold: float = -1.0
    safe: bool = False


@dataclass
class Result:
    status: int
    point: np.ndarray
    iterations: int = 0
    trials: int = 0
    linear_point: np.ndarray = None      # the point of the linear stage (before refinement)
    sigma: list = None                   # DLT: singular values of A, descending; LOST: |pivots|
    A: np.ndarray = None                 # the linear system (DLT: 2m x 4; LOST: 2m x 4 = [A b])
    decisions: list = field(default_factory=list)


class _Cam:
    """a camera in the arithmetic X"""

    def __init__(self, c: Camera, X, sensor=None):
        n = X.num
        R = np.array([[n(v) for v in row] for row in np.asarray(c.R, float).reshape(3, 3)], dtype=object)
        t = np.array([n(v) for v in np.asarray(c.t, float)], dtype=object)
        if sensor is not None:   # pose.compose(body_P_sensor)
            Rs = np.array([[n(v) for v in row] for row in np.asarray(sensor[0], float).reshape(3, 3)], dtype=object)
            ts = np.array([n(v) for v in np.asarray(sensor[1], float)], dtype=object)
            t = t + R.dot(ts)
            R = R.dot(Rs)
        self.R, self.t, self.X = R, t, X
        k = [n(v) for v in np.asarray(c.K, float)]
        if c.kind == 1:
            self.fx, self.fy, self.s, self.u0, self.v0, self.k1, self.k2 = k[0], k[0], n(0), k[3], k[4], k[1], k[2]
        else:
            self.fx, self.fy, self.s, self.u0, self.v0, self.k1, self.k2 = k[0], k[1], k[2], k[3], k[4], n(0), n(0)
        self.distorted = c.kind == 1

    def Kmat(self):
        z, o = self.X.num(0), self.X.num(1)
        return np.array([[self.fx, self.s, self.u0], [z, self.fy, self.v0], [z, z, o]], dtype=object)

    def projection_matrix(self):   # K [R' | -R' t]
        E = np.concatenate([self.R.T, (-self.R.T.dot(self.t)).reshape(3, 1)], axis=1)
        return self.Kmat().dot(E)

    def uncalibrate(self, x, y, jac=False):   # Cal3Bundler.cpp:64-90 / Cal3_S2.cpp:54-62
        r = x * x + y * y
        g = 1 + (self.k1 + self.k2 * r) * r
        u, v = g * x, g * y
        pi = (self.fx * u + self.s * v + self.u0, self.fy * v + self.v0)
        if not jac:
            return pi
        a = 2 * (self.k1 + 2 * self.k2 * r)
        D = np.array([[g + a * x * x, a * x * y], [a * x * y, g + a * y * y]], dtype=object)
        Kp = np.array([[self.fx, self.s], [self.X.num(0), self.fy]], dtype=object)
        return pi, Kp.dot(D)

    def calibrate(self, z):   # Cal3_S2.cpp:64-75 / Cal3Bundler.cpp:93-128; None where the reference throws
        py0 = (z[1] - self.v0) / self.fy
        px0 = (z[0] - self.u0 - self.s * py0) / self.fx
        if not self.distorted:
            return px0, py0
        px, py = px0, py0
        for _ in range(10):
            rr = px * px + py * py
            g = 1 + self.k1 * rr + self.k2 * rr * rr
            pn = (px0 / g, py0 / g)
            pi = self.uncalibrate(*pn)
            if self.X.sqrt((pi[0] - z[0]) ** 2 + (pi[1] - z[1]) ** 2) <= 1e-5:
                return pn
            px, py = pn
        return None

    def to_camera(self, p):
        return self.R.T.dot(p - self.t)

    def project(self, p, jac=False):   # None on cheirality (z <= 0)
        q = self.to_camera(p)
        if not q[2] > 0:
            return None
        d = 1 / q[2]
        u, v = q[0] * d, q[1] * d
        if not jac:
            return np.array(self.uncalibrate(u, v), dtype=object)
        pi, Dp = self.uncalibrate(u, v, True)
        o, z = self.X.num(1), self.X.num(0)
        Dpn = d * np.array([[o, z, -u], [z, o, -v]], dtype=object).dot(self.R.T)
        return np.array(pi, dtype=object), Dp.dot(Dpn)


def _whiten(noise, X, v):
    """v: a 2-vector or a 2 x k matrix (object array); the base model's whitening"""
    if noise is None:
        return v
    base, p = noise[0] & 15, [X.num(x) for x in noise[1]]
    if base == N_ISOTROPIC:
        return v / p[0]
    if base == N_DIAGONAL:
        W = np.array([[1 / p[0], X.num(0)], [X.num(0), 1 / p[1]]], dtype=object)
        return W.dot(v)
    if base == N_GAUSSIAN:
        W = np.array([[p[0], p[1]], [X.num(0), p[3]]], dtype=object)
        return W.dot(v)
    return v


def _nparams(base):
    return {N_UNIT: 0, N_ISOTROPIC: 1, N_DIAGONAL: 2, N_GAUSSIAN: 4}[base]


def _robust(noise, X):
    if noise is None or noise[0] >> 4 == 0:
        return 0, None
    return noise[0] >> 4, X.num(noise[1][_nparams(noise[0] & 15)])


def _weight(loss, k, dist):
    a = abs(dist)
    if loss == 1:
        return 1 if a <= k else k / a
    if loss == 2:
        return 0 if a > k else (1 - dist * dist / (k * k)) ** 2
    return (k * k) / (k * k + dist * dist)


def _loss(loss, k, dist, X):
    a = abs(dist)
    if loss == 1:
        return dist * dist / 2 if a <= k else k * (a - k / 2)
    if loss == 2:
        return k * k / 6 if a > k else k * k * (1 - (1 - dist * dist / (k * k)) ** 3) / 6
    return k * k * X.log1p(dist * dist / (k * k)) / 2


def lost_sigma(noise):
    """model ? model->sigmas().mean() : 1e-4 (triangulation.h:439); a robust model: its base model's"""
    if noise is None:
        return 1e-4
    base, p = noise[0] & 15, noise[1]
    if base == N_UNIT:
        return 1.0
    if base == N_ISOTROPIC:
        return float(p[0])
    if base == N_DIAGONAL:
        return 0.5 * (p[0] + p[1])
    a, b, c = p[0], p[1], p[3]
    return 0.5 * (math.sqrt(b * b + c * c) / abs(a * c) + 1.0 / abs(c))


def _factor(cam, z, p, X, jac):
    """TriangulationFactor::evaluateError (TriangulationFactor.h:122-136)"""
    r = cam.project(p, jac)
    if r is None:
        e = np.array([2 * cam.fx, 2 * cam.fx], dtype=object)
        return (e, np.array([[X.num(0)] * 3] * 2, dtype=object)) if jac else e
    if jac:
        return r[0] - z, r[1]
    return r - z


def _error(cams, Z, p, noise, X):
    loss, k = _robust(noise, X)
    total = X.num(0)
    for cam, z in zip(cams, Z):
        e = _whiten(noise, X, _factor(cam, z, p, X, False))
        sq = e[0] * e[0] + e[1] * e[1]
        total += _loss(loss, k, X.sqrt(sq), X) if loss else sq / 2
    return total


def _solve3(H, g, X):
    """Cholesky of a 3 x 3; None when not positive definite"""
    L = [[X.num(0)] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(i + 1):
            s = H[i][j] - sum(L[i][k] * L[j][k] for k in range(j))
            if i == j:
                if not s > 0:
                    return None
                L[i][j] = X.sqrt(s)
            else:
                L[i][j] = s / L[j][j]
    y = [X.num(0)] * 3
    for i in range(3):
        y[i] = (g[i] - sum(L[i][k] * y[k] for k in range(i))) / L[i][i]
    x = [X.num(0)] * 3
    for i in (2, 1, 0):
        x[i] = (y[i] - sum(L[k][i] * x[k] for k in range(i + 1, 3))) / L[i][i]
    return np.array(x, dtype=object)


def _refine(cams, Z, p, noise, X, dec):
    """optimize (triangulation.cpp:177-195): LevenbergMarquardtOptimizer with lambdaInitial 1, lambdaFactor 10,
    maxIterations 100, absoluteErrorTol 1.0, relativeErrorTol 1e-5, errorTol 0, lambdaUpperBound 1e5, minModelFidelity 1e-3"""
    loss, rk = _robust(noise, X)
    lam, factor, iterations, trials = X.num(1), 10, 0, 0
    cost = _error(cams, Z, p, noise, X)
    if cost <= 0:
        return p, 0, 0
    new_error = cost
    while True:
        current_error = new_error
        H = np.array([[X.num(0)] * 3] * 3, dtype=object)
        g = np.array([X.num(0)] * 3, dtype=object)
        f0 = X.num(0)
        for cam, z in zip(cams, Z):
            e, J = _factor(cam, z, p, X, True)
            b = _whiten(noise, X, -e)
            A = _whiten(noise, X, J)
            if loss:
                w = X.sqrt(_weight(loss, rk, X.sqrt(b[0] * b[0] + b[1] * b[1])))
                b, A = b * w, A * w
            H = H + A.T.dot(A)
            g = g + A.T.dot(b)
            f0 += (b[0] * b[0] + b[1] * b[1]) / 2
        while True:   # tryLambda
            Hd = H + lam * np.diag([X.num(1)] * 3)
            dx = _solve3(Hd.tolist(), list(g), X)
            take = settle = False
            if dx is not None:
                predicted = g.dot(dx) - dx.dot(H.dot(dx)) / 2
                if predicted >= 0:
                    trial = p + dx
                    trial_cost = _error(cams, Z, trial, noise, X)
                    cost_change = cost - trial_cost
                    if predicted > X.eps * f0:
                        ratio = cost_change / predicted
                        dec.append(("gain_ratio", ratio, 1e-3, 1))
                        take = ratio > 1e-3
                    dec.append(("relative_change", abs(cost_change), 1e-5 * cost, cost))
                    settle = abs(cost_change) < 1e-5 * cost
            if take:
                lam = lam / factor
                p, cost = trial, trial_cost
                iterations += 1
                trials += 1
                break
            if settle:
                break
            lam = lam * factor
            trials += 1
            dec.append(("lambda", lam, 1e5, 1e5))
            if lam >= 1e5:
                break
        new_error = cost
        if iterations >= 100:
            break
        # checkConvergence
        if new_error <= 0:
            break
        dec.append(("absolute_decrease", current_error - new_error, 1.0, 1.0))
        dec.append(("relative_decrease", (current_error - new_error) / current_error, 1e-5, 1e-5))
        if (current_error - new_error) / current_error <= 1e-5 or current_error - new_error <= 1.0:
            break
    return p, iterations, trials


def _colpiv_qr_solve(Ab, rank_tol, X, dec):
    """ColPivHouseholderQR of the 2m x 3 system with setThreshold(rank_tol): (status, x, |pivots|)"""
    M = np.array(Ab, dtype=object)
    rows = M.shape[0]
    perm = [0, 1, 2]
    piv = []
    for k in range(3):
        norms = [sum(M[i, j] * M[i, j] for i in range(k, rows)) for j in range(k, 3)]
        jmax = k + max(range(len(norms)), key=lambda j: (norms[j], -j))
        if jmax != k:
            M[:, [k, jmax]] = M[:, [jmax, k]]
            perm[k], perm[jmax] = perm[jmax], perm[k]
        x = M[k:, k].copy()
        nrm = X.sqrt(sum(v * v for v in x))
        if nrm == 0:
            piv.append(X.num(0))
            continue
        alpha = -nrm if x[0] >= 0 else nrm
        v = x.copy()
        v[0] = v[0] - alpha
        vv = sum(a * a for a in v)
        if vv != 0:
            for j in range(k, 4):
                f = 2 * sum(v[i] * M[k + i, j] for i in range(len(v))) / vv
                for i in range(len(v)):
                    M[k + i, j] = M[k + i, j] - f * v[i]
        piv.append(abs(M[k, k]))
    pmax = max(piv)
    for pv in piv:
        dec.append(("pivot_ratio", pv, rank_tol * pmax, pmax))
    if sum(1 for pv in piv if pv > rank_tol * pmax) < 3:
        return DEGENERATE, None, piv
    y = [X.num(0)] * 3
    for i in (2, 1, 0):
        y[i] = (M[i, 3] - sum(M[i, j] * y[j] for j in range(i + 1, 3))) / M[i, i]
    x = [X.num(0)] * 3
    for i in range(3):
        x[perm[i]] = y[i]
    return VALID, np.array(x, dtype=object), piv


def _cross_norm(a, b, X):
    c = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    return X.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])


def triangulate(cameras, measurements, params: Params, X=FLOAT, sensors=None) -> Result:
    """triangulatePoint3 (params.safe False) / triangulateSafe (True) on one track"""
    n = X.num
    nan = np.full(3, np.nan)
    dec = []
    m = len(cameras)
    if m < 2:
        return Result(DEGENERATE, nan, decisions=dec)
    cams = [_Cam(c, X, None if sensors is None else sensors[i]) for i, c in enumerate(cameras)]
    Z = [np.array([n(z[0]), n(z[1])], dtype=object) for z in measurements]
    res = Result(VALID, nan, decisions=dec)
    if params.use_lost:
        sigma = n(lost_sigma(params.noise))
        zc = []
        for cam, z in zip(cams, Z):
            pn = cam.calibrate(z)
            if pn is None:
                res.status = CALIBRATION_FAILED
                return res
            zc.append(np.array([pn[0], pn[1], n(1)], dtype=object))
        rows = []
        for i in range(m):
            wZi = cams[i].R.dot(zc[i])
            ok = False
            for k in range(1, m):
                j = (i + k) % m
                d_ij = cams[j].t - cams[i].t
                wZj = cams[j].R.dot(zc[j])
                num, den = _cross_norm(wZi, wZj, X), _cross_norm(d_ij, wZj, X)
                if (not (num == 0 or den == 0)) if k == 1 else (num > 0 and den > 0):
                    ok = True
                    break
            if not ok:
                res.status = DEGENERATE
                return res
            q = num / (sigma * den)
            S = np.array([[n(0), n(-1), zc[i][1]], [n(1), n(0), -zc[i][0]]], dtype=object)
            C = q * S.dot(cams[i].R.T)
            b = C.dot(cams[i].t)
            rows.append(list(C[0]) + [b[0]])
            rows.append(list(C[1]) + [b[1]])
        res.A = np.array(rows, dtype=object)
        st, x, piv = _colpiv_qr_solve(rows, n(params.rank_tol), X, dec)
        res.sigma = piv
        if st != VALID:
            res.status = st
            return res
        point = x
    else:
        rows = []
        for cam, z in zip(cams, Z):
            u, v = z
            if cam.distorted:
                pn = cam.calibrate(z)
                if pn is None:
                    res.status = CALIBRATION_FAILED
                    return res
                u, v = cam.fx * pn[0] + cam.s * pn[1] + cam.u0, cam.fy * pn[1] + cam.v0
            P = cam.projection_matrix()
            rows.append(list(u * P[2] - P[0]))
            rows.append(list(v * P[2] - P[1]))
        res.A = np.array(rows, dtype=object)
        s, V = X.svd(rows)
        res.sigma = s
        for sv in s:
            dec.append(("singular_value", sv, params.rank_tol, s[0]))
        if sum(1 for sv in s if sv > params.rank_tol) < 3:
            res.status = DEGENERATE
            return res
        v = V[:, 3]
        if v[3] == 0:
            res.status = DEGENERATE
            return res
        point = np.array([v[0] / v[3], v[1] / v[3], v[2] / v[3]], dtype=object)
    res.linear_point = np.array([float(x) for x in point]) if X is FLOAT else point.copy()
    if params.optimize:
        point, res.iterations, res.trials = _refine(cams, Z, point, params.noise, X, dec)
    for cam in cams:
        z = cam.to_camera(point)[2]
        dec.append(("depth", z, 0, X.sqrt(sum(a * a for a in (point - cam.t)))))
        if z <= 0:
            res.status = BEHIND_CAMERA
            return res
    if params.safe:
        max_reproj = n(0)
        for cam, z in zip(cams, Z):
            if params.landmark_distance_threshold > 0:
                dist = X.sqrt(sum(a * a for a in (point - cam.t)))
                dec.append(("distance", dist, params.landmark_distance_threshold, params.landmark_distance_threshold))
                if dist > params.landmark_distance_threshold:
                    res.status = FAR_POINT
                    return res
            if params.outlier_threshold > 0:
                e = cam.project(point) - z
                max_reproj = max(max_reproj, X.sqrt(e[0] * e[0] + e[1] * e[1]))
        if params.outlier_threshold > 0:
            dec.append(("reprojection", max_reproj, params.outlier_threshold, params.outlier_threshold))
            if max_reproj > params.outlier_threshold:
                res.status = OUTLIER
                return res
    res.point = np.array([float(x) for x in point]) if X is FLOAT else point
    return res


def well_separated(decisions, rel=1e-6) -> bool:
    """no decision quantity within a relative `rel` of its threshold"""
    for _, value, thr, scale in decisions:
        ref = max(abs(value), abs(thr)) if thr != 0 else abs(scale)
        if abs(value - thr) <= rel * ref:
            return False
    return True


def group_tracks(arrays):
    """the grouping of gsx_triangulation_tracks on ProblemArrays: (landmark_vars, track_ptr, obs_factor)"""
    per = {}
    for f in range(arrays.n_factors):
        if arrays.f_type[f] in (3, 4):
            per.setdefault(int(arrays.f_vars[arrays.f_key_ptr[f] + 1]), []).append(f)
    lm = sorted(per)
    ptr = np.cumsum([0] + [len(per[v]) for v in lm])
    return lm, ptr, [f for v in lm for f in per[v]]
