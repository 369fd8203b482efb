"""The yardstick of the PCG tests: preconditionedConjugateGradient (gtsam/linear/ConjugateGradientSolver.h:109-171) with
BlockJacobiPreconditioner (gtsam/linear/Preconditioner.cpp:87-176) and DummyPreconditioner, restated literally — once in
numpy float64 and once in 50-digit mpmath — on the dense A, b formed from gsx_get_jacobians output:

    system  A = J'J + lambda D,  b = J'rhs,  x0 = 0,  D = 1 or clamp(diag J'J, min, max)
    loop    for (k = 1; k <= maxIterations && (gamma > threshold || k <= minIterations); k++),
            threshold = max(epsilon_abs, epsilon_rel^2 gamma_0), restart from the true residual at k % reset == 0

Both return a PcgRun: x, the number of loop bodies executed (`k`: gamma_trace[k] is the gamma the loop ended on; the
reference's own counter stands at k + 1 then), the gamma trace (gamma_trace[0] = gamma_0), the threshold and the TRUE
(b - A x)' M^-1 (b - A x) of the returned x.  Nothing here knows the device; the cases the host and GPU tests share are at
the bottom.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from gtsam_petercdev_amd import _abi as A

DUMMY, BLOCK_JACOBI = A.PRECOND_DUMMY, A.PRECOND_BLOCK_JACOBI
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@dataclass
class Params:
    """ConjugateGradientParameters() — ConjugateGradientSolver.h:45-51."""
    max_iterations: int = 500
    min_iterations: int = 1
    reset: int = 501
    epsilon_rel: float = 1e-3
    epsilon_abs: float = 1e-3
    preconditioner: int = BLOCK_JACOBI

    def c_params(self) -> A.PCGParams:
        return A.PCGParams(self.max_iterations, self.min_iterations, self.reset, self.epsilon_rel, self.epsilon_abs,
                           self.preconditioner)


@dataclass
class PcgRun:
    x: np.ndarray
    k: int
    gamma_trace: List[float]
    threshold: float
    true_gamma: float
    blocks: Optional[list] = None     # the L_v of the block-Jacobi build (float64 run only)

    @property
    def gamma_initial(self):
        return self.gamma_trace[0]

    @property
    def gamma_final(self):
        return self.gamma_trace[-1]


# ---- the dense system ------------------------------------------------------------------------------------------------
def dense_system(arr: A.ProblemArrays, jac: np.ndarray):
    """(J [M x N], rhs [M]) from the [A b] blocks (graph order, each m x (sum d + 1) column-major)."""
    toff = arr.tangent_offsets()
    joff = arr.jacobian_offsets()
    M, N = int(arr.f_rows.sum()), int(toff[-1])
    J, rhs = np.zeros((M, N)), np.zeros(M)
    r0 = 0
    for f in range(arr.n_factors):
        m = int(arr.f_rows[f])
        vs = arr.f_vars[arr.f_key_ptr[f]:arr.f_key_ptr[f + 1]]
        cols = int(sum(arr.var_dims[v] for v in vs)) + 1
        blk = jac[joff[f]:joff[f] + m * cols].reshape(cols, m).T
        c = 0
        for v in vs:
            d = int(arr.var_dims[v])
            J[r0:r0 + m, toff[v]:toff[v] + d] += blk[:, c:c + d]
            c += d
        rhs[r0:r0 + m] = blk[:, c]
        r0 += m
    return J, rhs


def damping_vector(J, diagonal, min_diagonal=1e-6, max_diagonal=1e32):
    """LevenbergMarquardtState::buildDampedSystem's weights: 1, or clamp(diag J'J) (LevenbergMarquardtOptimizer.cpp:293-299)."""
    if not diagonal:
        return np.ones(J.shape[1])
    return np.minimum(np.maximum((J * J).sum(axis=0), min_diagonal), max_diagonal)


# ---- float64 ----------------------------------------------------------------------------------------------------------
def block_cholesky(H):
    """L = chol(H, lower), column by column as Eigen's unblocked llt (the upper triangle of the result is zero);
    None when a pivot is not positive."""
    d = H.shape[0]
    L = np.zeros((d, d))
    for j in range(d):
        s = H[j, j] - np.dot(L[j, :j], L[j, :j])
        if not (s > 0.0) or not np.isfinite(s):
            return None
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, d):
            L[i, j] = (H[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    return L


def build_blocks(J, dims, lam, D):
    """BlockJacobiPreconditioner::build on the damped graph: per variable chol(J_v'J_v + lambda D_v)."""
    out, o = [], 0
    for d in dims:
        Jv = J[:, o:o + d]
        out.append(block_cholesky(Jv.T @ Jv + lam * np.diag(D[o:o + d])))
        o += d
    return out


def _left(blocks, dims, v):      # L^-1 v
    if blocks is None:
        return v.copy()
    out, o = np.empty_like(v), 0
    for L, d in zip(blocks, dims):
        for i in range(d):
            out[o + i] = (v[o + i] - np.dot(L[i, :i], out[o:o + i])) / L[i, i]
        o += d
    return out


def _right(blocks, dims, v):     # L^-T v
    if blocks is None:
        return v.copy()
    out, o = np.empty_like(v), 0
    for L, d in zip(blocks, dims):
        for i in range(d - 1, -1, -1):
            out[o + i] = (v[o + i] - np.dot(L[i + 1:, i], out[o + i + 1:o + d])) / L[i, i]
        o += d
    return out


class IndeterminateBlock(Exception):
    def __init__(self, var):
        super().__init__(f"the diagonal block of variable {var} has no Cholesky factor")
        self.var = var


def pcg_float64(J, rhs, dims, lam, D, prm: Params) -> PcgRun:
    dims = [int(d) for d in dims]
    blocks = None
    if prm.preconditioner == BLOCK_JACOBI:
        blocks = build_blocks(J, dims, lam, D)
        for v, L in enumerate(blocks):
            if L is None:
                raise IndeterminateBlock(v)
    mul = lambda v: J.T @ (J @ v) + lam * D * v
    b = J.T @ rhs
    with np.errstate(all="ignore"):
        x = np.zeros(J.shape[1])
        q1 = b - mul(x)
        r = _left(blocks, dims, q1)
        p = _right(blocks, dims, r)
        gamma = float(np.dot(r, r))
        threshold = max(prm.epsilon_abs, prm.epsilon_rel * prm.epsilon_rel * gamma)
        trace = [gamma]
        k = 1
        while k <= prm.max_iterations and (gamma > threshold or k <= prm.min_iterations):
            if k % prm.reset == 0:
                q1 = b - mul(x)
                r = _left(blocks, dims, q1)
                p = _right(blocks, dims, r)
                gamma = float(np.dot(r, r))
            q1 = mul(p)
            alpha = np.float64(gamma) / np.float64(np.dot(p, q1))
            x = x + alpha * p
            q2 = _left(blocks, dims, q1)
            r = r + (-alpha) * q2
            prev = gamma
            gamma = float(np.dot(r, r))
            beta = np.float64(gamma) / np.float64(prev)
            q1 = _right(blocks, dims, r)
            p = beta * p + q1
            trace.append(gamma)
            k += 1
        t = _left(blocks, dims, b - mul(x))
        return PcgRun(x, k - 1, trace, threshold, float(np.dot(t, t)), blocks)


def true_gamma(J, rhs, dims, lam, D, precond, x):
    """(b - A x)' M^-1 (b - A x) of any x, in float64."""
    dims = [int(d) for d in dims]
    blocks = build_blocks(J, dims, lam, D) if precond == BLOCK_JACOBI else None
    t = _left(blocks, dims, J.T @ rhs - (J.T @ (J @ x) + lam * D * x))
    return float(np.dot(t, t))


def a_norm(J, lam, D, v):
    """sqrt(v' (J'J + lambda D) v)."""
    Jv = J @ v
    return float(np.sqrt(np.dot(Jv, Jv) + lam * np.dot(D * v, v)))


# ---- 50 digits ---------------------------------------------------------------------------------------------------------
def pcg_mp(J, rhs, dims, lam, D, prm: Params, digits=50) -> PcgRun:
    """The same loop in mpmath, on the float64 entries of J, rhs and D taken as exact (sparse rows: J is mostly zero)."""
    import mpmath as mp
    old = mp.mp.dps
    mp.mp.dps = digits
    try:
        f = mp.mpf
        dims = [int(d) for d in dims]
        N = J.shape[1]
        rows = [[(int(j), f(float(J[i, j]))) for j in np.nonzero(J[i])[0]] for i in range(J.shape[0])]
        rh = [f(float(v)) for v in rhs]
        Dm = [f(float(v)) for v in D]
        lm = f(float(lam))
        zero = f(0)

        def mul(v):
            q = [lm * Dm[j] * v[j] for j in range(N)]
            for row in rows:
                y = sum((a * v[j] for j, a in row), zero)
                for j, a in row:
                    q[j] += a * y
            return q

        b = [zero] * N
        for row, y in zip(rows, rh):
            for j, a in row:
                b[j] += a * y
        blocks = None
        if prm.preconditioner == BLOCK_JACOBI:
            blocks, o = [], 0
            for d in dims:
                H = [[zero] * d for _ in range(d)]
                for row in rows:
                    ent = [(j - o, a) for j, a in row if o <= j < o + d]
                    for i, ai in ent:
                        for j, aj in ent:
                            H[i][j] += ai * aj
                for i in range(d):
                    H[i][i] += lm * Dm[o + i]
                L = [[zero] * d for _ in range(d)]
                for j in range(d):
                    s = H[j][j] - sum((L[j][c] * L[j][c] for c in range(j)), zero)
                    if not s > 0:
                        raise IndeterminateBlock(len(blocks))
                    L[j][j] = mp.sqrt(s)
                    for i in range(j + 1, d):
                        L[i][j] = (H[i][j] - sum((L[i][c] * L[j][c] for c in range(j)), zero)) / L[j][j]
                blocks.append(L)
                o += d

        def left(v):
            if blocks is None:
                return list(v)
            out, o = list(v), 0
            for L, d in zip(blocks, dims):
                for i in range(d):
                    out[o + i] = (v[o + i] - sum((L[i][c] * out[o + c] for c in range(i)), zero)) / L[i][i]
                o += d
            return out

        def right(v):
            if blocks is None:
                return list(v)
            out, o = list(v), 0
            for L, d in zip(blocks, dims):
                for i in range(d - 1, -1, -1):
                    out[o + i] = (v[o + i] - sum((L[c][i] * out[o + c] for c in range(i + 1, d)), zero)) / L[i][i]
                o += d
            return out

        dot = lambda u, v: sum((s * t for s, t in zip(u, v)), zero)
        x = [zero] * N
        r = left(b)
        p = right(r)
        gamma = dot(r, r)
        threshold = max(f(prm.epsilon_abs), f(prm.epsilon_rel) * f(prm.epsilon_rel) * gamma)
        trace = [gamma]
        k = 1
        while k <= prm.max_iterations and (gamma > threshold or k <= prm.min_iterations):
            if k % prm.reset == 0:
                Ax = mul(x)
                r = left([bi - ai for bi, ai in zip(b, Ax)])
                p = right(r)
                gamma = dot(r, r)
            q1 = mul(p)
            alpha = gamma / dot(p, q1)
            x = [xi + alpha * pi for xi, pi in zip(x, p)]
            q2 = left(q1)
            r = [ri - alpha * qi for ri, qi in zip(r, q2)]
            prev = gamma
            gamma = dot(r, r)
            beta = gamma / prev
            q1 = right(r)
            p = [beta * pi + qi for pi, qi in zip(p, q1)]
            trace.append(gamma)
            k += 1
        Ax = mul(x)
        t = left([bi - ai for bi, ai in zip(b, Ax)])
        return PcgRun(np.array([float(v) for v in x]), k - 1, [float(g) for g in trace], float(threshold), float(dot(t, t)))
    finally:
        mp.mp.dps = old


# ---- a stop that is not a coin toss -----------------------------------------------------------------------------------
def pick_epsilon(J, rhs, dims, lam, D, prm: Params, want=lambda k: k >= 1, horizon=400):
    """epsilon_rel (with epsilon_abs = 0) for which the float64 restatement stops at an iteration k with want(k), gamma
    before it at least 2x the threshold and gamma at it at most 1/2 of it — chosen from one long run of the restatement
    alone.  Returns (epsilon_rel, k); None when the gamma trace has no such drop."""
    long = Params(horizon, 0, prm.reset, 1e-14, 0.0, prm.preconditioner)
    tr = pcg_float64(J, rhs, dims, lam, D, long).gamma_trace
    g0 = tr[0]
    if not g0 > 0:
        return None
    low = g0
    for k in range(1, len(tr)):
        if want(k) and tr[k] > 1e-20 * g0 and low / tr[k] >= 4.5 and np.isfinite(tr[k]):   # (not a gamma at rounding level)
            thr = np.sqrt(low * tr[k])
            return float(np.sqrt(thr / g0)), k
        low = min(low, tr[k])
    return None


def stop_is_decisive(run: PcgRun) -> bool:
    """gamma at iteration k - 1 at least twice the threshold, gamma at k at most half of it."""
    return run.k >= 1 and run.gamma_trace[run.k - 1] >= 2 * run.threshold and run.gamma_trace[run.k] <= 0.5 * run.threshold


# ---- the cases --------------------------------------------------------------------------------------------------------
LAMBDAS = (0.0, 1e-3, 10.0)


def _golden(name):
    from gtsam_petercdev_amd import _lib
    path = os.path.join(GOLDEN, name)
    if name.startswith("dubrovnik"):
        return _lib.read_bal(path, priors=True)
    return _lib.read_g2o(path, is3D=name.startswith("pose3"))


def _star(n_landmarks=130, seed=7):
    """One Pose3 seeing n landmarks through GenericProjectionFactor, a prior on every landmark and on the pose: the pose's
    term list is n + 1 long (more than two waves), beside n lists of length 2."""
    import gtsam_petercdev_amd as gt
    rng = np.random.default_rng(seed)
    g, v = gt.NonlinearFactorGraph(), gt.Values()
    K = gt.Cal3_S2(500.0, 500.0, 0.0, 320.0, 240.0)
    pose = gt.Pose3(gt.Rot3.Rodrigues(0.02, -0.01, 0.03), np.array([0.1, -0.2, 0.05]))
    v.insert(gt.X(0), pose)
    g.add(gt.PriorFactor(gt.X(0), pose, gt.noiseModel.Isotropic.Sigma(6, 0.1)))
    pix = gt.noiseModel.Isotropic.Sigma(2, 1.0)
    for j in range(n_landmarks):
        pt = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(4, 9)])
        v.insert(gt.L(j), gt.Point3(*pt))
        g.add(gt.GenericProjectionFactor(rng.uniform(0, 640, 2), pix, gt.X(0), gt.L(j), K))
        g.add(gt.PriorFactor(gt.L(j), gt.Point3(*(pt + rng.normal(0, 0.05, 3))), gt.noiseModel.Isotropic.Sigma(3, 0.5)))
    return g.to_arrays(v)


def _linear5(seed=11):
    """A GSX_F_LINEAR factor over 5 keys, a VECTOR(1) and a VECTOR(7) among them, a unary factor on every variable (one
    variable has ONLY its unary factor: the shortest term list); total tangent size 1 + 7 + 2 + 3 + 4 + 5 = 22."""
    import gtsam_petercdev_amd as gt
    rng = np.random.default_rng(seed)
    dims = [1, 7, 2, 3, 4, 5]
    g = gt.GaussianFactorGraph()
    args = []
    for k, d in enumerate(dims[:5]):
        args += [k, rng.normal(size=(6, d))]
    g.add(gt.JacobianFactor(*args, rng.normal(size=6)))
    for k, d in enumerate(dims):
        g.add(gt.JacobianFactor(k, np.eye(d) * rng.uniform(0.5, 2.0) + 0.1 * rng.normal(size=(d, d)), rng.normal(size=d)))
    arr = g.to_arrays(None)
    arr.values = np.zeros(int(arr.var_dims.sum()))
    return arr


def _huber():
    """pose3example with a Huber between factor added whose residual lies beyond k (reweighted rows)."""
    import gtsam_petercdev_amd as gt
    arr = _golden("pose3example.txt")
    base = gt.noiseModel.Diagonal.Sigmas([0.1, 0.1, 0.1, 0.3, 0.3, 0.3])
    rob = gt.noiseModel.Robust.Create(gt.noiseModel.mEstimator.Huber.Create(1.345), base)
    meas = gt.Pose3(gt.Rot3.Rodrigues(0.3, -0.2, 0.4), np.array([2.5, 1.5, 0.7]))
    return arr.with_factor(A.F_BETWEEN, [0, 3], 6, meas.state(), rob.kind, rob.params)


def _selfcal():
    """Three poses on a circle looking at eight points and one Cal3_S2 (VECTOR(5)) under three-key GeneralSFMFactor2
    (examples/SelfCalibrationExample.cpp); every point lies in front of every camera."""
    from tests import _sensor_restatement as S
    return S.selfcal_graph(3, 8, seed=5)


def host_jacobian_system(arr, oracle):
    """(J, rhs) at the case's values without a device: the oracle's [A b]; GSX_F_SFM2, which the oracle does not know, from
    the numpy restatement of the sensor factors."""
    if np.any(arr.f_type == A.F_SFM2):
        from tests import _sensor_restatement as S
        return S.dense_system(arr, arr.values)
    ob = oracle.oracle_backend(arr)
    ob.linearize()
    return dense_system(arr, ob.jacobians())


CASES = {
    "pose2example": lambda: _golden("pose2example.txt"),
    "pose3example": lambda: _golden("pose3example.txt"),
    "dubrovnik-3-7": lambda: _golden("dubrovnik-3-7-pre.txt"),
    "selfcal": _selfcal,
    "linear5": _linear5,
    "star130": _star,
    "huber": _huber,
}
# (preconditioner, diagonal damping, lambda) of every case; lambda = 0 needs a positive definite J'J, which every case has
# (each carries priors)
CONFIGS = [(pc, dg, lam) for pc in (BLOCK_JACOBI, DUMMY) for dg in (0, 1) for lam in LAMBDAS]
