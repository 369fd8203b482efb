"""Graphs shared by the InitializePose3 tests: the reference's simple::graph() / graph2()
(gtsam/slam/tests/testInitializePose3.cpp:36-89), its perturbed guess (:177-182), the g2o fixtures, seeded random graphs."""
import math
import os

import numpy as np

import gtsam_petercdev_amd as gt
from gtsam_petercdev_amd import _abi as A
from tests import _factor_restatement as FR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
X = [gt.symbol("x", j) for j in range(4)]
SIMPLE_R = [FR.so3_expmap(np.array([0.0, 0.0, th])) for th in (0.0, 1.570796, 3.141593, 4.712389)]
SIMPLE_P = [np.array(p, dtype=float) for p in ((0, 0, 0), (1, 2, 0), (0, 2, 0), (-1, 1, 0))]


def simple_poses():
    return [gt.Pose3(gt.Rot3(R), p) for R, p in zip(SIMPLE_R, SIMPLE_P)]


def simple_graph(second=False):
    """simple::graph(), or graph2() with its two zero-information loop closures."""
    pose = simple_poses()
    model = gt.noiseModel.Isotropic.Sigma(6, 0.1)
    g = gt.NonlinearFactorGraph()
    if not second:
        for a, b in ((0, 1), (1, 2), (2, 3), (2, 0), (0, 3)):
            g.add(gt.BetweenFactor(X[a], X[b], pose[a].between(pose[b]), model))
    else:
        one = gt.noiseModel.Isotropic.Precision(6, 1.0)
        zero = gt.noiseModel.Isotropic.Precision(6, 0.0)
        for a, b in ((0, 1), (1, 2), (2, 3)):
            g.add(gt.BetweenFactor(X[a], X[b], pose[a].between(pose[b]), one))
        g.add(gt.BetweenFactor(X[2], X[0], gt.Pose3(gt.Rot3.Ypr(0.1, 0.0, 0.1), [0.0, 0.0, 0.0]), zero))
        g.add(gt.BetweenFactor(X[0], X[3], gt.Pose3(gt.Rot3.Ypr(0.5, -0.2, 0.2), [10, 20, 30]), zero))
    g.addPrior(X[0], pose[0], model)
    return g


def simple_values(poses=None):
    v = gt.Values()
    for k, p in zip(X, poses or simple_poses()):
        v.insert(k, p)
    return v


def simple_arrays(second=False, poses=None):
    return simple_graph(second).to_arrays(simple_values(poses))


def perturbed_guess():
    """givenPoses of iterationGradient / orientationsGradient (:177-182)."""
    Rp = FR.so3_expmap(np.array([0.01, 0.01, 0.01]))
    p0 = simple_poses()[0]
    z = np.zeros(3)
    return [p0, p0.compose(gt.Pose3(gt.Rot3(Rp), z)), p0.compose(gt.Pose3(gt.Rot3(Rp.T), z)), p0.compose(gt.Pose3(gt.Rot3(Rp), z))]


ITERATION_GRADIENT = [np.array(m).reshape(3, 3) for m in (
    [0.999435813876064, -0.033571481675497, 0.001004768630281, 0.033572116359134, 0.999436104312325, -0.000621610948719,
     -0.000983333645009, 0.000654992453817, 0.999999302019670],
    [0.999905367545392, -0.010866391403031, 0.008436675399114, 0.010943459008004, 0.999898317528125, -0.009143047050380,
     -0.008336465609239, 0.009234508232789, 0.999922610604863],
    [0.998936644682875, 0.045376417678595, -0.008158469732553, -0.045306446926148, 0.998936408933058, 0.008566024448664,
     0.008538487960253, -0.008187284445083, 0.999930028850403],
    [0.999898767273093, -0.010834701971459, 0.009223038487275, 0.010911315499947, 0.999906044037258, -0.008297366559388,
     -0.009132272433995, 0.008397162077148, 0.999923041673329])]


def read_g2o_without_prior(name):
    """The 3-D g2o fixture `name` as the native reader lowers it, less the anchoring prior the reader appends last."""
    from gtsam_petercdev_amd import build, _lib
    build.build_lib()
    arr = _lib.read_g2o(os.path.join(GOLDEN, name), is3D=True)
    assert arr.f_type[-1] == A.F_PRIOR
    n = arr.n_factors - 1
    return A.ProblemArrays(
        arr.var_keys, arr.var_types, arr.var_dims, arr.f_type[:n], arr.f_rows[:n], arr.f_key_ptr[:n + 1],
        arr.f_vars[:arr.f_key_ptr[n]], arr.f_meas_ptr[:n + 1], arr.meas[:arr.f_meas_ptr[n]], arr.f_noise_kind[:n],
        arr.f_noise_ptr[:n + 1], arr.noise[:arr.f_noise_ptr[n]], arr.values.copy(), dict(arr.meta))


def gradient10_expected():
    """The rotations of the poses 1..4 of simpleGraph10gradIter.txt (orientationsGradient reads them with readG2o)."""
    arr = read_g2o_without_prior("simpleGraph10gradIter.txt")
    so = arr.state_offsets()
    idx = {int(k): i for i, k in enumerate(arr.var_keys)}
    return [arr.values[so[idx[k]]:so[idx[k]] + 9].reshape(3, 3) for k in (1, 2, 3, 4)]


GRADIENT10_TOL = [1e-4, 1e-4, 1e-3, 1e-4]


def grid_arrays():
    """pose3example-grid.txt + the Unit prior on pose 0 of initializePoses (:265-276); arr.values = the file's poses."""
    arr = read_g2o_without_prior("pose3example-grid.txt")
    i0 = int(np.searchsorted(arr.var_keys, np.uint64(0)))
    return arr.with_factor(A.F_PRIOR, [i0], 6, FR.pose3_state(np.eye(3), np.zeros(3)), A.NOISE_UNIT)


def random_pose_graph(n, seed, max_angle=None, min_span=2, loops=None):
    """A chain of n poses plus 3..10 loop closures; relative rotations with 0.05 rad noise; g2o-style full Gaussian, diagonal,
    isotropic and Huber-over-diagonal noise mixed; a prior on a pose that is not the first key; keys not contiguous.
    Returns (arrays with .values = the truth, truth rotations).  max_angle: upper bound on the relative rotation angles;
    min_span: least distance along the chain between the two poses of a loop closure; loops: their number (default: drawn)."""
    rng = np.random.default_rng(seed)
    keys = np.sort(rng.choice(np.arange(3, 20 * n), size=n, replace=False)).astype(np.int64)
    keys[n // 2:] += A.ANCHOR_KEY     # (some keys below the anchor's, some above)
    R, t = [FR.random_rot3(rng, 1.0)], [np.zeros(3)]
    for i in range(1, n):
        step = rng.normal(size=3)
        step *= rng.uniform(0.2, 1.0) / np.linalg.norm(step)
        R.append(R[-1] @ FR.so3_expmap(step))
        t.append(t[-1] + R[-2] @ rng.normal(size=3))
    edges = [(i, i + 1) for i in range(n - 1)]
    n_loops = min(int(rng.integers(3, 11)), (n - 1) * (n - 2) // 2 - 1)
    if loops is not None:
        n_loops = loops
    for _ in range(100000):
        if len(edges) == n - 1 + n_loops:
            break
        a, b = (int(x) for x in rng.choice(n, size=2, replace=False))
        if abs(a - b) < min_span or (a, b) in edges or (b, a) in edges:
            continue
        if max_angle is not None and np.linalg.norm(FR.so3_logmap(R[a].T @ R[b])) > max_angle - 0.3:
            continue
        edges.append((a, b))
    assert len(edges) >= n - 1 + 3
    values = gt.Values()
    for k, Ri, ti in zip(keys, R, t):
        values.insert(int(k), gt.Pose3(gt.Rot3(Ri), ti))
    g = gt.NonlinearFactorGraph()

    def noise(j):
        kind = j % 4
        if kind == 0:
            Lm = np.tril(rng.normal(size=(6, 6)) * 0.2) + np.diag(rng.uniform(2.0, 6.0, size=6))
            return gt.noiseModel.Gaussian.Information(Lm @ Lm.T)
        if kind == 1:
            return gt.noiseModel.Diagonal.Sigmas(rng.uniform(0.05, 0.3, size=6))
        if kind == 2:
            return gt.noiseModel.Isotropic.Sigma(6, float(rng.uniform(0.05, 0.3)))
        return gt.noiseModel.Robust.Create(gt.noiseModel.mEstimator.Huber.Create(1.345),
                                           gt.noiseModel.Diagonal.Sigmas(rng.uniform(0.05, 0.3, size=6)))
    for j, (a, b) in enumerate(edges):
        Rab = R[a].T @ R[b] @ FR.so3_expmap(0.05 * rng.normal(size=3) / math.sqrt(3.0))
        tab = R[a].T @ (t[b] - t[a]) + 0.05 * rng.normal(size=3)
        g.add(gt.BetweenFactor(int(keys[a]), int(keys[b]), gt.Pose3(gt.Rot3(Rab), tab), noise(j)))
    pk = 1 + int(rng.integers(0, n - 1))
    g.addPrior(int(keys[pk]), gt.Pose3(gt.Rot3(R[pk]), t[pk]), gt.noiseModel.Diagonal.Sigmas(rng.uniform(0.05, 0.2, size=6)))
    return g.to_arrays(values), R


def closest_rotation_cases(seed=11):
    """About 400 matrices whose closest rotation is unique with room to spare (sigma_2 + sigma_3 > 0.1 sigma_1 when the
    determinant is positive, sigma_2 - sigma_3 > 0.1 sigma_1 when negative; the tests assert 0.05 on 50-digit singular
    values): rotations plus noise of size 0, 1e-3, 0.3, the same scaled by 1e-3 and 1e3, the identity, a third singular
    value of 1e-9 with positive determinant, and matrices with det(U V') < 0."""
    rng = np.random.default_rng(seed)
    out = []

    def unique(M):
        s = np.linalg.svd(M, compute_uv=False)
        return (s[1] + s[2] > 0.1 * s[0]) if np.linalg.det(M) > 0 else (s[1] - s[2] > 0.1 * s[0])
    for noise in (0.0, 1e-3, 0.3):
        base = []
        while len(base) < 44:
            M = FR.random_rot3(rng, 3.0) + noise * rng.normal(size=(3, 3))
            if unique(M):
                base.append(M)
        for scale in (1.0, 1e-3, 1e3):
            out += [scale * M for M in base]
    out.append(np.eye(3))
    U, V = FR.random_rot3(rng, 3.0), FR.random_rot3(rng, 3.0)
    out.append(U @ np.diag([1.3, 0.7, 1e-9]) @ V.T)
    for _ in range(10):
        U, V = FR.random_rot3(rng, 3.0), FR.random_rot3(rng, 3.0)
        s = np.sort(rng.uniform(0.2, 2.0, size=3))[::-1]
        M = U @ np.diag([s[0], s[1], -s[2]]) @ V.T
        if unique(M):
            out.append(M)
    return np.stack(out)
