"""Graphs shared by the lago tests: the reference's simpleLago::graph() (gtsam/slam/tests/testLago.cpp:39-66) and its
variants with more priors, the toy g2o graph with the tests' prior, the 2-D golden files, spirals whose chords wrap
several times, seeded Manhattan graphs with mixed noise kinds, random trees."""
import math
import os

import numpy as np

import gtsam_petercdev_amd as gt
from gtsam_petercdev_amd import _abi as A, _lib, datasets

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
X = [gt.symbol("x", j) for j in range(4)]
SIMPLE_POSES = [(0.0, 0.0, 0.0), (1.0, 1.0, 1.570796), (0.0, 2.0, 3.141593), (-1.0, 1.0, 4.712389)]
SIMPLE_THETA = [0.0, 0.5 * math.pi, math.pi, 1.5 * math.pi]


def between(a, b):
    """Pose2::between; the angle as Rot2 keeps it, atan2(sin, cos)."""
    c, s = math.cos(a[2]), math.sin(a[2])
    dx, dy, th = b[0] - a[0], b[1] - a[1], b[2] - a[2]
    return gt.Pose2(c * dx + s * dy, -s * dx + c * dy, math.atan2(math.sin(th), math.cos(th)))


def simple_graph(extra=None):
    """simpleLago::graph(); extra = "pose": + a prior on x1 (multiplePosePriors), "rot": + a prior on x1's orientation as a
    1-vector (multiplePoseAndRotPriors)."""
    model = gt.noiseModel.Isotropic.Sigma(3, 0.1)
    p = SIMPLE_POSES
    g = gt.NonlinearFactorGraph()
    for a, b in ((0, 1), (1, 2), (2, 3), (2, 0), (0, 3)):
        g.add(gt.BetweenFactor(X[a], X[b], between(p[a], p[b]), model))
    g.addPrior(X[0], gt.Pose2(*p[0]), model)
    if extra == "pose":
        g.addPrior(X[1], gt.Pose2(*p[1]), model)
    elif extra == "rot":
        g.add(gt.PriorFactor(X[1], np.array([p[1][2]]), gt.noiseModel.Isotropic.Sigma(1, 0.1)))
    return g


def simple_values(zero_theta=False):
    v = gt.Values()
    for k, p in zip(X, SIMPLE_POSES):
        v.insert(k, gt.Pose2(p[0], p[1], 0.0 if zero_theta else p[2]))
    return v


def simple_arrays(extra=None, zero_theta=False):
    g = simple_graph(extra)
    if extra == "rot":   # the lowering wants one type per key: the orientation prior sits on a key of its own
        g.factors[-1].keys_ = [gt.symbol("r", 1)]
        v = simple_values(zero_theta)
        v.insert(gt.symbol("r", 1), np.array([SIMPLE_POSES[1][2]]))
        return g.to_arrays(v)
    return g.to_arrays(simple_values(zero_theta))


def with_pose2_prior(arr, var, variances, pose=(0.0, 0.0, 0.0)):
    return arr.with_factor(A.F_PRIOR, [var], 3, pose, A.NOISE_DIAGONAL, np.sqrt(np.asarray(variances, dtype=float)))


def noisy_toy_arrays(variances=(1e-2, 1e-2, 1e-4)):
    """noisyToyGraph.txt with the prior of largeGraphNoisy (testLago.cpp:295-298) in place of the reader's."""
    arr = _lib.load2d(os.path.join(GOLDEN, "noisyToyGraph.txt"), noise_format=A.NOISE_FORMAT_G2O)   # readG2o
    return with_pose2_prior(arr, 0, variances)


def read_g2o_poses(name):
    """{key: (x, y, theta)} of the VERTEX_SE2 lines of a golden file."""
    out = {}
    for line in open(os.path.join(GOLDEN, name)):
        t = line.split()
        if t and t[0] == "VERTEX_SE2":
            out[int(t[1])] = np.array([float(t[2]), float(t[3]), float(t[4])])
    return out


def graph_file_arrays(name):
    """A 2-D "graph" golden file (w100.graph, example.graph) through load2D, with a prior on its first pose."""
    arr = _lib.load2d(os.path.join(GOLDEN, name))
    first = int(np.flatnonzero(arr.var_types == A.VAR_POSE2)[0])
    so = arr.state_offsets()
    return with_pose2_prior(arr, first, (1e-6, 1e-6, 1e-8), arr.values[so[first]:so[first] + 3])


def chain_arrays(keys, edges, priors, sigmas=(0.1, 0.1, 0.05), seed=0):
    """Pose2 variables `keys` (ascending), between factors `edges` = (i, j) index pairs with measurements from a seeded
    random truth, priors on the variables `priors`."""
    rng = np.random.default_rng(seed)
    n = len(keys)
    truth = np.stack([rng.normal(0, 3, n), rng.normal(0, 3, n), rng.uniform(-3, 3, n)], axis=1)
    nf = len(edges) + len(priors)
    f_type = [A.F_BETWEEN] * len(edges) + [A.F_PRIOR] * len(priors)
    key_ptr, fv, meas = [0], [], []
    for i, j in edges:
        fv += [i, j]
        key_ptr.append(len(fv))
        meas.append(between(truth[i], truth[j]).state())
    for i in priors:
        fv.append(i)
        key_ptr.append(len(fv))
        meas.append(truth[i])
    return A.ProblemArrays(
        var_keys=np.array(keys, np.uint64), var_types=np.full(n, A.VAR_POSE2), var_dims=np.full(n, 3), f_type=f_type,
        f_rows=np.full(nf, 3), f_key_ptr=key_ptr, f_vars=fv, f_meas_ptr=3 * np.arange(nf + 1),
        meas=np.concatenate(meas) if meas else np.zeros(0), f_noise_kind=np.full(nf, A.NOISE_DIAGONAL),
        f_noise_ptr=3 * np.arange(nf + 1), noise=np.tile(np.asarray(sigmas, dtype=float), nf), values=truth.reshape(-1))


def noncontiguous_arrays():
    """Keys 3 4 5 6 20 21 22: two odometric runs joined by non-consecutive edges (MST mode only: the odometric path has a
    gap at 20)."""
    return chain_arrays([3, 4, 5, 6, 20, 21, 22], [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 0), (2, 5)], [0])


def two_prior_arrays():
    return chain_arrays(list(range(6)), [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (1, 4)], [0, 3], seed=1)


def duplicate_edge_arrays():
    """A second factor between the consecutive keys 1 and 2, once in each direction."""
    return chain_arrays(list(range(5)), [(0, 1), (1, 2), (2, 1), (1, 2), (2, 3), (3, 4), (4, 0)], [0], seed=2)


def key_gap_arrays():
    return chain_arrays([0, 1, 2, 4, 5], [(0, 1), (1, 2), (2, 3), (3, 4)], [0], seed=3)


def no_prior_arrays():
    return chain_arrays(list(range(4)), [(0, 1), (1, 2), (2, 3), (3, 0)], [], seed=4)


def spiral_arrays(n, turn, closure_every, seed, sigma_theta=0.01):
    """A trajectory that keeps turning by about `turn` radians per step (signed), so that the cumulative orientation along
    the odometry passes 2 pi many times; loop closures every `closure_every` poses to poses far back: their k is
    the number of whole turns in between, positive or negative, well beyond 1."""
    rng = np.random.default_rng(seed)
    truth = np.zeros((n, 3))
    for i in range(1, n):
        th = truth[i - 1, 2] + turn
        truth[i] = (truth[i - 1, 0] + math.cos(th), truth[i - 1, 1] + math.sin(th), th)
    ei = list(range(n - 1))
    ej = list(range(1, n))
    for j in range(closure_every, n, closure_every):
        i = int(rng.integers(0, max(1, j - closure_every // 2)))
        if rng.random() < 0.5:
            ei.append(i), ej.append(j)
        else:
            ei.append(j), ej.append(i)
    ei, ej = np.array(ei), np.array(ej)
    z = np.stack([between(truth[a], truth[b]).state() for a, b in zip(ei, ej)])
    z[:, 2] += rng.normal(0, sigma_theta, ei.size)
    z[:, 2] = np.arctan2(np.sin(z[:, 2]), np.cos(z[:, 2]))
    init = truth.copy()
    init[:, 2] = np.arctan2(np.sin(init[:, 2]), np.cos(init[:, 2]))
    return datasets._pose_graph_arrays(A.VAR_POSE2, init, ei, ej, z, np.array([0.05, 0.05, sigma_theta]),
                                       np.sqrt([1e-6, 1e-6, 1e-8]))


SPIRALS = {"left": dict(n=300, turn=0.37, closure_every=7, seed=11), "right": dict(n=300, turn=-0.41, closure_every=5, seed=12),
           "tight": dict(n=700, turn=1.1, closure_every=9, seed=13)}


def mixed_noise(arr, seed):
    """The same graph with its between factors' Diagonal models replaced in turn by Unit, Isotropic, Diagonal and
    Constrained (positive sigmas) ones."""
    rng = np.random.default_rng(seed)
    kinds, ptr, noise = arr.f_noise_kind.copy(), [0], []
    for f in range(arr.n_factors):
        p = arr.noise[arr.f_noise_ptr[f]:arr.f_noise_ptr[f + 1]]
        if arr.f_type[f] == A.F_BETWEEN:
            which = f % 4
            if which == 0:
                kinds[f], p = A.NOISE_UNIT, np.zeros(0)
            elif which == 1:
                kinds[f], p = A.NOISE_ISOTROPIC, np.array([rng.uniform(0.02, 0.2)])
            elif which == 2:
                kinds[f], p = A.NOISE_DIAGONAL, rng.uniform(0.02, 0.2, 3)
            else:
                kinds[f], p = A.NOISE_CONSTRAINED, np.concatenate([rng.uniform(0.02, 0.2, 3), np.full(3, 1000.0)])
        noise.append(p)
        ptr.append(ptr[-1] + p.size)
    return A.ProblemArrays(arr.var_keys, arr.var_types, arr.var_dims, arr.f_type, arr.f_rows, arr.f_key_ptr, arr.f_vars,
                           arr.f_meas_ptr, arr.meas, kinds, ptr, np.concatenate(noise), arr.values.copy(), dict(arr.meta))


def manhattan_arrays(n, seed=5):
    """A Manhattan-world Pose2 graph (odometry chain, loop closures, prior on pose 0 last) with mixed noise kinds."""
    arr = mixed_noise(datasets.synth_manhattan_pose2(n, seed=seed, closure_prob=0.8), seed)
    assert arr.n_factors > n          # some loop closures
    return arr


def random_tree(n, seed, max_back=None):
    """parent[i] < i for i > 0 (node 0 the root), delta of a few radians."""
    rng = np.random.default_rng(seed)
    parent = np.zeros(n, np.int32)
    for i in range(1, n):
        lo = 0 if max_back is None else max(0, i - max_back)
        parent[i] = rng.integers(lo, i)
    delta = rng.uniform(-3.2, 3.2, n)
    return parent, delta
