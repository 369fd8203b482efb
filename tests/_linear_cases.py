"""Seeded problems for the backward-error tests (test_host_linear_judge.py judges the CPU oracle on them,
test_gpu_linear_bounds.py the device): the smallest shapes that still reach each elimination / solve / marginal kernel."""
import numpy as np

from gtsam_petercdev_amd import datasets
from gtsam_petercdev_amd.graph import GaussianFactorGraph, JacobianFactor, noiseModel

# (dim A, dim B) of the two-clique tree (A | B) <- (B, c): frontal width of the child over the kernels' size classes
LADDER_A = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 230]
LADDER_B = [12, 60, 131]
LADDER = [(a, b) for b in LADDER_B for a in LADDER_A] + [(385, 12)]     # + one front of three 192-column chunks
LEAF_HEIGHTS = [(a, b) for a in (1, 3, 6, 16) for b in (63, 64, 65, 69, 72, 73, 127, 128, 129, 139, 140)]
MEDIUM = [(a, 131) for a in (15, 17, 33, 64, 65, 127)]
MARGINAL_POINTS = [(16, 12), (17, 60), (65, 131), (193, 60), (230, 131)]
LAMBDAS = [(0.0, False), (0.1, True), (1e-3, False)]


def _split_dims(total, rng):
    out = []
    while total > 0:
        d = int(min(total, rng.integers(1, 9)))
        out.append(d)
        total -= d
    return out


def two_clique_arrays(dim_a, dim_b):
    """test_gpu_parity.py::_two_clique_case's graph (same seed, same draws): variables of 1-8 dimensions, A and B mutually
    adjacent through two-row factors, one last variable c hanging on B.  Returns (arrays, natural ordering, #A, #B)."""
    rng = np.random.default_rng(dim_a * 1000 + dim_b)
    da, db = _split_dims(dim_a, rng), _split_dims(dim_b, rng)
    dims = da + db + [3]
    nv = len(dims)
    fg = GaussianFactorGraph()
    for k, d in enumerate(dims):
        fg.add(JacobianFactor(k, np.eye(d) * (0.7 + rng.random()), rng.normal(size=d), noiseModel.Isotropic.Sigma(d, 1.5)))
    nab = len(da) + len(db)
    for a in range(nab):
        for b in range(a + 1, nab):
            fg.add(JacobianFactor(a, rng.normal(0, 0.3, (2, dims[a])), b, rng.normal(0, 0.3, (2, dims[b])), rng.normal(size=2),
                                  noiseModel.Isotropic.Sigma(2, 1.0)))
    kb, kc = len(da), nv - 1
    fg.add(JacobianFactor(kb, rng.normal(0, 0.4, (3, dims[kb])), kc, rng.normal(0, 0.4, (3, 3)), rng.normal(size=3),
                          noiseModel.Isotropic.Sigma(3, 0.5)))
    arr = fg.to_arrays(None)
    arr.values = np.zeros(int(arr.var_dims.sum()))
    return arr, list(range(nv)), len(da), len(db)


RANDOM_SEEDS = range(6)


def random_linear_arrays(seed):
    """The generator of test_gpu_parity.py::test_random_linear_graphs (a chain with random chords, two hubs, a dense cluster
    on every third seed) with variables of 1 to 40 dimensions, sized for a dense longdouble judge (at most ~400 scalars)."""
    rng = np.random.default_rng(7000 + seed)
    nv = [9, 30, 70, 20, 30, 80][seed]
    ds = ([1, 2, 3], [2, 6, 9], [1, 5, 9], [1, 5, 17, 40], [9, 3, 24], [3, 6])[seed]
    dims = [int(d) for d in rng.choice(ds, size=nv)]
    fg = GaussianFactorGraph()
    for k, d in enumerate(dims):
        fg.add(JacobianFactor(k, np.eye(d) * (0.5 + rng.random()), rng.normal(size=d), noiseModel.Isotropic.Sigma(d, 2.0)))
    pairs = {(k, k + 1) for k in range(nv - 1)}
    for a, b in rng.integers(0, nv, (int(nv * rng.choice([0.2, 1.0, 2.5])), 2)):
        if a != b:
            pairs.add((int(min(a, b)), int(max(a, b))))
    for hub in rng.integers(0, nv, 2):
        for b in rng.choice(nv, size=min(nv - 1, int(rng.choice([5, 22, 40]))), replace=False):
            if int(b) != int(hub):
                pairs.add((int(min(hub, b)), int(max(hub, b))))
    if nv >= 30 and seed % 3 == 0:
        c0 = int(rng.integers(0, nv - 20))
        pairs |= {(a, b) for a in range(c0, c0 + 18) for b in range(a + 1, c0 + 18)}
    for a, b in sorted(pairs):
        m = int(rng.integers(1, 1 + min(dims[a] + dims[b], 6)))
        fg.add(JacobianFactor(a, rng.normal(0, 0.4, (m, dims[a])), b, rng.normal(0, 0.4, (m, dims[b])), rng.normal(size=m),
                              noiseModel.Diagonal.Sigmas(0.5 + rng.random(m))))
    arr = fg.to_arrays(None)
    arr.values = np.zeros(int(arr.var_dims.sum()))
    return arr


def bal_arrays(n_cams):
    """Bundle adjustment, 150 landmarks: 7 cameras (stored complements, fused star leaves) or 30 (product-form / lean)."""
    return datasets.synth_bal_arrays(n_cams, 150, 600 if n_cams == 7 else 1500, seed=21 + n_cams, long_range=0.3, priors=True)


def pose3_arrays():
    """A Pose3 chain of 60 poses with loop closures."""
    return datasets.synth_manhattan_pose3(60, seed=4)


TREE_AMALGAMATION = (0.5, 64)


def tree_arrays(name):
    """The two makers of test_gpu_parity.py::test_tree_kernels_against_the_level_launches at their small sizes: with
    TREE_AMALGAMATION under nested dissection every front is LDS-class and both tiers of the tree kernels occur."""
    return datasets.synth_manhattan_pose3(300, seed=4) if name == "pose3" else datasets.synth_manhattan_pose2(400, seed=3)
