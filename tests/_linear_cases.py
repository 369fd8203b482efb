"""Seeded problems for the backward-error tests (test_host_linear_judge.py judges the CPU oracle on them,
test_gpu_linear_bounds.py the device): the smallest shapes that still reach each elimination / solve / marginal kernel."""
import os

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


# ---- deep and wide trees for the dependency-driven launches (front_tree / front_tree_med / backsolve_tree) ----------------------
# Natural ordering, the reference's cliques (amalgamation 0): the bottom clique of every arm or chain is a leaf-kernel
# front, everything above it a tree front.
DEEP_AMALGAMATION = (0.0, 128)


def _edge_graph(dims, edges, seed):
    """A unary factor per variable and a two-row factor per edge, as two_clique_arrays draws them; natural ordering."""
    rng = np.random.default_rng(seed)
    fg = GaussianFactorGraph()
    for k, d in enumerate(dims):
        fg.add(JacobianFactor(k, np.eye(d) * (0.7 + rng.random()), rng.normal(size=d), noiseModel.Isotropic.Sigma(d, 1.5)))
    for a, b in edges:
        fg.add(JacobianFactor(a, rng.normal(0, 0.3, (2, dims[a])), b, rng.normal(0, 0.3, (2, dims[b])), rng.normal(size=2),
                              noiseModel.Isotropic.Sigma(2, 1.0)))
    arr = fg.to_arrays(None)
    arr.values = np.zeros(int(arr.var_dims.sum()))
    return arr, list(range(len(dims)))


def chain(n, dim, band=1, tail_dim=None):
    """0 - 1 - ... - (n-1): cliques one on top of the other.  band = 2 also joins k and k + 2: still a chain of cliques, each
    with two separator variables (3 dim + 1 rows: variables have at most 64 dimensions, so a chain of single-variable
    cliques stops at 129 rows, below the medium class).  tail_dim: the dimension of the last `band` variables, which keeps
    the root clique (band + 1 variables, all frontal) out of the blocked class."""
    dims = [dim] * n if tail_dim is None else [dim] * (n - band) + [tail_dim] * band
    return _edge_graph(dims, [(k, k + b) for k in range(n - 1) for b in range(1, band + 1) if k + b < n],
                       9100 + 7 * n + dim + 1000 * (band - 1))


def broom(arms, length, hub_dim, dim=3):
    """`arms` chains of `length` variables (free end first), each ending on one hub variable, which comes last: the root
    clique (the hub with the top of the last arm) has `arms` children."""
    hub = arms * length
    edges = []
    for a in range(arms):
        edges += [(a * length + k, a * length + k + 1) for k in range(length - 1)] + [(a * length + length - 1, hub)]
    return _edge_graph([dim] * hub + [hub_dim], edges, 9200 + 11 * arms + length)


def caterpillar(n, dim=3):
    """A spine of n variables, each carrying an arm of two; all arms come first in the ordering, then the spine: a chain
    n deep whose every clique has two children."""
    edges = []
    for k in range(n):
        edges += [(2 * k, 2 * k + 1), (2 * k + 1, 2 * n + k)]
    edges += [(2 * n + k, 2 * n + k + 1) for k in range(n - 1)]
    return _edge_graph([dim] * (3 * n), edges, 9300 + n)


def forest(chains, dim):
    """`chains` separate chains of three variables: as many roots."""
    edges = []
    for c in range(chains):
        edges += [(3 * c, 3 * c + 1), (3 * c + 1, 3 * c + 2)]
    return _edge_graph([dim] * (3 * chains), edges, 9400 + chains + dim)


def colamd_pose2():
    """tree_arrays("pose2") under the reference's COLAMD ordering (tests/golden/make_colamd_orderings.py): the chain-like
    tree the reference itself eliminates.  Returns (arrays, ordering)."""
    arr = datasets.synth_manhattan_pose2(400, seed=3)
    perm = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colamd_perm_pose2_400_seed3.npy"))
    assert np.array_equal(np.sort(perm), np.arange(arr.n_vars))
    return arr, arr.var_keys[perm]


# tiers of the tree kernels (symbolic.cpp, without GSX_TREE_TIERS): subtrees of at most 67 rows, of at most 140, and the
# medium tier
TIER_BOUNDS = (67, 140)


def tree_shape(arr, ordering, amalgamation=DEEP_AMALGAMATION):
    """Host only: what the symbolic analysis makes of (arrays, ordering) — the figures the deep and wide cases are aimed
    at.  Tree children / height / roots / tickets follow the tables of the top-down launch that upload_symbolic (upload.hip) builds (a tree front's tree
    children whatever their tier; tickets = roots + sum of max(children - 1, 0)); start fronts follow symbolic.cpp (no
    unfinished child in the front's own tier), with the tier restated from the largest front of the tree subtree."""
    from gtsam_petercdev_amd import _lib
    hb = _lib.ProductBackend(arr, host_only=True)
    hb.set_amalgamation(*amalgamation)
    hb.set_ordering(ordering)
    parent, fronts = hb.get_tree()
    cls = [int(c) for c in hb.front_classes()]
    st = hb.stats()
    hb.close()
    nf = len(fronts)
    tree = [bool(c & 4) for c in cls]
    rows = [sum(int(arr.var_dims[v]) for v in f + s) + 1 for f, s in fronts]
    nchild, height, subn = [0] * nf, [0] * nf, [0] * nf
    for f in range(nf):                                   # children have smaller ids
        assert parent[f] < 0 or parent[f] > f
        if not tree[f]:
            continue
        subn[f] = max(subn[f], 141 if cls[f] & 3 == 3 else rows[f])
        p = parent[f]
        if p >= 0 and tree[p]:
            nchild[p] += 1
            height[p] = max(height[p], height[f] + 1)
            subn[p] = max(subn[p], subn[f])
    tier = [-1 if not tree[f] else sum(subn[f] > b for b in TIER_BOUNDS) for f in range(nf)]
    same = [0] * nf
    for f in range(nf):
        if tree[f] and parent[f] >= 0 and tier[parent[f]] == tier[f]:
            same[parent[f]] += 1
    roots = sum(1 for f in range(nf) if tree[f] and (parent[f] < 0 or not tree[parent[f]]))
    return {"scalars": int(arr.var_dims.sum()), "fronts": nf, "tree_fronts": sum(tree), "max_children": max(nchild),
            "height": max(height), "roots": roots, "tickets": roots + sum(max(c - 1, 0) for c in nchild),
            "starts": [sum(1 for f in range(nf) if tier[f] == t and same[f] == 0) for t in range(3)],
            "classes": set(cls), "tree_rows": [rows[f] for f in range(nf) if tree[f]],
            "tree_classes": set(cls[f] for f in range(nf) if tree[f]), "n_big_fronts": int(st["n_big_fronts"])}


# name -> (maker, environment the handle is created under, amalgamation)
DEEP_DENSE = {
    "chain600": (lambda: chain(600, 3), {}, DEEP_AMALGAMATION),
    "broom65": (lambda: broom(65, 3, 6), {}, DEEP_AMALGAMATION),
    "broom66": (lambda: broom(66, 3, 6), {}, DEEP_AMALGAMATION),
    "broom130": (lambda: broom(130, 3, 6), {}, DEEP_AMALGAMATION),
    "caterpillar200": (lambda: caterpillar(200), {}, DEEP_AMALGAMATION),
    "chain40x40": (lambda: chain(40, 40), {}, DEEP_AMALGAMATION),                        # the second tier (81 rows)
    "medium_chain": (lambda: chain(12, 48, band=2, tail_dim=8), {"GSX_MEDIUM": "1"}, DEEP_AMALGAMATION),
    "colamd_pose2": (colamd_pose2, {}, DEEP_AMALGAMATION),
}
DEEP_WIDE = {
    "forest1300": (lambda: forest(1300, 1), {}, DEEP_AMALGAMATION),
    "forest2100": (lambda: forest(2100, 1), {}, DEEP_AMALGAMATION),
    "chain1400": (lambda: chain(1400, 3), {}, DEEP_AMALGAMATION),
}
# test_neighbouring_lambdas_on_one_arena's sequence on one handle (the first solved twice by the tests), then the third
# of LAMBDAS
L2 = 0.1 * (1 + 1e-8)
DEEP_LAMBDAS = [(0.1, True), (L2, True), (0.0, False), (L2, True), (1e-3, False)]

# grids of the dependency-driven launches (kernels.hip: launch_front_tree; bigfront.hip: launch_backsolve_tree)
BACKSOLVE_TREE_GRID = 256 * 5


def front_tree_grid_cap(max_n, threads):
    """launch_front_tree: 256 CUs x min(156 KB / (LDS of the tier's largest front + 2 KB), 2048 / threads, 16)."""
    lds = (max_n * max_n + max_n) * 8
    return 256 * max(1, min((156 * 1024) // (lds + 2048), 2048 // threads, 16))


def assert_deep_shape(name, s):
    """The shape each deep / wide case is aimed at, from tree_shape() with the tree kernels on (host facts)."""
    assert s["n_big_fronts"] == 0, s
    assert all(c & 4 for c in s["tree_classes"]) and s["tree_fronts"] > 0, s
    rows = s["tree_rows"]
    if name == "chain600":
        assert s["height"] >= 500 and (s["max_children"], s["roots"], s["tickets"], s["starts"]) == (1, 1, 1, [1, 0, 0]), s
    elif name.startswith("broom"):
        arms = int(name[5:])
        assert (s["max_children"], s["tickets"], s["roots"], s["height"]) == (arms, arms, 1, 2), s
        assert s["tree_fronts"] == 2 * arms and s["scalars"] == 9 * arms + 6, s
    elif name == "caterpillar200":
        assert (s["scalars"], s["fronts"], s["tree_fronts"]) == (1800, 599, 399), s
        assert (s["max_children"], s["height"], s["roots"], s["tickets"]) == (2, 200, 1, 199), s
    elif name == "chain40x40":     # every front in the second tier (more than 67 rows, 512 threads)
        assert min(rows) > 67 and max(rows) <= 140 and s["tree_classes"] == {5}, s
        assert s["height"] == 38 and s["starts"] == [0, 1, 0] and s["tickets"] == 1, s
    elif name == "medium_chain":   # medium fronts (145 rows) under two LDS fronts, all in the medium tier, one chain
        assert s["tree_classes"] == {7, 5} and max(rows) > 140 and s["starts"] == [0, 0, 1], s
        assert s["height"] == s["tree_fronts"] - 1 == 9 and s["max_children"] == 1 and s["tickets"] == 1, s
        assert all(r * 48 <= 18432 for r in rows if r > 140), rows      # (kMedMaxPanel doubles of panel)
    elif name == "colamd_pose2":   # the reference's default ordering: ten times as deep as nested dissection's tree
        assert s["height"] >= 40 and s["tree_fronts"] >= 250 and s["roots"] == 1 and s["tickets"] > 1, s
    elif name == "forest1300":     # more tickets than backsolve_tree's grid
        assert s["roots"] == s["tickets"] == 1300 > BACKSOLVE_TREE_GRID and s["height"] == 0, s
    elif name == "forest2100":     # more start fronts than front_tree's grid: fronts of 3 rows in the 256-thread tier
        assert max(rows) == 3 and s["starts"] == [2100, 0, 0], s
        assert s["starts"][0] > front_tree_grid_cap(3, 256) == 2048 and s["tickets"] == 2100, s
    elif name == "chain1400":
        assert (s["scalars"], s["fronts"], s["tree_fronts"]) == (4200, 1399, 1398), s
        assert (s["max_children"], s["height"], s["roots"], s["tickets"]) == (1, 1397, 1, 1), s
    else:
        raise KeyError(name)
