"""Marginal covariances of all variables from one top-down pass on the device (gsx_marginal_covariances, marginals.hip)
against the oracle's dense inverse where that is small enough, and against the per-variable entry point
(gsx_marginal_covariance: forward substitution up one clique path, independent code) on larger graphs.

Bound per block, as test_marginal_covariance_matches_oracle uses for the per-variable entry point:
max|S_g - S_o| <= 1e-7 max|S_o|.
"""
import numpy as np
import pytest

import gtsam_petercdev_amd as gt
from gtsam_petercdev_amd import _abi as A
from gtsam_petercdev_amd import datasets
from gtsam_petercdev_amd.graph import (Pose2, Values, NonlinearFactorGraph, GaussianFactorGraph, JacobianFactor,
                                       BetweenFactor, PriorFactor, noiseModel, Marginals)
from tests.test_gpu_parity import PROBLEMS, relerr

pytestmark = pytest.mark.gpu

BOUND = 1e-7


@pytest.fixture(scope="module")
def gpu():
    from gtsam_petercdev_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the HIP path has no fallback"
    return _lib


def _dense_blocks(ob, arr):
    """{key: block} of the oracle's dense H^-1 (joint marginal of all keys, in key order)."""
    keys = [int(k) for k in arr.var_keys]
    J = ob.joint_marginal_covariance(keys)
    off = np.concatenate([[0], np.cumsum(arr.var_dims)]).astype(int)
    return {k: J[off[i]:off[i + 1], off[i]:off[i + 1]] for i, k in enumerate(keys)}


def _check_blocks(got, expected, what):
    assert set(got) == set(expected), what
    worst = 0.0
    for k, co in expected.items():
        cg = got[k]
        assert cg.shape == co.shape, (what, k)
        assert np.allclose(cg, cg.T, rtol=1e-9, atol=1e-14 * np.max(np.abs(co))), (what, k)
        err = float(np.max(np.abs(cg - co)) / np.max(np.abs(co)))
        worst = max(worst, err)
        assert err <= BOUND, (what, k, err)
    print(f"all-marginals {what}: {len(expected)} blocks, worst relative error {worst:.3e}")
    return worst


# ---- 2. every variable of the parity problems against the oracle ----------------------------------------------------------
@pytest.mark.parametrize("name", ["bal_small", "bal_bigfront", "bal_wide_landmarks", "pose2", "pose3"])
@pytest.mark.parametrize("relax", [0.0, 0.5])
@pytest.mark.parametrize("natural", [False, True])
def test_all_marginals_match_oracle(gpu, oracle, name, relax, natural):
    arr = PROBLEMS[name]
    assert int(arr.var_dims.sum()) <= 6000
    gb, ob = gpu.product_backend(arr), oracle.oracle_backend(arr)
    kind = A.ORDER_NATURAL if natural else (A.ORDER_SCHUR_ND if name.startswith("bal") else A.ORDER_ND)
    ordering = gb.compute_ordering(kind)
    gb.set_amalgamation(relax, 128)
    gb.set_ordering(ordering)
    ob.set_ordering(ordering)
    gb.linearize()
    ob.linearize()
    _check_blocks(gb.marginal_covariances(), _dense_blocks(ob, arr), (name, relax, natural))
    # the arena still holds the undamped factorization: a following solve is unaffected
    assert relerr(gb.solve(1e-3, False), ob.solve(1e-3, False)) < 1e-8


# ---- 3. the reference's planar-SLAM known answers (tests/testMarginals.cpp:76-100) ----------------------------------------
def test_planarSLAM_all_marginals(gpu):
    from tests.test_oracle_golden import PLANAR_SLAM_MARGINALS, planar_slam_linear_graph
    arrays = planar_slam_linear_graph().to_arrays(None)
    arrays.values = np.zeros(int(arrays.var_dims.sum()))
    for ordering in ([1, 2, 3, 11, 12], [11, 12, 1, 2, 3], [3, 12, 2, 11, 1]):
        be = gpu.product_backend(arrays)
        be.set_ordering(ordering)
        be.linearize()
        got = be.marginal_covariances()
        assert sorted(got) == sorted(PLANAR_SLAM_MARGINALS)
        for key, expected in PLANAR_SLAM_MARGINALS.items():
            assert np.allclose(got[key], expected, atol=1e-8), (ordering, key)
        some = be.marginal_covariances([12, 2])
        assert list(some) == [12, 2] and np.array_equal(some[12], got[12]) and np.array_equal(some[2], got[2])


def test_Marginals_class_serves_from_one_pass(gpu):
    from tests.test_oracle_golden import PLANAR_SLAM_MARGINALS, planar_slam_nonlinear_graph
    g, v = planar_slam_nonlinear_graph()
    m = Marginals(g, v, ordering=[1, 2, 3, 11, 12], backend_factory=gpu.product_backend)
    single = m.marginalCovariance(2)
    blocks = m.marginalCovariances()
    for key, expected in PLANAR_SLAM_MARGINALS.items():
        assert np.allclose(blocks[key], expected, atol=1e-8), key
        assert np.array_equal(m.marginalCovariance(key), blocks[key])
    assert np.allclose(single, blocks[2], atol=1e-12)
    assert list(m.marginalCovariances([11, 1])) == [11, 1]


# ---- 4. the size-class boundaries ------------------------------------------------------------------------------------------
def _split_dims(total, rng):
    out = []
    while total > 0:
        d = int(min(total, rng.integers(1, 9)))
        out.append(d)
        total -= d
    return out


def _two_clique_arrays(dim_a, dim_b):
    """The tree (A | B) <- (B, c) of test_gpu_parity._two_clique_case under the ordering 0 .. nv - 1, amalgamation off."""
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
    return arr, [((0.0, 128), list(range(nv)))]


def _wide_arrays(seed, dense):
    """The graph of test_linear_graph_with_wide_variables: vector variables of 1 to 40 dimensions."""
    rng = np.random.default_rng(seed)
    dims = [int(d) for d in rng.choice([1, 2, 5, 9, 17, 24, 33, 40], size=36)]
    fg = GaussianFactorGraph()
    for k, d in enumerate(dims):
        fg.add(JacobianFactor(k, np.eye(d) + 0.1 * rng.normal(size=(d, d)), rng.normal(size=d),
                              noiseModel.Isotropic.Sigma(d, 1.0 + 0.1 * k)))
    pairs = [(k, k + 1) for k in range(len(dims) - 1)] + [(int(a), int(b)) for a, b in rng.integers(0, len(dims), (30, 2)) if a != b]
    if dense:
        pairs += [(a, b) for a in range(8, 16) for b in range(a + 1, 16)]
    for a, b in pairs:
        m = max(1, min(dims[a], dims[b], 6))
        fg.add(JacobianFactor(a, rng.normal(0, 0.3, (m, dims[a])), b, rng.normal(0, 0.3, (m, dims[b])), rng.normal(size=m),
                              noiseModel.Diagonal.Sigmas(0.5 + rng.random(m))))
    arr = fg.to_arrays(None)
    arr.values = np.zeros(int(arr.var_dims.sum()))
    assert int(arr.var_dims.max()) > 16
    return arr, [((0.0, 128), A.ORDER_MINDEGREE), ((0.0, 128), A.ORDER_ND), ((0.5, 64), A.ORDER_NATURAL)]


def _fuzz_arrays(seed):
    """The structure fuzz of test_random_linear_graphs: chains with chords, hubs, dense clusters, variables of 1-9 dimensions."""
    rng = np.random.default_rng(1000 + seed)
    nv = int(rng.choice([4, 9, 30, 70, 140, 260]))
    dim_sets = ([3], [6], [1, 2, 3], [2, 6, 9], [9, 3])
    ds = dim_sets[seed % len(dim_sets)]
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
    return arr, [((0.0, 128), (A.ORDER_NATURAL, bool(seed % 2))), (None, A.ORDER_MINDEGREE), ((1.0, 48), A.ORDER_ND)]


TWO_CLIQUE = [(a, b) for b in (12, 60, 131, 150)
              for a in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 230)]
SWEEP = ([("two", c) for c in TWO_CLIQUE] + [("wide", c) for c in ((1, False), (2, True))] +
         [("fuzz", s) for s in range(24)])


def _sweep_case(case):
    what, c = case
    if what == "two":
        return _two_clique_arrays(*c)
    if what == "wide":
        return _wide_arrays(*c)
    return _fuzz_arrays(c)


def _set_config(be, amalg, order):
    """One (amalgamation, ordering) setting of a sweep case on a backend; returns the ordering (amalg None: keep)."""
    if isinstance(order, tuple):
        kind, rev = order
        ordering = be.compute_ordering(kind)
        if rev:
            ordering = ordering[::-1].copy()
    elif isinstance(order, list):
        ordering = order
    else:
        ordering = be.compute_ordering(order)
    if amalg is not None:
        be.set_amalgamation(*amalg)
    be.set_ordering(ordering)
    return ordering


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: f"{c[0]}-{c[1]}")
def test_size_class_boundaries(gpu, oracle, case):
    arr, configs = _sweep_case(case)
    gb, ob = gpu.product_backend(arr), oracle.oracle_backend(arr)
    for amalg, order in configs:
        ordering = _set_config(gb, amalg, order)
        ob.set_ordering(ordering)
        gb.linearize()
        ob.linearize()
        _check_blocks(gb.marginal_covariances(), _dense_blocks(ob, arr), (case, amalg, order))


def test_size_class_pairs_are_all_met(gpu):
    """The sweep above meets every (child class, parent class) pair that exists — a class-0 clique is childless — and a
    leaf-kernel clique with more than 64 separator rows (the strips of the leaf kernel)."""
    pairs, tallest_leaf = set(), 0
    for case in SWEEP:
        arr, configs = _sweep_case(case)
        be = gpu.product_backend(arr)
        for amalg, order in configs:
            _set_config(be, amalg, order)
            parent, fronts = be.get_tree()
            cls = [min(int(c) & 3, 2) if (int(c) & 3) != 3 else 1 for c in be.front_classes()]
            for f, p in enumerate(parent):
                if p >= 0:
                    pairs.add((cls[f], cls[p]))
                if cls[f] == 0:
                    tallest_leaf = max(tallest_leaf, int(sum(arr.var_dims[v] for v in fronts[f][1])))
        be.close()
    assert pairs == {(0, 1), (0, 2), (1, 1), (1, 2), (2, 1), (2, 2)}, pairs
    assert tallest_leaf > 64


# ---- 5. larger graphs against the per-variable entry point --------------------------------------------------------------------
def _big(name):
    if name == "pose3":
        return datasets.synth_manhattan_pose3(3000, seed=2), A.ORDER_ND
    if name == "pose2":
        return datasets.synth_manhattan_pose2(5000, seed=2), A.ORDER_ND
    return datasets.synth_bal_arrays(49, 7776, 31843, seed=42), A.ORDER_SCHUR_ND


def _against_per_variable(gb, blocks, keys, what):
    worst = 0.0
    for k in keys:
        co = gb.marginal_covariance(k)
        cg = blocks[k]
        assert np.allclose(cg, cg.T, rtol=1e-9, atol=1e-14 * np.max(np.abs(co))), (what, k)
        err = float(np.max(np.abs(cg - co)) / np.max(np.abs(co)))
        worst = max(worst, err)
        assert err <= BOUND, (what, k, err)
    print(f"all-marginals {what}: {len(keys)} blocks against the per-variable entry point, worst {worst:.3e}")


@pytest.mark.parametrize("name", ["pose3", "pose2", "bal49"])
def test_large_graphs_against_the_per_variable_entry_point(gpu, name):
    arr, kind = _big(name)
    gb = gpu.product_backend(arr)
    ordering = gb.compute_ordering(kind)
    gb.set_ordering(ordering)
    gb.linearize()
    blocks = gb.marginal_covariances()
    assert len(blocks) == arr.n_vars
    rng = np.random.default_rng(7)
    keys = [int(k) for k in rng.choice(arr.var_keys, size=200, replace=False)]
    for k in (int(ordering[0]), int(ordering[-1])):
        if k not in keys:
            keys.append(k)
    _against_per_variable(gb, blocks, keys, name)
    some = gb.marginal_covariances(keys)
    assert list(some) == keys
    for k in keys:
        assert np.array_equal(some[k], blocks[k]), (name, k)


# ---- 6. repeatability, the factorization left behind, stale tables ------------------------------------------------------------
@pytest.mark.parametrize("name", ["bal_bigfront", "pose3"])
def test_repeatable_and_not_stale(gpu, oracle, name):
    arr = PROBLEMS[name]
    gb, ob = gpu.product_backend(arr), oracle.oracle_backend(arr)
    kinds = (A.ORDER_SCHUR_ND, A.ORDER_SCHUR) if name.startswith("bal") else (A.ORDER_ND, A.ORDER_MINDEGREE)
    oa, o2 = gb.compute_ordering(kinds[0]), gb.compute_ordering(kinds[1])
    gb.set_ordering(oa)
    ob.set_ordering(oa)
    gb.linearize()
    ob.linearize()
    first, second = gb.marginal_covariances(), gb.marginal_covariances()
    for k in first:
        assert np.array_equal(first[k], second[k]), k
    assert relerr(gb.solve(1e-3, False), ob.solve(1e-3, False)) < 1e-8
    # another tree on the same handle: the covariance arena and the work lists of the old one must not be used
    gb.set_ordering(o2)
    keys = [int(k) for k in arr.var_keys]
    _against_per_variable(gb, gb.marginal_covariances(), keys, (name, "reordered"))
    _check_blocks(gb.marginal_covariances(), first, (name, "reordered against the first ordering"))


def test_after_update(gpu):
    arr = datasets.synth_manhattan_pose2(400, seed=3)
    gb = gpu.product_backend(arr)
    gb.set_ordering(gb.compute_ordering(A.ORDER_ND))
    gb.linearize()
    before = gb.marginal_covariances()
    i = arr.n_vars // 2
    so = arr.state_offsets()
    arr2 = arr.with_factor(A.F_PRIOR, [i], 3, arr.values[so[i]:so[i] + 3], A.NOISE_DIAGONAL, [0.05, 0.05, 0.02])
    gb.update(arr2, list(range(arr.n_factors)) + [-1], np.zeros(0))
    after = gb.marginal_covariances()
    keys = [int(k) for k in arr.var_keys]
    _against_per_variable(gb, after, keys, "after gsx_update")
    ki = int(arr.var_keys[i])
    assert np.trace(after[ki]) < np.trace(before[ki])   # the new prior was seen


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    # hard constraints
    fg = GaussianFactorGraph()
    fg.add(JacobianFactor(0, np.eye(2), [1.0, -1.0], noiseModel.Constrained.All(2)))
    fg.add(JacobianFactor(0, np.eye(2), 1, -np.eye(2), [0.5, 0.5], noiseModel.Isotropic.Sigma(2, 1.0)))
    fg.add(JacobianFactor(1, np.eye(2), [0.0, 0.0], noiseModel.Isotropic.Sigma(2, 1.0)))
    arr = fg.to_arrays(None)
    arr.values = np.zeros(int(arr.var_dims.sum()))
    be = gpu.product_backend(arr)
    be.set_ordering([0, 1])
    be.linearize()
    with pytest.raises(gt.GsxError) as ei:
        be.marginal_covariances()
    assert ei.value.status == A.GSX_E_STATE
    # a sharded handle
    arr = datasets.synth_manhattan_pose2(200, seed=1)
    sh = gpu.product_backend(arr)
    sh.set_shard(0, 2, lambda ptr, count: None)
    sh.set_ordering(sh.compute_ordering(A.ORDER_ND))
    with pytest.raises(gt.GsxError) as ei:
        sh.marginal_covariances()
    assert ei.value.status == A.GSX_E_STATE
    # repeated and unknown keys, wrong size
    be = gpu.product_backend(arr)
    be.set_ordering(be.compute_ordering(A.ORDER_ND))
    be.linearize()
    k0, k1 = int(arr.var_keys[0]), int(arr.var_keys[1])
    assert be.marginal_blocks_size([k0, k1, k0]) == -1
    for bad in ([k0, k1, k0], [k0, int(arr.var_keys.max()) + 5]):
        with pytest.raises(gt.GsxError) as ei:
            be.marginal_covariances(bad)
        assert ei.value.status == A.GSX_E_INVALID
    assert be.marginal_covariances([]) == {}


def test_underconstrained_then_anchored(gpu):
    """A gauge-free graph (the pattern of test_failed_factorization_is_not_reused): an indeterminate Gauss-Newton run
    leaves a failed factorization in the arena, the pass must report GSX_E_INDETERMINATE, not read the wreck; once a prior
    anchors the gauge the same call is correct."""
    fg = NonlinearFactorGraph()
    for i in range(5):
        fg.add(BetweenFactor(i, i + 1, Pose2(1, 0, 0.1), noiseModel.Isotropic.Sigma(3, 0.1)))
    v = Values()
    for i in range(6):
        v.insert(i, Pose2(1.0 * i + 0.05 * i, 0.02 * i, 0.1 * i))
    be = gpu.product_backend(fg.to_arrays(v))
    be.set_ordering(list(range(6)))
    with pytest.raises(gt.IndeterminantLinearSystemException):
        be.gn_optimize(max_iterations=3)
    with pytest.raises(gt.IndeterminantLinearSystemException):
        be.marginal_covariances()
    with pytest.raises(gt.IndeterminantLinearSystemException):
        be.marginal_covariances([2])
    fg.add(PriorFactor(0, Pose2(0, 0, 0), noiseModel.Isotropic.Sigma(3, 0.1)))
    be = gpu.product_backend(fg.to_arrays(v))
    be.set_ordering(list(range(6)))
    blocks = be.marginal_covariances()
    _against_per_variable(be, blocks, list(range(6)), "anchored chain")
