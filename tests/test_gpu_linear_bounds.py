"""The elimination, back-substitution and marginal kernels under float64 BACKWARD-error bounds (tests/_ld_linear.py): the
device's own conditionals [R S d], gathered into R and d, must reproduce the damped system the kernels were given, and
its step that system's solution, to gamma = k u with k derived from the longest accumulation (a few hundred to a few
thousand u) — five or more digits under the forward-error bounds of the parity tests, and independent of conditioning
and of the oracle's rounding.  The cases are the smallest shapes that reach each front kernel (leaf, fused star, LDS,
medium, blocked, tree), each back-substitution kernel and each (child class, parent class) pair of marginals.hip; the
last test asserts that every front class really occurred.

The dependency-driven launches (front_tree, front_tree_med, backsolve_tree: one workgroup's results consumed by another
inside the launch) are also judged on deep and wide trees (test_deep_trees, test_wide_trees; _linear_cases.DEEP_DENSE /
DEEP_WIDE): chains 597 and 1397 fronts high that one workgroup climbs alone, parents with 65 / 66 / 130 tree children,
a caterpillar, chains in the second and in the medium tier, a pose graph under the reference's COLAMD ordering, and
forests with more tickets / start fronts than the launches' grids — each with the tree kernels on and off, over the
neighbouring-lambda sequence on one handle, with bit-equal repeats.  These judge the result of one run each: they cannot
show a race in the hand-off and do not loop to look for one.

gsx_get_conditional reports the factorization the arena holds: after solve(lambda, diag) the DAMPED one of that call
(handle.h: fact_lambda), after a marginal query the undamped one.  Measures (1) and (2) are therefore taken right after
each solve, against Hd of that lambda; measure (3) does not depend on it.

Every test prints its ratios in units of u (or of u kappa_2); the worst of the module are printed by the last test.
Measured on the MI355X: factor 29.1 u, rhs 18.6 u, solve 6.6 u, step 2.1 u kappa_2, marginals 1.1 u kappa_2.
The deep trees (both schedules alike): factor 4.9 u, rhs 2.9 u, solve 1.8 u, step 0.25 u kappa_2 against k of 1100 to 3600
(factor, rhs) and 3100 to 10900 (solve, step); the wide trees: rhs 2.2 u, solve 1.8 u against k of 7800 to 12600 and 23400
to 37800; nine tiers: factor 13.7 u, rhs 7.1 u, solve 2.6 u.
"""
import numpy as np
import pytest

from gtsam_petercdev_amd import _abi as A
from tests import _ld_linear as J
from tests import _linear_cases as cases

pytestmark = pytest.mark.gpu

SEEN = set()                                                   # union of front_classes() over the module
WORST = {"factor": 0.0, "rhs": 0.0, "solve": 0.0, "step": 0.0, "marginals": 0.0}


@pytest.fixture(scope="module")
def gpu():
    from gtsam_petercdev_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the HIP path has no fallback"
    return _lib


def _device_case(gpu, arr, ordering, amalgamation=(0.0, 128)):
    """(backend, judge, front classes): linearized under the ordering; the judge is built from the device's own [A b]."""
    gb = gpu.product_backend(arr)
    gb.set_amalgamation(*amalgamation)
    if isinstance(ordering, int):
        ordering = gb.compute_ordering(ordering)
    gb.set_ordering(ordering)
    cls = set(int(c) for c in gb.front_classes())
    SEEN.update(cls)
    gb.linearize()
    return gb, J.Judge(arr, gb.jacobians()), cls


def _judge(gb, judge, what, lambdas=cases.LAMBDAS, step=True):
    for lam, diag in lambdas:
        x = gb.solve(lam, diag)
        f, r, s = judge.check_backward(gb, x, lam, diag, what)
        for k, v in (("factor", f), ("rhs", r), ("solve", s)):
            WORST[k] = max(WORST[k], v)
        if step:
            WORST["step"] = max(WORST["step"], judge.check_step(x, lam, diag, what))


def _two_clique(gpu, dim_a, dim_b):
    arr, order, na, nb = cases.two_clique_arrays(dim_a, dim_b)
    gb, judge, cls = _device_case(gpu, arr, order)
    _, fronts = gb.get_tree()
    assert len(fronts) == 2 and sorted(len(f) for f, _ in fronts) == sorted([na, nb + 1])
    return gb, judge, cls


# ---- the size classes of the front and back-substitution kernels -------------------------------------------------------
@pytest.mark.parametrize("dim_a,dim_b", cases.LADDER)
def test_size_class_ladder(gpu, dim_a, dim_b):
    """(A | B) <- (B, c) with the child's frontal width over the leaf kernel's limit (16), the back-substitution kernels'
    (32 / 64), the blocked factorization's chunk (192; 385 = three chunks) and its height over the LDS / blocked boundary
    (140 rows): measures (1)-(3) on the full R, (4) on the step."""
    gb, judge, cls = _two_clique(gpu, dim_a, dim_b)
    _judge(gb, judge, f"ladder ({dim_a},{dim_b}) classes {sorted(cls)}")


@pytest.mark.parametrize("dim_a,dim_b", cases.LEAF_HEIGHTS)
def test_leaf_heights(gpu, dim_a, dim_b):
    """A leaf-kernel child at the boundaries of the leaf launch's thread classes (64 / 128 / 256 threads) and over the
    point where the parent becomes a blocked front and the leaf keeps only its panel (lean)."""
    gb, judge, cls = _two_clique(gpu, dim_a, dim_b)
    # (16 frontal scalars over 127-129 separator rows are past the LDS height with an LDS parent: a blocked child)
    assert (0 in {c & 3 for c in cls}) == (not (dim_a == 16 and 127 <= dim_b <= 129)), cls
    _judge(gb, judge, f"leaf ({dim_a},{dim_b}) classes {sorted(cls)}")


@pytest.mark.parametrize("tiers", ["default", "off"])
@pytest.mark.parametrize("dim_a,dim_b", cases.MEDIUM)
def test_medium_path(gpu, dim_a, dim_b, tiers, monkeypatch):
    """The dim B = 131 column with the MEDIUM-front path switched on: as a tree front (the medium tier) and in its level's
    launch."""
    monkeypatch.setenv("GSX_MEDIUM", "1")
    if tiers == "off":
        monkeypatch.setenv("GSX_TREE_TIERS", "0")
    gb, judge, cls = _two_clique(gpu, dim_a, dim_b)
    # the listed widths bracket the medium class: 15 frontal scalars still make a leaf-kernel front, and at 127 the panel
    # (259 rows x 127) is past what a medium front keeps in LDS — a blocked front; the four between are medium
    medium = dim_a in (17, 33, 64, 65)
    assert ((7 if tiers == "default" else 3) in cls) == medium, cls
    assert (gb.stats()["n_medium_fronts"] > 0) == medium
    assert medium or (0 if dim_a == 15 else 2) in cls, cls
    _judge(gb, judge, f"medium ({dim_a},{dim_b}) tiers {tiers} classes {sorted(cls)}")


# ---- the dependency-driven launches -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["tree", "levels"])
@pytest.mark.parametrize("name", ["pose3", "pose2"])
def test_tree_kernels(gpu, name, mode, monkeypatch):
    """The two makers of test_tree_kernels_against_the_level_launches (nested dissection; amalgamation 0.5 / 64, at which
    these sizes reach both tiers and no blocked front) with the tree kernels and with them switched off: each schedule on
    its own against the system, not against each other."""
    if mode == "levels":
        monkeypatch.setenv("GSX_TREE_TIERS", "0")
    gb, judge, cls = _device_case(gpu, cases.tree_arrays(name), A.ORDER_ND, cases.TREE_AMALGAMATION)
    st = gb.stats()
    assert (st["n_tree_fronts"] > 0) == (mode == "tree") and st["n_big_fronts"] == 0
    assert any(c & 4 for c in cls) == (mode == "tree")
    if mode == "tree":    # both tiers: fronts of at most 67 rows and taller ones
        _, fronts = gb.get_tree()
        rows = [sum(int(judge.sys.arrays.var_dims[v]) for v in f + s) + 1
                for (f, s), c in zip(fronts, gb.front_classes()) if c & 4]
        assert min(rows) <= 67 < max(rows), (min(rows), max(rows))
    _judge(gb, judge, f"tree kernels {name} {mode} classes {sorted(cls)}", step=False)


# ---- the dependency-driven launches on deep and wide trees ------------------------------------------------------------------------
_DEEP_JUDGES = {}          # case -> (jacobians, Judge): the system and its refined x* are shared by the two schedules of a case


def _deep_case(gpu, name, mode, monkeypatch, table):
    """The case's shape asserted host-only (tree kernels on), then the device handle under the schedule of `mode`."""
    maker, env, amalgamation = table[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    arr, ordering = maker()
    cases.assert_deep_shape(name, cases.tree_shape(arr, ordering, amalgamation))
    if mode == "levels":
        monkeypatch.setenv("GSX_TREE_TIERS", "0")
    gb = gpu.product_backend(arr)
    gb.set_amalgamation(*amalgamation)
    gb.set_ordering(ordering)
    cls = set(int(c) for c in gb.front_classes())
    SEEN.update(cls)
    st = gb.stats()
    assert st["n_big_fronts"] == 0 and (st["n_tree_fronts"] > 0) == (mode == "tree")
    assert any(c & 4 for c in cls) == (mode == "tree"), cls
    gb.linearize()
    return arr, gb, cls


def _repeat_is_bit_equal(gb, lam, diag, what):
    x = gb.solve(lam, diag)
    assert np.array_equal(x, gb.solve(lam, diag)), (what, "two solves at one lambda differ")


@pytest.mark.parametrize("mode", ["tree", "levels"])
@pytest.mark.parametrize("name", list(cases.DEEP_DENSE))
def test_deep_trees(gpu, name, mode, monkeypatch):
    """A workgroup that climbs (and descends) hundreds of fronts alone; parents with 65 / 66 / 130 tree children (the
    publish loop's one, two and three trips of 64 lanes; a pending counter counted down by as many workgroups); a chain in
    the second tier, one in the medium tier, and a pose graph under the reference's COLAMD ordering.  One handle, the
    neighbouring-lambda sequence: a counter not restored, a cursor not zeroed or a ticket of the previous epoch shows in
    the next solve, which is judged for ITS lambda.  Each schedule is judged on its own against the system."""
    arr, gb, cls = _deep_case(gpu, name, mode, monkeypatch, cases.DEEP_DENSE)
    jac = gb.jacobians()
    kept = _DEEP_JUDGES.pop(name, None)     # (the second schedule takes the judge out again: nothing stays behind)
    if kept is None:
        kept = _DEEP_JUDGES[name] = (jac, J.Judge(arr, jac))
    assert np.array_equal(jac, kept[0])
    what = f"deep {name} {mode} classes {sorted(cls)}"
    _repeat_is_bit_equal(gb, *cases.DEEP_LAMBDAS[0], what)
    _judge(gb, kept[1], what, lambdas=cases.DEEP_LAMBDAS, step=name != "colamd_pose2")


_WIDE_STEPS = {}           # case -> {(lambda, diag): the step of the first schedule that ran}


@pytest.mark.parametrize("mode", ["tree", "levels"])
@pytest.mark.parametrize("name", list(cases.DEEP_WIDE))
def test_wide_trees(gpu, name, mode, monkeypatch):
    """More tickets than backsolve_tree's grid (1300 roots), more start fronts than front_tree's (2100), and a chain 1397
    fronts high: measures (2) and (3) from the vector judge, bit-equal repeats, and the two schedules against each other
    at the tolerance of test_tree_kernels_against_the_level_launches."""
    arr, gb, cls = _deep_case(gpu, name, mode, monkeypatch, cases.DEEP_WIDE)
    judge = J.VectorJudge(arr, gb.jacobians())
    what = f"wide {name} {mode} classes {sorted(cls)}"
    _repeat_is_bit_equal(gb, *cases.DEEP_LAMBDAS[0], what)
    steps = {}
    for k, (lam, diag) in enumerate(cases.DEEP_LAMBDAS):
        x = gb.solve(lam, diag)
        r, s = judge.check_backward(gb, x, lam, diag, what)
        WORST["rhs"], WORST["solve"] = max(WORST["rhs"], r), max(WORST["solve"], s)
        if (lam, diag) in steps:
            assert np.array_equal(x, steps[(lam, diag)]), (what, "the same lambda later on the handle", lam)
        steps[(lam, diag)] = x
    other = _WIDE_STEPS.setdefault(name, steps)
    for key, x in steps.items():
        np.testing.assert_allclose(x, other[key], rtol=1e-9, atol=1e-11 * np.abs(other[key]).max(), err_msg=f"{what} {key}")


def test_nine_tiers_are_clamped(gpu, monkeypatch):
    """A GSX_TREE_TIERS list longer than the start-list cursors: the extra tiers' fronts go to the upper schedule (none is
    left unfactored), and the result holds the backward-error bounds."""
    monkeypatch.setenv("GSX_TREE_TIERS", "40:128,50:128,60:256,67:256,75:256,85:512,95:512,105:512,140:512")
    gb, judge, cls = _device_case(gpu, cases.tree_arrays("pose3"), A.ORDER_ND, cases.TREE_AMALGAMATION)
    rows = [sum(int(judge.sys.arrays.var_dims[v]) for v in f + s) + 1 for f, s in gb.get_tree()[1]]
    tree_rows = [r for r, c in zip(rows, gb.front_classes()) if c & 4]
    # seven bounds are kept (the eighth cursor is the medium tier's): tree fronts stop at 95 rows, and the 115-row LDS
    # front, which the ninth tier would have held, is eliminated by its level's launch
    upper = [r for r, c in zip(rows, gb.front_classes()) if c == 1]
    assert tree_rows and upper and max(tree_rows) <= 95 < max(upper) and min(tree_rows) <= 40, (tree_rows, upper)
    assert gb.stats()["n_big_fronts"] == 0
    _judge(gb, judge, f"nine tiers classes {sorted(cls)}", step=False)


# ---- structure ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relax", [0.0, 0.5])
@pytest.mark.parametrize("seed", cases.RANDOM_SEEDS)
def test_random_linear_graphs(gpu, seed, relax):
    """Hubs, chords, a dense cluster, variables of 1 to 40 dimensions, the reference's cliques and relaxed amalgamation."""
    gb, judge, cls = _device_case(gpu, cases.random_linear_arrays(seed), A.ORDER_MINDEGREE, (relax, 128))
    _judge(gb, judge, f"random graph {seed} relax {relax} classes {sorted(cls)}")


@pytest.mark.parametrize("relax", [0.0, 0.5])
@pytest.mark.parametrize("name", ["bal7", "bal30", "pose3_chain"])
def test_nonlinear_problems(gpu, name, relax):
    """Bundle adjustment under the Schur ordering (fused star leaves, stored and product-form complements, lean leaves) and
    a Pose3 chain with loop closures.  [A b] is what jacobians() returns: the float64 input of the elimination."""
    arr = cases.pose3_arrays() if name == "pose3_chain" else cases.bal_arrays(int(name[3:]))
    gb, judge, cls = _device_case(gpu, arr, A.ORDER_ND if name == "pose3_chain" else A.ORDER_SCHUR, (relax, 128))
    if name == "bal30":
        assert 8 in cls, cls
    _judge(gb, judge, f"{name} relax {relax} classes {sorted(cls)}", lambdas=[(0.1, True), (1e-3, False)], step=False)


# ---- two trials at neighbouring lambdas on one arena ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blocked", "tree", "bal7"])
def test_neighbouring_lambdas_on_one_arena(gpu, name):
    """One handle, no relinearization: lambda1 = 0.1, lambda2 = 0.1 (1 + 1e-8), 0, lambda2 again (diagonal damping), each
    result judged for ITS lambda.  A square, a panel or a right-hand side left over from the previous trial is 1e7 u off;
    the forward-error tests cannot tell trials this close apart.  (Run once: this judges results, it does not hunt a
    race.)"""
    if name == "blocked":
        gb, judge, cls = _two_clique(gpu, 193, 60)
        assert 2 in {c & 3 for c in cls}
    elif name == "tree":
        gb, judge, cls = _device_case(gpu, cases.tree_arrays("pose3"), A.ORDER_ND, cases.TREE_AMALGAMATION)
        assert any(c & 4 for c in cls)
    else:
        gb, judge, cls = _device_case(gpu, cases.bal_arrays(7), A.ORDER_SCHUR)
    l2 = 0.1 * (1 + 1e-8)
    _judge(gb, judge, f"neighbouring lambdas {name}", lambdas=[(0.1, True), (l2, True), (0.0, False), (l2, True)],
           step=False)


# ---- marginals ------------------------------------------------------------------------------------------------------------------
def _judge_marginals(gb, judge, what):
    """All blocks of marginal_covariances(), a key list, the per-variable entry point and one joint marginal against the
    refined inverse (after a solve at lambda = 0, as the existing tests do)."""
    gb.solve(0.0, False)
    keys = [int(k) for k in judge.sys.arrays.var_keys]
    blocks = gb.marginal_covariances()
    assert sorted(blocks) == keys
    worst = max(judge.check_covariance([k], blocks[k], what + " all") for k in keys)
    some = keys[::3][::-1]
    listed = gb.marginal_covariances(some)
    assert sorted(listed) == sorted(some)
    worst = max([worst] + [judge.check_covariance([k], listed[k], what + " list") for k in some])
    worst = max([worst] + [judge.check_covariance([k], gb.marginal_covariance(k), what + " single") for k in keys])
    jk = [keys[0], keys[len(keys) // 2], keys[-1]]
    worst = max(worst, judge.check_covariance(jk, gb.joint_marginal_covariance(jk), what + " joint"))
    print(f"{what}: marginals {worst:.3f} u*kappa (kappa {judge.sigma()[1]:.1f}, k {judge.ks})")
    WORST["marginals"] = max(WORST["marginals"], worst)


@pytest.mark.parametrize("dim_a,dim_b", cases.MARGINAL_POINTS)
def test_marginals_on_the_ladder(gpu, dim_a, dim_b):
    """Between them the five points cover the six (child class, parent class) pairs of marginals.hip."""
    gb, judge, cls = _two_clique(gpu, dim_a, dim_b)
    _judge_marginals(gb, judge, f"marginals ({dim_a},{dim_b}) classes {sorted(cls)}")


@pytest.mark.parametrize("name", ["random1", "random3", "bal7"])
def test_marginals_on_graphs(gpu, name):
    """Two random graphs and the 7-camera bundle.  The bundle's gauge is held by weak priors only: kappa_2(H) is about
    2e10, so its bound gamma kappa_2 is about 1e-2 max|S*| and S* itself (a stalled refinement, see _ld_linear._converged)
    is good to about 1e-9 — this case checks the entry points on fused-star / lean structure, it is NOT tight; the five
    ladder points and the random graphs (kappa_2 below 1000) carry the tight marginal check."""
    if name == "bal7":
        gb, judge, cls = _device_case(gpu, cases.bal_arrays(7), A.ORDER_SCHUR)
    else:
        gb, judge, cls = _device_case(gpu, cases.random_linear_arrays(int(name[6:])), A.ORDER_MINDEGREE)
    _judge_marginals(gb, judge, f"marginals {name} classes {sorted(cls)}")


# ---- every case reached the kernel it was aimed at --------------------------------------------------------------------------------
def test_every_front_class_was_judged():
    """The union of front_classes() over the cases above: leaf kernel 0, LDS 1, blocked 2, medium 3, the tree fronts 1|4
    and 3|4, and the lean leaf 0|8.  (symbolic.cpp gives a tree tier to LDS-class fronts only — class 1, medium included —
    so 0|4 and 2|4 do not exist; bit 3 only goes with class 0.)  SEEN and WORST are filled by the tests above: this test
    means something only when the whole module runs in one process, in file order; alone, under -k, --lf or split over
    workers it fails for want of the others, not because a class is unreachable."""
    print("front classes judged:", sorted(SEEN), "worst ratios (u; step and marginals in u*kappa_2):",
          {k: round(v, 3) for k, v in WORST.items()})
    assert SEEN >= {0, 1, 2, 3, 1 | 4, 3 | 4, 0 | 8}, sorted(SEEN)
