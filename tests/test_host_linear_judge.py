"""Pins the extended-precision judge of tests/_ld_linear.py without a GPU: its longdouble arithmetic against mpmath at 50
digits, the CPU oracle under its four measures on every linear case the device is judged on, and four mutations of a
correct oracle result that must each fail the measure that owns them (the judge can bite without touching a kernel).
The deep and wide trees of the dependency-driven launches (chains, brooms, a caterpillar, forests, a pose graph under
COLAMD) have their shapes asserted here host-only, and the oracle is judged on them: densely, or by the vector judge, which
is pinned against the dense one.

Measured (CPU oracle, worst over the cases): factor 13.5 u, rhs 8.3 u, solve 5.2 u against k of 100 to 3700 (factor, rhs)
and 190 to 11000 (solve); step 1.6 and marginals 1.1 u kappa_2 against the same k, kappa_2 between 5 and 1000 (2e10 for
the marginals of the bundle-adjustment case, whose gauge only weak priors hold).  On the deep and wide trees: factor 4.6 u,
rhs 2.8 u, solve 1.9 u, step 0.27 u kappa_2 (k of 1100 to 12600 and 3100 to 37800)."""
import mpmath
import numpy as np
import pytest

from gtsam_petercdev_amd import _abi as A
from tests import _ld_linear as J
from tests import _linear_cases as cases

LD = np.longdouble


def _oracle_case(oracle, arr, ordering):
    ob = oracle.oracle_backend(arr)
    ob.set_ordering(ordering)
    ob.linearize()
    return ob, J.Judge(arr, ob.jacobians())


# ---- the judge's own arithmetic ----------------------------------------------------------------------------------------
def _mp(a):
    return mpmath.matrix([[mpmath.mpf(float(v)) + mpmath.mpf(float(v - LD(float(v)))) for v in row] for row in np.atleast_2d(a)])


def _rel(got, want):
    """max |got - want| / max |want| with the difference taken in mpmath (got: longdouble array, want: mpmath matrix)."""
    g = _mp(got)
    if g.rows != want.rows:
        g = g.T
    diff = max(abs(g[i, j] - want[i, j]) for i in range(want.rows) for j in range(want.cols))
    return float(diff / max(abs(want[i, j]) for i in range(want.rows) for j in range(want.cols)))


@pytest.mark.parametrize("dim_a,dim_b", [(1, 12), (17, 12), (16, 20)])
def test_longdouble_arithmetic_against_mpmath(oracle, dim_a, dim_b):
    """Gram matrix, product, refined solve and refined inverse of the judge against 50-digit arithmetic, n <= 40."""
    arr, order, _, _ = cases.two_clique_arrays(dim_a, dim_b)
    ob, judge = _oracle_case(oracle, arr, order)
    S = judge.sys
    assert S.n <= 40
    mpmath.mp.dps = 50
    Ad = np.zeros((sum(b[1].shape[0] for b in S.blocks), S.n))
    bd = np.zeros(Ad.shape[0])
    r = 0
    for idx, Af, bf in S.blocks:
        Ad[r:r + Af.shape[0], idx] = Af.astype(np.float64)
        bd[r:r + Af.shape[0]] = bf.astype(np.float64)
        r += Af.shape[0]
    Am, bm = mpmath.matrix(Ad.tolist()), mpmath.matrix(bd.tolist())
    Hm = Am.T * Am
    gm = Am.T * bm
    assert _rel(S.H, Hm) <= 1e-17
    assert _rel(S.g, gm) <= 1e-17
    absHm = mpmath.matrix(np.abs(Ad).tolist())
    assert _rel(S.absH, absHm.T * absHm) <= 1e-17
    lam = 0.1
    Hdm = Hm.copy()
    for i in range(S.n):
        Hdm[i, i] += mpmath.mpf(lam) * max(Hm[i, i], mpmath.mpf(1e-6))
    assert _rel(S.damped(lam, True), Hdm) <= 1e-17
    x = np.linspace(-1.0, 2.0, S.n)
    assert _rel(S.times(x, lam, True), Hdm * mpmath.matrix(x.tolist())) <= 1e-17
    xs, kappa = J.refined_solve(S, lam, True)
    assert _rel(xs, mpmath.lu_solve(Hdm, gm)) <= 1e-17
    Sg, kappa0 = J.refined_inverse(S.H)
    assert _rel(Sg, Hm ** -1) <= 1e-17
    ev = np.linalg.eigvalsh(S.H.astype(np.float64))
    assert abs(kappa0 - ev[-1] / ev[0]) <= 1e-9 * kappa0


def test_k_is_what_the_derivation_says():
    assert J.k_factor(100, 300) == 2 * (100 + 5 + 300 + 5)
    assert J.k_solve(100, 300) == 2 * ((100 + 5) + (300 + 5) + (300 + 1) + (300 + 5))
    assert J.U == 2.0 ** -53 and np.finfo(LD).eps <= 2.0 ** -63


# ---- the oracle under the four measures ------------------------------------------------------------------------------------
def _judge_oracle(ob, judge, what, lambdas=cases.LAMBDAS, step=True):
    for lam, diag in lambdas:
        x = ob.solve(lam, diag)
        judge.check_backward(ob, x, lam, diag, what)
        if step:
            judge.check_step(x, lam, diag, what)


def _judge_oracle_marginals(ob, judge, what):
    """Every variable's marginal and one joint of three variables against the refined inverse (after a solve at 0)."""
    ob.solve(0.0, False)
    keys = [int(k) for k in judge.sys.arrays.var_keys]
    worst = max(judge.check_covariance([k], ob.marginal_covariance(k), what) for k in keys)
    jk = [keys[0], keys[len(keys) // 2], keys[-1]]
    worst = max(worst, judge.check_covariance(jk, ob.joint_marginal_covariance(jk), what))
    print(f"{what}: marginals {worst:.3f} u*kappa (kappa {judge.sigma()[1]:.1f}, k {judge.ks})")


@pytest.mark.parametrize("dim_a,dim_b", cases.LADDER + cases.LEAF_HEIGHTS)
def test_oracle_two_clique_cases(oracle, dim_a, dim_b):
    arr, order, _, _ = cases.two_clique_arrays(dim_a, dim_b)
    ob, judge = _oracle_case(oracle, arr, order)
    _judge_oracle(ob, judge, f"oracle two-clique ({dim_a},{dim_b})")
    if (dim_a, dim_b) in cases.MARGINAL_POINTS:
        _judge_oracle_marginals(ob, judge, f"oracle two-clique ({dim_a},{dim_b})")


@pytest.mark.parametrize("seed", cases.RANDOM_SEEDS)
def test_oracle_random_linear_graphs(oracle, seed):
    from gtsam_petercdev_amd import _lib
    arr = cases.random_linear_arrays(seed)
    ordering = _lib.ProductBackend(arr, host_only=True).compute_ordering(A.ORDER_MINDEGREE)
    ob, judge = _oracle_case(oracle, arr, ordering)
    _judge_oracle(ob, judge, f"oracle random graph {seed}")
    if seed in (1, 3):
        _judge_oracle_marginals(ob, judge, f"oracle random graph {seed}")


@pytest.mark.parametrize("name", ["bal7", "pose3"])
def test_oracle_nonlinear_cases(oracle, name):
    """[A b] is what jacobians() returns: the float64 input of the elimination (linearization is judged elsewhere)."""
    from gtsam_petercdev_amd import _lib
    arr = cases.bal_arrays(7) if name == "bal7" else cases.pose3_arrays()
    kind = A.ORDER_SCHUR if name == "bal7" else A.ORDER_ND
    ordering = _lib.ProductBackend(arr, host_only=True).compute_ordering(kind)
    ob, judge = _oracle_case(oracle, arr, ordering)
    _judge_oracle(ob, judge, f"oracle {name}", lambdas=[(0.1, True), (1e-3, False)])
    if name == "bal7":
        ob.solve(0.0, False)
        keys = [int(k) for k in arr.var_keys]
        worst = max(judge.check_covariance([k], ob.marginal_covariance(k), name) for k in keys[:3] + keys[-3:])
        print(f"oracle {name}: marginals {worst:.3f} u*kappa (kappa {judge.sigma()[1]:.1f}, k {judge.ks})")


# ---- the deep and wide trees of the dependency-driven launches ---------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.DEEP_DENSE) + list(cases.DEEP_WIDE))
def test_deep_and_wide_shapes(name, monkeypatch):
    """What each case is aimed at (depth, children of one parent, tickets, start fronts, tier) is a fact of the symbolic
    analysis: asserted here without a GPU, and again by the device tests before they judge."""
    maker, env, amalgamation = {**cases.DEEP_DENSE, **cases.DEEP_WIDE}[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    arr, ordering = maker()
    shape = cases.tree_shape(arr, ordering, amalgamation)
    print(name, {k: v for k, v in shape.items() if k != "tree_rows"}, "rows", min(shape["tree_rows"]), max(shape["tree_rows"]))
    cases.assert_deep_shape(name, shape)
    monkeypatch.setenv("GSX_TREE_TIERS", "0")
    off = cases.tree_shape(arr, ordering, amalgamation)
    assert off["tree_fronts"] == 0 and not any(c & 4 for c in off["classes"]) and off["n_big_fronts"] == 0, off


@pytest.mark.parametrize("name", list(cases.DEEP_DENSE))
def test_oracle_deep_dense_cases(oracle, name):
    """The oracle under the unchanged k on every densely judged deep case (m, the longest accumulation, is 267 on the hub of
    the 130-arm broom).  Measure (4) where kappa_2 allows it: the pose graph under COLAMD has kappa_2 of 1e6."""
    arr, ordering = cases.DEEP_DENSE[name][0]()
    ob, judge = _oracle_case(oracle, arr, ordering)
    _judge_oracle(ob, judge, f"oracle {name}", lambdas=cases.DEEP_LAMBDAS, step=name != "colamd_pose2")


@pytest.mark.parametrize("name", list(cases.DEEP_WIDE))
def test_oracle_wide_cases(oracle, name):
    """Measures (2) and (3) of the oracle on the cases too large for the dense judge."""
    arr, ordering = cases.DEEP_WIDE[name][0]()
    ob = oracle.oracle_backend(arr)
    ob.set_ordering(ordering)
    ob.linearize()
    judge = J.VectorJudge(arr, ob.jacobians())
    for lam, diag in cases.DEEP_LAMBDAS:
        judge.check_backward(ob, ob.solve(lam, diag), lam, diag, f"oracle {name}")


# ---- mutations of a correct result: each must fail the measure that owns it ----------------------------------------------------
class _Frozen:
    """A backend's tree and conditionals, copied: what gather() reads, open to mutation."""

    def __init__(self, backend):
        self.parent, self.fronts = backend.get_tree()
        self.conds = [np.array(backend.conditional(c)) for c in range(len(self.fronts))]

    def get_tree(self):
        return self.parent, self.fronts

    def conditional(self, c):
        return self.conds[c]


@pytest.fixture(scope="module")
def correct(oracle):
    arr, order, _, _ = cases.two_clique_arrays(33, 60)
    ob, judge = _oracle_case(oracle, arr, order)
    lam = 0.1
    x = ob.solve(lam, True)
    frozen = _Frozen(ob)
    ob.solve(lam * (1 + 1e-8), True)
    neighbour = _Frozen(ob)
    f, r, s = judge.backward(frozen, x, lam, True)
    assert f <= judge.kf and r <= judge.kf and s <= judge.ks
    return judge, frozen, neighbour, x, lam


def _child(frozen):
    return [c for c, p in enumerate(frozen.parent) if p >= 0][0]


def test_mutation_one_R_entry_by_2_to_minus_26(correct):
    judge, frozen, _, x, lam = correct
    c = _child(frozen)
    keep = frozen.conds[c].copy()
    try:
        frozen.conds[c][5, 9] *= 1 + 2.0 ** -26
        f, r, s = judge.backward(frozen, x, lam, True)
    finally:
        frozen.conds[c] = keep
    print(f"R entry * (1 + 2^-26): factor {f:.3g}u rhs {r:.3g}u solve {s:.3g}u")
    assert f > judge.kf


def test_mutation_one_conditional_from_the_neighbouring_lambda(correct):
    judge, frozen, neighbour, x, lam = correct
    c = _child(frozen)
    keep = frozen.conds[c]
    try:
        frozen.conds[c] = neighbour.conds[c]
        f, r, s = judge.backward(frozen, x, lam, True)
    finally:
        frozen.conds[c] = keep
    print(f"conditional at lambda (1 + 1e-8): factor {f:.3g}u rhs {r:.3g}u solve {s:.3g}u")
    assert f > judge.kf


def test_mutation_one_d_entry_by_1e_minus_10(correct):
    judge, frozen, _, x, lam = correct
    c = _child(frozen)
    keep = frozen.conds[c].copy()
    try:
        frozen.conds[c][7, -1] *= 1 + 1e-10
        f, r, s = judge.backward(frozen, x, lam, True)
    finally:
        frozen.conds[c] = keep
    print(f"d entry * (1 + 1e-10): factor {f:.3g}u rhs {r:.3g}u solve {s:.3g}u")
    assert r > judge.kf and f <= judge.kf


def test_mutation_one_structural_zero_set_to_1e_minus_30(correct):
    judge, frozen, _, x, lam = correct
    c = _child(frozen)
    keep = frozen.conds[c].copy()
    try:
        assert frozen.conds[c][9, 5] == 0.0          # below the diagonal of R
        frozen.conds[c][9, 5] = 1e-30
        f, r, s = judge.backward(frozen, x, lam, True)
    finally:
        frozen.conds[c] = keep
    print(f"structural zero = 1e-30: factor {f:.3g}u rhs {r:.3g}u solve {s:.3g}u")
    assert f == float("inf")


# ---- the vector judge ---------------------------------------------------------------------------------------------------------------
def test_vector_judge_agrees_with_the_dense_judge(correct):
    """Measures (2) and (3) summed clique by clique and factor by factor against the same two from the n x n arrays."""
    judge, frozen, _, x, lam = correct
    vj = J.VectorJudge(judge.sys.arrays, _jac_of(judge))
    assert (vj.m, vj.n, vj.kf, vj.ks) == (judge.sys.m, judge.sys.n, judge.kf, judge.ks)
    for lm, diag in [(lam, True), (0.0, False), (1e-3, False)]:
        _, r, s = judge.backward(frozen, x, lm, diag)
        rv, sv = vj.backward(frozen, x, lm, diag)
        print(f"lam {lm:g}: dense rhs {r:.6f}u solve {s:.6f}u, vector rhs {rv:.6f}u solve {sv:.6f}u")
        assert abs(rv - r) <= 1e-6 * r and abs(sv - s) <= 1e-6 * s


def _jac_of(judge):
    """The packed [A b] a judge was built from, back from its factor blocks (column-major per factor, b last)."""
    arr = judge.sys.arrays
    joff = arr.jacobian_offsets()
    jac = np.zeros(int(joff[-1]))
    blocks = iter(judge.sys.blocks)
    for f in range(arr.n_factors):
        if int(arr.f_rows[f]) == 0 or arr.f_key_ptr[f + 1] == arr.f_key_ptr[f]:
            continue
        _, Af, bf = next(blocks)
        jac[joff[f]:joff[f + 1]] = np.column_stack([Af, bf]).astype(np.float64).T.ravel()
    return jac


def test_vector_mutation_one_d_entry_by_1e_minus_10(correct):
    judge, frozen, _, x, lam = correct
    vj = J.VectorJudge(judge.sys.arrays, _jac_of(judge))
    c = _child(frozen)
    keep = frozen.conds[c].copy()
    r0, s0 = vj.backward(frozen, x, lam, True)
    assert r0 <= vj.kf and s0 <= vj.ks
    try:
        frozen.conds[c][7, -1] *= 1 + 1e-10
        r, s = vj.backward(frozen, x, lam, True)
    finally:
        frozen.conds[c] = keep
    print(f"vector judge, d entry * (1 + 1e-10): rhs {r:.3g}u solve {s:.3g}u")
    assert r > vj.kf
