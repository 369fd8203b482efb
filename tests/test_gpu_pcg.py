"""The device PCG solver (csrc/pcg.hip; include/gsx.h: gsx_solve_pcg, gsx_set_linear_solver) against the float64
restatement of the reference's loop (tests/_pcg_restatement.py), on the device's own [A b] blocks.

Bounds, per preconditioner.  The float64 restatement deviates from its 50-digit twin over all cases and configurations by
at most 6.3e-5 (x, relative in the A-norm) and 1.2e-3 (gamma_initial / gamma_final, relative) without a preconditioner and
by 6.2e-13 / 4.3e-13 with block-Jacobi (tests/test_host_pcg.py: DEV, asserted there on the CPU); the device, which sums
term lists of up to 131 terms in another order than BLAS, gets 8x that: 5.0e-4 / 9.6e-3 and 5.0e-12 / 3.4e-12.
The true preconditioned residual of the device's x, computed in numpy, must be at most threshold (1 + rho), rho = twice
the relative drift between the recursive and the true gamma that the float64 restatement shows on the same configuration.
The iteration count must be EQUAL, which is meaningful because epsilon is chosen (from the restatement alone) so that gamma
is at least 2x the threshold before the last iteration and at most 1/2 of it after (R.stop_is_decisive, asserted).
"""
import numpy as np
import pytest

from gtsam_petercdev_amd import _abi as A
from tests import _pcg_restatement as R
from tests.test_host_pcg import DEV

pytestmark = pytest.mark.gpu
BOUND = {pc: (8 * dx, 8 * dg) for pc, (dx, dg) in DEV.items()}   # preconditioner -> (x, gamma)
BATCH = 8   # kPcgBatch (csrc/kernels.h) of the default build: iterations between two reads of the done flag
_CACHE = {}


@pytest.fixture(scope="module")
def gpu():
    from gtsam_petercdev_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the HIP path has no fallback"
    return _lib


def _case(gpu, name):
    """(backend linearized at the case's values, arrays, J, rhs) — built once per case."""
    if name not in _CACHE:
        arr = R.CASES[name]()
        gb = gpu.product_backend(arr)
        gb.set_ordering(gb.compute_ordering(A.ORDER_MINDEGREE))
        gb.linearize()
        J, rhs = R.dense_system(arr, gb.jacobians())
        _CACHE[name] = (gb, arr, J, rhs)
    return _CACHE[name]


def _compare(gb, arr, J, rhs, lam, dg, prm, what, decisive=True):
    D = R.damping_vector(J, dg)
    ref = R.pcg_float64(J, rhs, arr.var_dims, lam, D, prm)
    if decisive:
        assert R.stop_is_decisive(ref), (what, "the restatement's stop is a coin toss: replace the case")
    x, st = gb.solve_pcg(lam, bool(dg), params=prm.c_params())
    BOUND_X, BOUND_GAMMA = BOUND[prm.preconditioner]
    ex = R.a_norm(J, lam, D, x - ref.x) / R.a_norm(J, lam, D, ref.x)
    eg = max(abs(st["gamma_initial"] - ref.gamma_initial) / ref.gamma_initial,
             abs(st["gamma_final"] - ref.gamma_final) / ref.gamma_final)
    print(f"{what}: k {st['iterations']} / {ref.k}, x {ex:.2e} (bound {BOUND_X:.1e}), gamma {eg:.2e} (bound {BOUND_GAMMA:.1e})")
    assert st["iterations"] == ref.k, what
    assert ex <= BOUND_X and eg <= BOUND_GAMMA, what
    assert st["threshold"] == pytest.approx(ref.threshold, rel=BOUND_GAMMA)
    assert st["converged"] == int(ref.gamma_final <= ref.threshold)
    return x, st, ref, D


@pytest.mark.parametrize("name", list(R.CASES))
@pytest.mark.parametrize("pc", [R.BLOCK_JACOBI, R.DUMMY], ids=["jacobi", "dummy"])
def test_cases_against_the_restatement(gpu, name, pc):
    gb, arr, J, rhs = _case(gpu, name)
    assert int(arr.var_dims.sum()) % 64 != 0   # tails: no case's tangent size is a multiple of 64
    for dg in (0, 1):
        for lam in R.LAMBDAS:
            D = R.damping_vector(J, dg)
            picked = R.pick_epsilon(J, rhs, arr.var_dims, lam, D, R.Params(preconditioner=pc))
            assert picked is not None, (name, pc, dg, lam, "no decisive stop: replace the case")
            prm = R.Params(500, 1, 501, picked[0], 0.0, pc)
            what = f"{name} pc {pc} diag {dg} lambda {lam:g}"
            x, st, ref, D = _compare(gb, arr, J, rhs, lam, dg, prm, what)
            rho = 2 * abs(ref.true_gamma - ref.gamma_final) / ref.gamma_final
            tg = R.true_gamma(J, rhs, arr.var_dims, lam, D, pc, x)
            print(f"   true gamma {tg:.3e}, threshold {ref.threshold:.3e}, rho {rho:.2e}")
            assert tg <= ref.threshold * (1 + rho), what
            x2, st2 = gb.solve_pcg(lam, bool(dg), params=prm.c_params())          # the same bits on every run
            assert np.array_equal(x, x2) and st == st2, what


def test_star_tangent_size_is_not_a_multiple_of_64(gpu):
    assert int(R.CASES["star130"]().var_dims.sum()) % 64 != 0


# ---- loop edges, on pose2example ---------------------------------------------------------------------------------------
def test_reset_3(gpu):
    gb, arr, J, rhs = _case(gpu, "pose2example")
    D = R.damping_vector(J, 0)
    base = R.Params(500, 1, 3, 1e-3, 0.0, R.DUMMY)
    eps, k = R.pick_epsilon(J, rhs, arr.var_dims, 1e-3, D, base, want=lambda k: k >= 4)
    _compare(gb, arr, J, rhs, 1e-3, 0, R.Params(500, 1, 3, eps, 0.0, R.DUMMY), "reset 3")


def test_max_iterations_below_k(gpu):
    gb, arr, J, rhs = _case(gpu, "pose2example")
    D = R.damping_vector(J, 0)
    eps, k = R.pick_epsilon(J, rhs, arr.var_dims, 1e-3, D, R.Params(preconditioner=R.DUMMY), want=lambda k: k >= 4)
    x, st, ref, _ = _compare(gb, arr, J, rhs, 1e-3, 0, R.Params(k - 2, 1, 501, eps, 0.0, R.DUMMY), "truncated", decisive=False)
    assert st["iterations"] == k - 2 and st["converged"] == 0


def test_min_iterations_above_k(gpu):
    gb, arr, J, rhs = _case(gpu, "pose2example")
    D = R.damping_vector(J, 0)
    eps, k = R.pick_epsilon(J, rhs, arr.var_dims, 1e-3, D, R.Params(preconditioner=R.BLOCK_JACOBI))
    x, st, ref, _ = _compare(gb, arr, J, rhs, 1e-3, 0, R.Params(500, k + 3, 501, eps, 0.0, R.BLOCK_JACOBI), "min iterations",
                             decisive=False)
    assert st["iterations"] == k + 3


@pytest.mark.parametrize("residue", [0, 1, BATCH - 1])
def test_stop_at_every_place_of_a_batch(gpu, residue):
    gb, arr, J, rhs = _case(gpu, "pose2example")
    hit = None
    for pc in (R.DUMMY, R.BLOCK_JACOBI):      # (checked on the CPU: residue 7 is met by block-Jacobi at lambda = 100, k = 7)
        for dg in (0, 1):
            for lam in (0.0, 1e-3, 1e-2, 1e-1, 1.0, 10.0, 100.0):
                picked = None if hit else R.pick_epsilon(J, rhs, arr.var_dims, lam, R.damping_vector(J, dg),
                                                         R.Params(preconditioner=pc),
                                                         want=lambda k: k % BATCH == residue and k < 30)
                # (a stop the 50-digit restatement does not share is decided by rounding alone — the unpreconditioned
                # runs at cond 7e8 are — and is no yardstick for k: such a configuration is passed over)
                if picked and R.pcg_mp(J, rhs, arr.var_dims, lam, R.damping_vector(J, dg),
                                       R.Params(500, 1, 501, picked[0], 0.0, pc)).k == picked[1]:
                    hit = (pc, dg, lam, picked)
    assert hit is not None, "no decisive stop with this residue: replace the configuration"
    pc, dg, lam, (eps, k) = hit
    x, st, ref, _ = _compare(gb, arr, J, rhs, lam, dg, R.Params(500, 1, 501, eps, 0.0, pc), f"k = {k} mod {BATCH}")
    assert st["iterations"] % BATCH == residue


def test_gamma0_zero_does_what_the_restatement_does(gpu):
    """Linearized at the optimum of a linear-factor graph: b = 0, gamma_0 = 0; with min_iterations = 1 the reference's first
    body computes 0 / 0 and returns NaNs (include/gsx.h), with min_iterations = 0 it returns zero."""
    import gtsam_petercdev_amd as gt
    g = gt.GaussianFactorGraph()
    g.add(gt.JacobianFactor(0, np.eye(2), np.zeros(2)))
    g.add(gt.JacobianFactor(0, np.eye(2), 1, -np.eye(2), np.zeros(2)))
    arr = g.to_arrays(None)
    arr.values = np.zeros(4)
    gb = gpu.product_backend(arr)
    gb.set_ordering(gb.compute_ordering(A.ORDER_NATURAL))
    gb.linearize()
    J, rhs = R.dense_system(arr, gb.jacobians())
    for min_it in (1, 0):
        prm = R.Params(500, min_it, 501, 1e-3, 1e-3, R.BLOCK_JACOBI)
        ref = R.pcg_float64(J, rhs, arr.var_dims, 0.0, np.ones(4), prm)
        x, st = gb.solve_pcg(0.0, False, params=prm.c_params())
        assert st["iterations"] == ref.k and st["gamma_initial"] == 0.0
        assert np.array_equal(np.isnan(x), np.isnan(ref.x)) and np.array_equal(np.nan_to_num(x), np.nan_to_num(ref.x))
        assert np.isnan(st["gamma_final"]) == np.isnan(ref.gamma_final)


# ---- against the direct solver -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pose2example", "pose3example", "dubrovnik-3-7"])
def test_against_the_direct_solver(gpu, name):
    arr = R.CASES[name]()
    gb = gpu.product_backend(arr)
    gb.set_ordering(gb.compute_ordering(A.ORDER_MINDEGREE))
    gb.linearize()
    J, rhs = R.dense_system(arr, gb.jacobians())
    D = R.damping_vector(J, 0)
    prm = R.Params(500, 1, 501, 1e-12, 0.0, R.BLOCK_JACOBI)
    x, st = gb.solve_pcg(1e-3, False, params=prm.c_params())
    with pytest.raises(A.GsxError) as e:       # nothing was factored: the arena-dependent query still says so
        gb.conditional(0)
    assert e.value.status == A.GSX_E_STATE
    direct = gb.solve(1e-3, False)
    fresh = gpu.product_backend(arr)
    fresh.set_ordering(fresh.compute_ordering(A.ORDER_MINDEGREE))
    fresh.linearize()
    assert np.array_equal(direct, fresh.solve(1e-3, False))
    # The residual bound, expressed through A: |x - x*|_A^2 = r' A^-1 r <= r' M^-1 r / lambda_min(M^-1 A), and r' M^-1 r <=
    # threshold (1 + rho) as in the cases above; the direct step stands in for x*, with the rounding allowance the device
    # gets everywhere (8x the restatement's own deviation) for both solves together.
    ref = R.pcg_float64(J, rhs, arr.var_dims, 1e-3, D, prm)
    rho = 2 * abs(ref.true_gamma - ref.gamma_final) / ref.gamma_final
    tg = R.true_gamma(J, rhs, arr.var_dims, 1e-3, D, R.BLOCK_JACOBI, x)
    assert tg <= ref.threshold * (1 + rho), (tg, ref.threshold, rho)
    Aden = J.T @ J + 1e-3 * np.diag(D)
    Linv = np.linalg.inv(np.linalg.cholesky(_block_diag(ref.blocks)))
    lmin = float(np.linalg.eigvalsh(Linv @ Aden @ Linv.T).min())
    dist = R.a_norm(J, 1e-3, D, x - direct)
    bound = np.sqrt(ref.threshold * (1 + rho) / lmin) + BOUND[R.BLOCK_JACOBI][0] * R.a_norm(J, 1e-3, D, direct)
    print(f"{name}: |pcg - direct|_A {dist:.3e}, bound {bound:.3e} (lambda_min(M^-1 A) {lmin:.3e}, rho {rho:.2e})")
    assert dist <= bound


def _block_diag(blocks):
    """M = blockdiag(L_v L_v')."""
    n = sum(L.shape[0] for L in blocks)
    M, o = np.zeros((n, n)), 0
    for L in blocks:
        d = L.shape[0]
        M[o:o + d, o:o + d] = L @ L.T
        o += d
    return M


def test_pcg_between_a_factorization_and_its_users(gpu):
    """gsx_solve(lambda1), gsx_solve_pcg(lambda2), then the users of the resident factorization: the conditionals are the
    same bits, and a solve at lambda1 gives the same step as before."""
    arr = R.CASES["pose3example"]()
    gb = gpu.product_backend(arr)
    gb.set_ordering(gb.compute_ordering(A.ORDER_MINDEGREE))
    gb.linearize()
    first = gb.solve(1e-3, True)
    n_fronts = len(gb.get_tree()[0])
    before = [gb.conditional(f) for f in range(n_fronts)]
    gb.solve_pcg(10.0, False, params=R.Params(500, 1, 501, 1e-6, 0.0, R.BLOCK_JACOBI).c_params())
    for f in range(n_fronts):
        assert np.array_equal(gb.conditional(f), before[f]), f
    assert np.array_equal(gb.solve(1e-3, True), first)
    cov = gb.marginal_covariance(arr.var_keys[1])
    fresh = gpu.product_backend(arr)
    fresh.set_ordering(fresh.compute_ordering(A.ORDER_MINDEGREE))
    fresh.linearize()
    assert np.array_equal(cov, fresh.marginal_covariance(arr.var_keys[1]))


# ---- drivers -----------------------------------------------------------------------------------------------------------------
def _lm_pair(gpu, arr, params, pcg):
    out = []
    for kind in (A.SOLVER_MULTIFRONTAL, A.SOLVER_PCG):
        gb = gpu.product_backend(arr)
        gb.set_ordering(gb.compute_ordering(A.ORDER_MINDEGREE))
        if kind == A.SOLVER_PCG:
            gb.set_linear_solver(kind, pcg)
        out.append((gb, gb.lm_optimize(params)))
    return out


@pytest.mark.parametrize("name", ["pose2example", "pose3example", "dubrovnik-3-7"])
@pytest.mark.parametrize("which", ["legacy", "ceres"])
def test_lm_with_pcg_follows_the_multifrontal_trace(gpu, name, which):
    arr = R.CASES[name]()
    params = A.lm_params_legacy() if which == "legacy" else A.lm_params_ceres()
    pcg = R.Params(500, 1, 501, 1e-10, 0.0, R.BLOCK_JACOBI).c_params()
    (gd, rd), (gp, rp) = _lm_pair(gpu, arr, params, pcg)
    assert rp["trace_accepted"].tolist() == rd["trace_accepted"].tolist()
    assert rp["iterations"] == rd["iterations"]
    assert abs(rp["final_error"] - rd["final_error"]) <= 1e-8 * abs(rd["final_error"])
    assert rp["pcg_iterations"] > 0 and rd["pcg_iterations"] == 0
    assert gp.stats()["n_pcg_iterations"] == rp["pcg_iterations"] and gp.stats()["n_pcg_solves"] == len(rp["trace_accepted"])


@pytest.mark.parametrize("name", ["pose2example", "pose3example"])
def test_gauss_newton_with_pcg(gpu, name):
    arr = R.CASES[name]()
    res = []
    for kind in (A.SOLVER_MULTIFRONTAL, A.SOLVER_PCG):
        gb = gpu.product_backend(arr)
        gb.set_ordering(gb.compute_ordering(A.ORDER_MINDEGREE))
        if kind == A.SOLVER_PCG:
            gb.set_linear_solver(kind, R.Params(500, 1, 501, 1e-10, 0.0, R.BLOCK_JACOBI).c_params())
        res.append(gb.gn_optimize())
    assert res[1]["iterations"] == res[0]["iterations"]
    assert abs(res[1]["final_error"] - res[0]["final_error"]) <= 1e-8 * abs(res[0]["final_error"])
    assert res[1]["pcg_iterations"] > 0


@pytest.mark.parametrize("which", ["legacy", "ceres"])
def test_lm_trial_and_lm_iterate_with_pcg(gpu, which):
    """gsx_lm_trial and gsx_lm_iterate on a PCG handle (ceres: diagonal damping, whose weights need the H panels the PCG
    path otherwise never assembles) against the multifrontal handle: the same numbers to 1e-8."""
    arr = R.CASES["pose3example"]()
    params = A.lm_params_legacy() if which == "legacy" else A.lm_params_ceres()
    diag = bool(params.diagonal_damping)
    out = []
    for kind in (A.SOLVER_MULTIFRONTAL, A.SOLVER_PCG):
        gb = gpu.product_backend(arr)
        gb.set_ordering(gb.compute_ordering(A.ORDER_MINDEGREE))
        if kind == A.SOLVER_PCG:
            gb.set_linear_solver(kind, R.Params(500, 1, 501, 1e-10, 0.0, R.BLOCK_JACOBI).c_params())
        trial = gb.lm_trial(True, 1e-2, diag)
        again = gb.lm_trial(False, 1.0, diag)          # same linearization, another lambda
        gb.lm_reset(params)
        it = [gb.lm_iterate(params) for _ in range(2)]
        out.append((trial, again, it, gb.stats()["n_pcg_solves"]))
    (t0, a0, i0, n0), (t1, a1, i1, n1) = out
    for want, got in list(zip(t0 + a0, t1 + a1)) + [(w[0], g[0]) for w, g in zip(i0, i1)]:
        assert abs(got - want) <= 1e-8 * abs(want), (want, got)
    # (the next lambda is a continuous function of the gain ratio under the ceres rule: the same decisions, not the same bits)
    for (_, want), (_, got) in zip(i0, i1):
        assert abs(got - want) <= 1e-8 * abs(want), (want, got)
    assert n0 == 0 and n1 >= 4


def test_python_route(gpu):
    import gtsam_petercdev_amd as gt
    arr = R.CASES["pose2example"]()
    values = gt.Values.unpack(arr.var_keys, arr.var_types, arr.var_dims, arr.values)

    class _Graph:                       # the lowered arrays stand in for the graph they were read from
        def to_arrays(self, v):
            return arr
    pcg = gt.PCGSolverParameters(gt.BlockJacobiPreconditionerParameters())
    pcg.setEpsilon_rel(1e-10)
    pcg.setEpsilon_abs(0.0)
    p = gt.LevenbergMarquardtParams()
    p.linearSolverType, p.iterativeParams = "ITERATIVE", pcg
    opt = gt.LevenbergMarquardtOptimizer(_Graph(), values, p)
    opt.optimize()
    (gd, rd), (gp, rp) = _lm_pair(gpu, arr, A.lm_params_legacy(), pcg.c_params())
    assert opt.result["final_error"] == rp["final_error"] and opt.result["pcg_iterations"] == rp["pcg_iterations"] > 0


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    arr = R.CASES["pose2example"]()
    gb = gpu.product_backend(arr)
    gb.set_ordering(gb.compute_ordering(A.ORDER_MINDEGREE))
    with pytest.raises(A.GsxError) as e:
        gb.solve_pcg()
    assert e.value.status == A.GSX_E_STATE            # not linearized
    gb.set_linear_solver(A.SOLVER_PCG)
    with pytest.raises(A.GsxError) as e:
        gb.dogleg_optimize()
    assert e.value.status == A.GSX_E_STATE and "PCG" in str(e.value)
    con = arr.with_factor(A.F_PRIOR, [1], 3, arr.values[3:6], A.NOISE_CONSTRAINED, [0.0, 0.0, 0.0, 1000.0, 1000.0, 1000.0])
    gc = gpu.product_backend(con)
    gc.set_ordering(gc.compute_ordering(A.ORDER_MINDEGREE))
    gc.linearize()
    with pytest.raises(A.GsxError) as e:
        gc.solve_pcg()
    assert e.value.status == A.GSX_E_STATE and "constraint" in str(e.value)


@pytest.mark.parametrize("pc", [R.BLOCK_JACOBI, R.DUMMY], ids=["jacobi", "dummy"])
def test_dimension_cap_is_refused_for_both_preconditioners(gpu, pc):
    """A VECTOR(33) variable is beyond the 32 the kernels' per-wave LDS arrays hold: GSX_E_INVALID, not a launch; VECTOR(32)
    is served."""
    import gtsam_petercdev_amd as gt
    rng = np.random.default_rng(3)
    for d, ok in ((32, True), (33, False)):
        g = gt.GaussianFactorGraph()
        g.add(gt.JacobianFactor(0, np.eye(d) + 0.1 * rng.normal(size=(d, d)), rng.normal(size=d)))
        g.add(gt.JacobianFactor(0, rng.normal(size=(2, d)), 1, rng.normal(size=(2, 2)), rng.normal(size=2)))
        g.add(gt.JacobianFactor(1, np.eye(2), rng.normal(size=2)))
        arr = g.to_arrays(None)
        arr.values = np.zeros(d + 2)
        gb = gpu.product_backend(arr)
        gb.set_ordering(gb.compute_ordering(A.ORDER_NATURAL))
        gb.linearize()
        prm = R.Params(500, 1, 501, 1e-8, 0.0, pc)
        if ok:
            J, rhs = R.dense_system(arr, gb.jacobians())
            ref = R.pcg_float64(J, rhs, arr.var_dims, 1e-3, np.ones(d + 2), prm)
            x, st = gb.solve_pcg(1e-3, False, params=prm.c_params())
            assert st["converged"] == 1 and ref.gamma_final <= ref.threshold
            assert R.true_gamma(J, rhs, arr.var_dims, 1e-3, np.ones(d + 2), pc, x) <= 2 * ref.threshold
        else:
            with pytest.raises(A.GsxError) as e:
                gb.solve_pcg(1e-3, False, params=prm.c_params())
            assert e.value.status == A.GSX_E_INVALID and "32" in str(e.value)


def test_indeterminate_names_the_variable(gpu):
    """A variable that only a zero Jacobian touches, at lambda = 0: its diagonal block has no Cholesky factor."""
    import gtsam_petercdev_amd as gt
    g = gt.GaussianFactorGraph()
    g.add(gt.JacobianFactor(0, np.eye(2), np.ones(2)))
    g.add(gt.JacobianFactor(0, np.eye(2), 1, np.zeros((2, 3)), np.ones(2)))
    arr = g.to_arrays(None)
    arr.values = np.zeros(5)
    gb = gpu.product_backend(arr)
    gb.set_ordering(gb.compute_ordering(A.ORDER_NATURAL))
    gb.linearize()
    with pytest.raises(A.IndeterminantLinearSystemException) as e:
        gb.solve_pcg(0.0, False)
    assert e.value.key == 1
    x, st = gb.solve_pcg(1.0, False)                 # damped: fine again, the handle is still usable
    assert st["converged"] == 1 and np.all(np.isfinite(x))
