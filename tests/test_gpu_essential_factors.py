"""The Unit3 and EssentialMatrix variables and the epipolar factors (GSX_F_ESSENTIAL, GSX_F_ESSENTIAL_DEPTH in both forms,
GSX_F_ESSENTIAL_CALIB, GSX_F_ESSENTIAL_CONSTRAINT; PriorFactor on both variables) on the device, through the C ABI, against
the restatements of tests/_essential_restatement.py (float64) and tests/_mp_essential_restatement.py (50 digits), which
tests/test_host_essential_factors.py pins with the reference's known answers and true derivatives.

Bounds (those of tests/test_gpu_absolute_factors.py): every [A b] block within 1e-13 max(1, max |block|) of the 50-digit
value, or, where float64 numpy itself is further away, within twice numpy's own distance — never anything taken from the
device's result; the graph error within error_bound.  Retracted states: within 1e-15 max(1, |v|) of the 50-digit state — the
angle |B v| carries a few ulp of relative error, hence a few 1.1e-16 |v| of absolute error into sin and cos, and each
component (at most 1 in magnitude) a handful of roundings more."""
import ctypes
import math

import numpy as np
import pytest

from gtsam_petercdev_amd import _abi as A
from gtsam_petercdev_amd import _lib
from tests import _absolute_restatement as SA
from tests import _essential_restatement as S
from tests import _factor_restatement as R
from tests import _mp_essential_restatement as MS
from tests.test_gpu_factor_types import backend, error_bound

pytestmark = pytest.mark.gpu
U3, ES, P3, V = S.UNIT3, S.ESSENTIAL, A.VAR_POSE3, A.VAR_VECTOR


def blocks_of(arr, flat):
    off = arr.jacobian_offsets()
    return [flat[off[f]:off[f + 1]] for f in range(arr.n_factors)]


def check_linearization(arr, what):
    be = backend(arr)
    be.linearize()
    got = be.jacobians()
    gb, worst, n_wide = blocks_of(arr, got), 0.0, 0
    for f in range(arr.n_factors):
        want = MS.linearized(arr, arr.values, f)[0].reshape(-1, order="F")
        project = 1e-13 * max(1.0, float(np.max(np.abs(want))))
        dev = float(np.max(np.abs(gb[f] - want)))
        bound = project
        if dev > project:   # how far float64 numpy itself lies from the 50-digit value on this block
            np_dist = float(np.max(np.abs(S.linearized(arr, arr.values, f)[0].reshape(-1, order="F") - want)))
            bound, n_wide = max(project, 2.0 * np_dist), n_wide + 1
        worst = max(worst, dev / project)
        assert dev <= bound, (what, f, int(arr.f_type[f]), dev, project, bound)
    scale = max(1.0, float(np.max(np.abs(got))))
    eg, ew = be.error(), MS.graph_error(arr, arr.values)
    # error_bound is the first-order term sum |r_i| d of a residual off by d = 1e-13 scale; the chart edges sit where the
    # error itself is zero, so the second-order term sum d^2 / 2 that it drops is added
    bound = error_bound(arr, scale, ew) + 0.5 * float(arr.f_rows.sum()) * (1e-13 * scale) ** 2
    print(f"{what}: {arr.n_factors} factors, worst block {worst:.2f} of its bound ({n_wide} judged by numpy's distance), error "
          f"{eg:.12g} vs {ew:.12g} (diff {abs(eg - ew):.3e}, bound {bound:.3e})")
    assert abs(eg - ew) <= bound, (eg, ew)
    be.close()
    return gb


def one(ftype, vts, m, states, z, kind=A.NOISE_UNIT, params=()):
    dims = {P3: 6, U3: 2, ES: 5}
    var_list = [(i, t, dims[t] if t != V else len(states[i])) for i, t in enumerate(vts)]
    return R.make_arrays(var_list, [(ftype, list(range(len(vts))), m, z, kind, params)], np.concatenate(states))


# ---- 1. per form and noise ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["unit", "isotropic", "diagonal", "gaussian", "huber"])
@pytest.mark.parametrize("form", S.FORMS)
def test_jacobians_and_error_match_the_50_digit_restatement(form, noise):
    """301 factors of one form: two blocks of 256 threads, the second partly filled."""
    arr, _ = S.random_graph([form], 301, noise, seed=60 + S.FORMS.index(form))
    assert arr.n_factors == 301
    check_linearization(arr, f"{form}/{noise}")


# ---- 2. all five forms in one graph -----------------------------------------------------------------------------------------
def test_mixed_forms_sorted_and_shuffled():
    sorted_arr, _ = S.random_graph(S.FACTOR_FORMS, 37, "diagonal", seed=31)
    shuffled, perm = S.random_graph(S.FACTOR_FORMS, 37, "diagonal", seed=31, shuffle=True)
    assert sorted_arr.n_factors == 37 * 5 and not np.array_equal(perm, np.arange(len(perm)))
    a = check_linearization(sorted_arr, "mixed, form order")
    b = check_linearization(shuffled, "mixed, shuffled")
    for pos, src in enumerate(perm):
        assert np.array_equal(b[pos], a[src]), (pos, src)


# ---- 3. chart edges ---------------------------------------------------------------------------------------------------------
def tie(sign):
    n = np.array([0.6, 0.6 * (1 - 2.0 ** -52), 0.5]) * sign
    return n / np.linalg.norm(n)


POINTS = {"111": np.ones(3) / math.sqrt(3.0), "z": np.array([0.0, 0.0, 1.0]), "y": np.array([0.0, 1.0, 0.0]),
          "tie": tie(1.0), "tie-": tie(-1.0)}


@pytest.mark.parametrize("norm", [0.0, 1e-17, 1e-8, math.pi, 7.0])
@pytest.mark.parametrize("name", sorted(POINTS))
def test_unit3_retract(name, norm):
    p = POINTS[name]
    v = norm * np.array([0.6, -0.8])
    arr = one(A.F_PRIOR, [U3], 2, [p], p)
    be = backend(arr)
    be.retract(v, commit=True, want_error=False)
    got = be.get_values()
    be.close()
    want = MS.retract(U3, p, v)
    assert np.max(np.abs(got - want)) <= 1e-15 * max(1.0, norm), (name, norm, got, want)


@pytest.mark.parametrize("away", [0.0, 1e-9, 1e-4, "antipode"])
@pytest.mark.parametrize("name", sorted(POINTS))
def test_unit3_local_through_a_prior(name, away):
    p = POINTS[name]
    q = -p if away == "antipode" else MS.retract(U3, p, away * np.array([0.6, -0.8]))
    arr = one(A.F_PRIOR, [U3], 2, [p], q)
    gb = check_linearization(arr, f"prior unit3 {name} {away}")
    if away == "antipode":          # b = Local(x, prior) = (pi, 0): float64 puts 1 - (p . q)^2 below epsilon at all five points
        assert 1.0 - S.dot64(p, q) ** 2 < S.EPS and np.array_equal(gb[0][4:6], [math.pi, 0.0])


@pytest.mark.parametrize("angle", [0.0, 1e-10, math.pi - 1e-7])
def test_essential_retract_and_local(angle):
    rng = np.random.default_rng(5)
    E = S.random_essential(rng)
    E[:9] = np.eye(3).reshape(9) if angle == 0.0 else E[:9]
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    xi = np.concatenate([axis * angle, [0.2, -0.1]])
    want = MS.retract(ES, E, xi)
    arr = one(A.F_PRIOR, [ES], 5, [E], want)
    be = backend(arr)
    be.retract(xi, commit=True, want_error=False)
    got = be.get_values()
    be.close()
    assert np.max(np.abs(got - want)) <= 1e-15 * max(1.0, angle), (angle, got, want)
    check_linearization(arr, f"prior essential at {angle}")     # local coordinates of the retracted point


# ---- 4. factor edges --------------------------------------------------------------------------------------------------------
def test_depth_edges_and_factor3_with_identity():
    rng = np.random.default_rng(6)
    E = S.random_essential(rng)
    z = np.array([0.3, -0.2, 1.0, 0.1, 0.05, 1.0])
    check_linearization(one(S.F_E_DEPTH, [ES, V], 2, [E, np.array([0.0])], z), "depth d = 0")
    Rm, t = S.e_of(E)
    d = 5.0
    while (Rm.T @ (z[:3] - d * t))[2] >= 0:
        d = -d * 1.5
    check_linearization(one(S.F_E_DEPTH, [ES, V], 2, [E, np.array([d])], z), "depth dP2.z < 0")
    a = check_linearization(one(S.F_E_DEPTH, [ES, V], 2, [E, np.array([0.3])], z), "factor 2")
    b = check_linearization(one(S.F_E_DEPTH, [ES, V], 2, [E, np.array([0.3])], np.concatenate([z, np.eye(3).reshape(9)])),
                            "factor 3, cRb = I")
    assert np.max(np.abs(a[0] - b[0])) <= 2e-13 * max(1.0, float(np.max(np.abs(a[0]))))


@pytest.mark.parametrize("skew", [0.0, 3.0])
def test_calib_with_and_without_skew(skew):
    rng = np.random.default_rng(8)
    K = np.array([510.0, 490.0, skew, 320.0, 240.0])
    check_linearization(one(S.F_E_CALIB, [ES, V], 1, [S.random_essential(rng), K], [400.0, 200.0, 250.0, 300.0]), f"calib {skew}")


def test_constraint_at_truth():
    rng = np.random.default_rng(3)
    x1, x2 = (R.pose3_state(S.S.big_rot3(rng), rng.normal(size=3)) for _ in range(2))
    R1, t1 = R.pose3_of(x1)
    R2, t2 = R.pose3_of(x2)
    th = R1.T @ (t2 - t1)
    z = np.concatenate([(R1.T @ R2).reshape(9), th / np.linalg.norm(th)])
    gb = check_linearization(one(S.F_E_CONSTRAINT, [P3, P3], 5, [x1, x2], z), "constraint at truth")
    assert np.max(np.abs(gb[0][60:65])) <= 1e-13


# ---- 5. the reference's minimisations (testEssentialMatrixFactor.cpp:158-200, 229-261, 388-432) ---------------------------
def check_lm_run(arr, p, what, ill_conditioned=False):
    """gsx_lm_optimize against the restated LM (tests/_absolute_restatement.restated_lm on this module's restatement): the
    project's bounds of tests/test_gpu_absolute_factors.check_lm_run — the same decisions, lambdas to 1e-9, trial errors to
    1e-8, final values to 1e-7, all relative.  These minima have a ZERO residual, where a relative bound on the error says
    nothing; so the errors BELOW 1e-6 — the last trials, six orders under the starts — get the absolute term that the 1e-7
    bound on the values itself allows: states 1e-7 max |x| apart move the whitened residual by at most
    a = 1e-7 max |x| |J|_F, hence the error 1/2 |r|^2 by sqrt(2 e) a + a^2 / 2.  Every trial above keeps the plain 1e-8.
    ill_conditioned (the Factor4 graph: five correspondences leave the calibration to a prior of sigma 10, cond(J'J) =
    2.7e13): there the float64 restated LM is itself 1.2e-8 ... 3.3e-7 relative away, trial by trial, from the same LM on the
    50-digit errors and Jacobians (measured on the host), so 1e-8 is beyond any float64 solve of these systems; each trial
    error and the final values get, on top of the project's bound, 4x the float64 restatement's own distance from the
    50-digit one on that trial — the margin rule of the [A b] blocks; nothing is taken from the device's result."""
    run = SA.restated_lm(arr, p, S.dense_system, S.graph_error, S.retract_values)
    trace, want_values, want_error = run
    spread, value_spread = [0.0] * (len(trace) + 1), 0.0
    if ill_conditioned:
        mp_trace, mp_values, mp_error = SA.restated_lm(arr, p, MS.dense_system, MS.graph_error, MS.retract_values)
        assert [t[2] for t in mp_trace] == [t[2] for t in trace]
        spread = [abs(t[0] - m[0]) for t, m in zip(trace, mp_trace)] + [abs(want_error - mp_error)]
        value_spread = float(np.max(np.abs(want_values - mp_values)))
    J, _ = S.dense_system(arr, arr.values)
    a = 1e-7 * float(np.max(np.abs(want_values))) * float(np.linalg.norm(J))
    floor = lambda e: (math.sqrt(2.0 * e) * a + 0.5 * a * a) if e < 1e-6 else 0.0
    be = backend(arr)
    res = be.lm_optimize(p)
    got_values = be.get_values()
    be.close()
    acc = [t[2] for t in trace]
    print(f"{what}: {len(trace)} trials, accepted {acc}, final error {res['final_error']:.6g} vs {want_error:.6g}")
    assert res["trace_accepted"].tolist() == acc, (what, res["trace_accepted"].tolist(), acc)
    assert np.allclose(res["trace_lambda"], [t[1] for t in trace], rtol=1e-9, atol=0), what
    for got, (want, _, _), sp in zip(res["trace_error"], trace, spread):
        print(f"  trial error {got:.12g} vs {want:.12g}: diff {abs(got - want):.3e}, float64-to-50-digit spread {sp:.3e}")
        assert abs(got - want) <= 1e-8 * want + floor(want) + 4.0 * sp, (what, got, want, sp)
    assert abs(res["final_error"] - want_error) <= 1e-8 * want_error + floor(want_error) + 4.0 * spread[-1], what
    assert np.max(np.abs(got_values - want_values)) <= 1e-7 * np.max(np.abs(want_values)) + 4.0 * value_spread, what
    return res, got_values


def lm_params():
    p = A.lm_params_legacy()        # the reference's LevenbergMarquardtParams defaults
    p.max_iterations = 100
    return p


def test_five_point_minimization():
    arr, trueE = S.two_view_graph("five")
    be = backend(arr)
    assert abs(be.error() - 643.26) <= 1e-2
    be.close()
    res, got = check_lm_run(arr, lm_params(), "five-point")
    assert 0 in res["trace_accepted"] and 1 in res["trace_accepted"]
    assert res["final_error"] < 1e-4
    assert np.max(np.abs(got - trueE)) <= 1e-1


def test_depth_minimization_on_the_18_point_data():
    arr, truth = S.two_view_graph("depth")
    assert arr.n_vars == 19 and arr.n_factors == 18
    res, got = check_lm_run(arr, lm_params(), "18-point depth")
    assert res["final_error"] < 1e-4
    assert np.max(np.abs(got - truth)) <= 1e-1          # the depths and E


def test_minimization_with_strong_cal3_s2_prior():
    arr, truth = S.two_view_graph("calib")
    res, got = check_lm_run(arr, lm_params(), "Factor4, strong prior", ill_conditioned=True)
    assert res["final_error"] < 1e-4
    assert np.max(np.abs(got[:12] - truth[:12])) <= 1e-1 and np.max(np.abs(got[12:] - truth[12:])) <= 1e-2
    Rm, t = S.e_of(got[:12])
    for f in range(5):                                   # the individual epipolar errors at the result (:425-431)
        z = R.factor_parts(arr, f)[2]
        vA, vB = (np.append(S.calibrate(got[12:], q)[0], 1.0) for q in (z[:2], z[2:]))
        assert abs(vA @ R.skew(t) @ Rm @ vB) <= 1e-6


def test_wide_essential_goes_through_the_heavy_assembly():
    """One E under 3 000 GSX_F_ESSENTIAL factors (and eight GSX_F_ESSENTIAL_CALIB ones to a calibration eliminated after it,
    without which the diagonal class takes it): the handle says its panel was assembled by a heavy class, and the panel meets the bound of
    tests/test_gpu_assembly_classes.py (the gamma_k bound of tests/_assembly_cases.judge on the handle's own [A b] blocks,
    which a float64 comparison with the restatement covers to 1e-12 of their largest entry)."""
    from tests import _assembly_cases as AC
    arr = S.wide_graph()
    assert int(np.sum(arr.f_type == S.F_E)) == 3000
    be = _lib.ProductBackend(arr)
    be.set_ordering(arr.var_keys)                        # E, then the calibration
    cls = int(be.hessian_groups()["class"][0])
    assert cls in (A.H_HEAVY, A.H_HUGE), cls
    be.linearize()
    jac = be.jacobians()
    want = S.jacobians(arr, arr.values)[0]
    assert np.max(np.abs(jac - want)) <= 1e-12 * np.max(np.abs(want))
    got, row_var, row_scalar = be.hessian_panel(int(arr.var_keys[0]))
    p = AC.expected_panel(arr, jac, 0)
    assert got.shape == p.exact.shape and np.array_equal(row_var, p.row_var) and np.array_equal(row_scalar, p.row_scalar)
    ok, worst, k = AC.judge(got, p, cls, "real")
    print(f"wide: class {AC.NAMES[cls]}, worst {worst:.2f} u against k <= {k}")
    assert ok, (worst, k)
    res = be.lm_optimize(lm_params())
    be.close()
    assert res["final_error"] < res["initial_error"]


# ---- 5b. the rest of the handle on a small view graph ----------------------------------------------------------------------
def test_view_graph_blocks_steps_and_marginals():
    arr = S.view_graph()
    check_linearization(arr, "view graph")
    be = backend(arr)
    be.linearize()
    J, b = MS.dense_system(arr, arr.values)
    H, g = J.T @ J, J.T @ b
    for lam in (0.0, 1e-3):
        want = np.linalg.solve(H + lam * np.eye(H.shape[0]), g)
        got = be.solve(lam, False)
        assert np.linalg.norm(got - want) <= 1e-6 * np.linalg.norm(want), lam
    be.solve(0.0, False)
    cov = np.linalg.inv(H)
    to = arr.tangent_offsets()
    allm = be.marginal_covariances()
    for v in range(arr.n_vars):       # the bound of tests/test_gpu_all_marginals.py as test_gpu_absolute_factors.py takes it
        d = int(arr.var_dims[v])
        assert np.max(np.abs(allm[int(arr.var_keys[v])] - cov[to[v]:to[v] + d, to[v]:to[v] + d])) <= 1e-7
        assert np.max(np.abs(be.marginal_covariance(int(arr.var_keys[v])) - cov[to[v]:to[v] + d, to[v]:to[v] + d])) <= 1e-7
    # joint marginals: two poses under a constraint edge, a pose with a free E, two free E
    for pair in ((0, 1), (2, arr.n_vars - 1), (arr.n_vars - 2, arr.n_vars - 1)):
        idx = np.concatenate([np.arange(to[v], to[v] + int(arr.var_dims[v])) for v in pair])
        joint = be.joint_marginal_covariance([int(arr.var_keys[v]) for v in pair])
        assert joint.shape == (idx.size, idx.size) and np.max(np.abs(joint - cov[np.ix_(idx, idx)])) <= 1e-7, pair
    be.close()


def test_view_graph_pcg_matches_the_direct_solve():
    arr = S.view_graph()
    be = backend(arr)
    be.linearize()
    prm = _lib.pcg_params_default()
    prm.max_iterations, prm.epsilon_rel, prm.epsilon_abs = 2000, 1e-24, 0.0
    for lam in (0.0, 1e-3):
        want = be.solve(lam, False)
        got, st = be.solve_pcg(lam, False, params=prm)
        rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
        assert st["converged"] == 1 and rel <= 1e-6, (lam, st, rel)
    be.close()


def test_view_graph_relinearize_partial_is_bit_identical():
    arr = S.view_graph()
    P, F = backend(arr, A.ORDER_ND), backend(arr, A.ORDER_ND)
    for be in (P, F):
        be.linearize()
        be.solve(0.0, False)
    F.retract(None, commit=True)
    x1 = F.get_values()
    so = arr.state_offsets()
    current = arr.values.copy()
    for round_, idx in enumerate([np.array([0, 1]), np.array([2, 6, 8]), np.arange(arr.n_vars - 3, arr.n_vars)]):
        states = np.concatenate([x1[so[i]:so[i + 1]] for i in idx])
        for i in idx:
            current[so[i]:so[i + 1]] = x1[so[i]:so[i + 1]]
        stats = P.relinearize_partial(arr.var_keys[idx], states)
        assert 0 < stats["n_fronts_reeliminated"] <= stats["n_fronts"]
        dp = P.solve(0.0, False)
        F.set_values(current)
        F.linearize()
        df = F.solve(0.0, False)
        assert np.array_equal(P.get_values(), current), round_
        assert np.array_equal(P.jacobians(), F.jacobians()), round_
        assert np.array_equal(dp, df), (round_, float(np.max(np.abs(dp - df))))
    P.close()
    F.close()


def grow(arr, keep):
    """The variables `keep` (indices, ascending) of `arr` with the factors on them alone, and the factor_origin of the
    gsx_update that grows that graph into `arr`."""
    new = {v: i for i, v in enumerate(keep)}
    so = arr.state_offsets()
    var_list = [(int(arr.var_keys[v]), int(arr.var_types[v]), int(arr.var_dims[v])) for v in keep]
    factors, origin = [], []
    for f in range(arr.n_factors):
        ftype, vs, z = R.factor_parts(arr, f)
        if all(v in new for v in vs):
            origin.append(len(factors))
            factors.append((ftype, [new[v] for v in vs], int(arr.f_rows[f]), z, int(arr.f_noise_kind[f]),
                            arr.noise[arr.f_noise_ptr[f]:arr.f_noise_ptr[f + 1]]))
        else:
            origin.append(-1)
    return R.make_arrays(var_list, factors, np.concatenate([arr.values[so[v]:so[v + 1]] for v in keep])), origin


def test_view_graph_update_adds_a_pose_and_an_essential():
    """gsx_update from the graph without the last pose and the last E to the whole of it, against a fresh handle with the
    same ordering (the bounds of tests/test_gpu_update.py); and a new E whose direction is not of unit length is refused."""
    arr = S.view_graph()
    keep = [v for v in range(arr.n_vars) if v not in (5, arr.n_vars - 1)]
    first, origin = grow(arr, keep)
    so = arr.state_offsets()
    new_values = np.concatenate([arr.values[so[5]:so[6]], arr.values[so[arr.n_vars - 1]:]])
    be = backend(first, A.ORDER_ND)
    be.linearize()
    be.solve(0.0, False)
    bad = new_values.copy()
    bad[-3:] *= 1.001
    with pytest.raises(A.GsxError, match="GSX_VAR_ESSENTIAL"):
        be.update(arr, origin, bad)
    be.close()
    be = backend(first, A.ORDER_ND)
    be.linearize()
    be.solve(0.0, False)
    st = be.update(arr, origin, new_values)
    assert st["n_factors_added"] == origin.count(-1) and st["n_vars_added"] == 2
    assert np.array_equal(be.get_values(), arr.values)
    fresh = _lib.ProductBackend(arr)
    fresh.set_ordering(be.get_ordering())
    assert abs(be.error() - fresh.error()) <= 1e-12 * abs(fresh.error())
    fresh.linearize()
    jb, jf = be.jacobians(), fresh.jacobians()
    assert np.max(np.abs(jb - jf)) <= 1e-12 * np.max(np.abs(jf))
    du, dn = be.solve(0.0, False), fresh.solve(0.0, False)
    assert np.max(np.abs(du - dn)) <= 1e-9 * np.max(np.abs(dn))
    be.close()
    fresh.close()


def test_view_graph_with_a_hard_essential_prior():
    """A GSX_NOISE_CONSTRAINED (sigma 0) Prior<EssentialMatrix>: five hard-constraint rows against a dense KKT solve of the
    restated rows (tests/test_gpu_constraints.dense_kkt_step), undamped and damped."""
    from tests.test_gpu_constraints import constraint_rows, dense_kkt_step
    arr = S.view_graph(hard_prior=True)
    con = constraint_rows(arr)
    assert len(con) == 5
    be = backend(arr)
    assert be.stats()["n_constraint_rows"] == 5
    be.linearize()
    jac = MS.jacobians(arr, arr.values)[0]
    n = int(arr.var_dims.sum())
    for lam in (0.0, 1e-3):
        want = dense_kkt_step(arr, jac, con, lam, np.ones(n))
        got = be.solve(lam, False)
        rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
        assert rel <= 1e-6, (lam, rel)
    be.close()


def test_view_graph_sharded_two_ways_over_gloo():
    """The view graph on two ranks (tests/_essential_shard_worker.py) against the single handle in the same process: error,
    Hessian diagonal, steps, an LM run — the bounds of tests/test_gpu_shard.py; between them the ranks evaluate every factor
    of the new lists."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = 29600 + (os.getpid() % 2000) + 11
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "tests", "_essential_shard_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=root)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    res = json.loads([line for line in out.stdout.splitlines() if line.startswith("{")][-1])
    assert res["world"] == 2 and len(res["ranks"]) == 2 and res["allreduce_calls"] > 0
    for r in res["ranks"]:
        assert abs(r["error0"][0] - r["error0"][1]) <= 1e-12 * abs(r["error0"][1])
        assert r["hdiag"] < 1e-12
        for s in r["steps"]:
            assert s["delta"] < 1e-9, s
            assert np.allclose(s["lin"][0], s["lin"][1], rtol=1e-10), s
            assert abs(s["trial"][0] - s["trial"][1]) <= 1e-9 * abs(s["trial"][1]), s
        run = r["lm"]
        assert run["accepted"][0] == run["accepted"][1], run
        assert abs(run["final"][0] - run["final"][1]) <= 1e-8 * abs(run["final"][1]), run
        assert run["trace"] < 1e-8 and run["values"] < 1e-7, run
    assert res["ranks"][0]["lm"] == res["ranks"][1]["lm"] and res["ranks"][0]["steps"] == res["ranks"][1]["steps"]
    owned = set(res["ranks"][0]["owned_new"]) | set(res["ranks"][1]["owned_new"])
    assert len(owned) == res["ranks"][0]["n_new"] > 0


# ---- 5c. the example ----------------------------------------------------------------------------------------------------------
def test_essential_matrix_example_end_to_end():
    """examples/EssentialMatrixExample.py: both minimisations end below 1e-4 within 1e-1 of the true E (the reference's
    tolerances), the depths within 1e-1; and the program prints them."""
    import re
    from tests.test_gpu_factor_types import run_example
    text = run_example("EssentialMatrixExample.py")
    assert "Five-point minimisation (5pointExample2.txt):" in text and "Depth minimisation (18pointExample1.txt):" in text
    finals = [float(x) for x in re.findall(r"final error ([-+0-9.eE]+)", text)]
    dists = [float(x) for x in re.findall(r"distance to the true E: ([-+0-9.eE]+)", text)]
    starts = [float(x) for x in re.findall(r"initial error ([-+0-9.eE]+),", text)]
    assert len(finals) == 2 and all(e < 1e-4 for e in finals) and len(dists) == 2 and all(d <= 1e-1 for d in dists)
    assert abs(starts[0] - 643.26) <= 1e-2      # testEssentialMatrixFactor.cpp:626
    assert float(re.search(r"largest inverse-depth error: ([-+0-9.eE]+)", text).group(1)) <= 1e-1


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def refused(arr, word):
    with pytest.raises(A.GsxError) as ei:
        _lib.ProductBackend(arr)
    assert ei.value.status == A.GSX_E_INVALID
    f = _lib.load().gsx_last_error
    f.restype = ctypes.c_char_p
    line = (f(None) or b"").decode()
    assert word in line, line


def test_refusals():
    rng = np.random.default_rng(2)
    E, u = S.random_essential(rng), S.unit(rng)
    refused(one(A.F_BETWEEN, [U3, U3], 2, [u, u], u), "GSX_VAR_UNIT3")
    refused(one(A.F_BETWEEN, [ES, ES], 5, [E, E], E), "GSX_VAR_ESSENTIAL")
    refused(one(A.F_PRIOR, [U3], 2, [u], 1.001 * u), "not of unit length")
    bad = E.copy()
    bad[9:] *= 1.001
    refused(one(A.F_PRIOR, [ES], 5, [E], bad), "not of unit length")
    x = R.pose3_state(np.eye(3), [1.0, 2.0, 3.0])
    refused(one(S.F_E_CONSTRAINT, [P3, P3], 5, [x, x], bad), "not of unit length")
    z6 = np.array([0.1, 0.2, 1.0, 0.3, 0.1, 1.0])
    refused(one(S.F_E, [U3], 1, [u], z6), "malformed factor 0")                       # wrong key type
    refused(one(S.F_E, [ES], 2, [E], z6), "malformed factor 0")                       # wrong m
    refused(one(S.F_E, [ES], 1, [E], z6[:5]), "malformed factor 0")                   # wrong measurement length
    refused(one(S.F_E_DEPTH, [ES, V], 2, [E, np.array([0.1])], z6[:5]), "malformed factor 0")
    refused(one(S.F_E_DEPTH, [ES, V], 2, [E, np.array([0.1, 0.2])], z6), "malformed factor 0")
    refused(one(S.F_E_CALIB, [ES, V], 1, [E, np.array([0.1])], z6[:4]), "malformed factor 0")
    refused(one(S.F_E_CONSTRAINT, [P3, ES], 5, [x, E], E), "malformed factor 0")
    # a state whose direction is not of unit length: gsx_set_values names the variable
    arr = one(A.F_PRIOR, [ES], 5, [bad], E)
    with pytest.raises(A.GsxError, match="GSX_VAR_ESSENTIAL"):
        _lib.ProductBackend(arr)


@pytest.mark.parametrize("vtype", [U3, ES])
def test_calls_that_read_states_by_their_own_rules_refuse_the_new_variables(vtype, tmp_path):
    """The writers, the Pose3 initializer, lago and landmark triangulation answer a description that holds a Unit3 or an
    EssentialMatrix variable with GSX_E_INVALID and a line that names the variable."""
    rng = np.random.default_rng(4)
    x = S.unit(rng) if vtype == U3 else S.random_essential(rng)
    d, name = (2, "GSX_VAR_UNIT3") if vtype == U3 else (5, "GSX_VAR_ESSENTIAL")
    pose = R.pose3_state(np.eye(3), np.zeros(3))
    arr = R.make_arrays([(5, P3, 6), (7, vtype, d)],
                        [(A.F_PRIOR, [0], 6, pose, A.NOISE_UNIT, ()), (A.F_PRIOR, [1], d, x, A.NOISE_UNIT, ())],
                        np.concatenate([pose, x]))
    f = _lib.load().gsx_last_error
    f.restype, f.argtypes = ctypes.c_char_p, [ctypes.c_void_p]
    last = lambda: (f(None) or b"").decode()
    for call_name, call in (("gsx_write_g2o", lambda: _lib.write_g2o(str(tmp_path / "a.g2o"), arr, arr.values)),
                            ("gsx_write_bal", lambda: _lib.write_bal(str(tmp_path / "a.bal"), arr, arr.values)),
                            ("gsx_save2d", lambda: _lib.save2d(str(tmp_path / "a.graph"), arr, arr.values, [1.0, 1.0, 1.0])),
                            ("gsx_initialize_pose3", lambda: _lib.initialize_pose3(arr)),
                            ("gsx_lago_initialize", lambda: _lib.lago_initialize(arr)),
                            ("gsx_triangulate_landmarks", lambda: _lib.triangulate_landmarks(arr, arr.values))):
        with pytest.raises(Exception):
            call()
        assert last().startswith(call_name + ":") and f"variable 1 (key 7) is a {name}" in last(), (call_name, last())
