"""The Rot3 variable and the absolute-measurement factors (GSX_F_GPS, GSX_F_POSE_TRANSLATION_PRIOR, GSX_F_POSE_ROTATION_PRIOR,
GSX_F_ATTITUDE, GSX_F_MAG; PriorFactor / BetweenFactor on Rot3) on the device, through the C ABI, against the restatements
of tests/_absolute_restatement.py (float64) and tests/_mp_absolute_restatement.py (50 digits), which
tests/test_host_absolute_factors.py pins with the reference's known answers and true derivatives.

Bounds (the project's, tests/test_gpu_sensor_factors.py): every [A b] block within 1e-13 max(1, max |block|) of the
50-digit value, or, where float64 numpy itself is further away, within twice numpy's own distance — never anything taken from
the device's result; the graph error within error_bound; steps within 1e-6 relative of a dense solve of the restated normal
equations; marginal blocks within 1e-7."""
import ctypes
import math

import numpy as np
import pytest

from gtsam_petercdev_amd import _abi as A
from gtsam_petercdev_amd import _lib
from gtsam_petercdev_amd import graph as G
from tests import _absolute_restatement as S
from tests import _factor_restatement as R
from tests import _mp_absolute_restatement as MS
from tests.test_gpu_factor_types import backend, error_bound, run_example

pytestmark = pytest.mark.gpu
P2, P3, V, ROT3 = A.VAR_POSE2, A.VAR_POSE3, A.VAR_VECTOR, S.ROT3


def blocks_of(arr, flat):
    off = arr.jacobian_offsets()
    return [flat[off[f]:off[f + 1]] for f in range(arr.n_factors)]


def check_blocks(arr, got, what):
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
    print(f"{what}: worst |[A b] - 50-digit| = {worst:.2f} of the per-block bound; {n_wide} blocks judged by numpy's distance")
    return gb


def check_linearization(arr, what):
    be = backend(arr)
    be.linearize()
    got = be.jacobians()
    gb = check_blocks(arr, got, what)
    scale = max(1.0, float(np.max(np.abs(got))))
    eg, ew = be.error(), MS.graph_error(arr, arr.values)
    print(f"{what}: {arr.n_factors} factors, error {eg:.12g} vs {ew:.12g} (diff {abs(eg - ew):.3e}, bound "
          f"{error_bound(arr, scale, ew):.3e})")
    assert abs(eg - ew) <= error_bound(arr, scale, ew), (eg, ew)
    be.close()
    return gb


# ---- 1. per form and noise ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["unit", "isotropic", "diagonal", "gaussian", "huber"])
@pytest.mark.parametrize("form", S.FORMS)
def test_jacobians_and_error_match_the_50_digit_restatement(form, noise):
    """301 factors of one form: two blocks of 256 threads, the second partly filled; rotations of 1 to 2.5 rad."""
    arr, _ = S.random_graph([form], 301, noise, seed=80 + S.FORMS.index(form))
    assert arr.n_factors == 301
    check_linearization(arr, f"{form}/{noise}")


# ---- 2. the mixed TL_ABSOLUTE list ------------------------------------------------------------------------------------------
def test_mixed_absolute_list_sorted_and_shuffled():
    """Every sub-kind of the one list, 37 factors each (every wave boundary inside a kind, most kind boundaries inside a
    wave), once in sub-kind order and once shuffled in the graph: both match the restatement block for block, and the
    device's blocks of corresponding factors are identical."""
    sorted_arr, _ = S.random_graph(S.ABSOLUTE_FORMS, 37, "diagonal", seed=31)
    shuffled, perm = S.random_graph(S.ABSOLUTE_FORMS, 37, "diagonal", seed=31, shuffle=True)
    assert sorted_arr.n_factors == 37 * 11 and not np.array_equal(perm, np.arange(len(perm)))
    a = check_linearization(sorted_arr, "mixed, sub-kind order")
    b = check_linearization(shuffled, "mixed, shuffled")
    for pos, src in enumerate(perm):
        assert np.array_equal(b[pos], a[src]), (pos, src)


# ---- 3. kernel edges --------------------------------------------------------------------------------------------------------
def one(ftype, vts, m, states, z, kind=A.NOISE_UNIT, params=()):
    dims = {P2: 3, P3: 6, ROT3: 3, V: 3}
    var_list = [(i, t, dims[t]) for i, t in enumerate(vts)]
    return R.make_arrays(var_list, [(ftype, list(range(len(vts))), m, z, kind, params)], np.concatenate(states))


def axis_angle(axis, angle):
    return R.so3_expmap(np.asarray(axis, float) / np.linalg.norm(axis) * angle)


def test_attitude_edges():
    """R b equal to nRef, opposite to it and 1e-9 rad from both; nRef along each axis and at the three ties of
    CalculateBestAxis."""
    rng = np.random.default_rng(9)
    refs = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 2), (2, 1, 1), (1, 2, 1), (1, 1, 1)]
    for ref in refs:
        n = np.array(ref, float) / np.linalg.norm(ref)
        Rm = S.big_rot3(rng)
        perp = np.cross(n, [0.3, -0.5, 0.8])
        for flip in (1.0, -1.0):
            for tilt in (0.0, 1e-9):
                q = axis_angle(perp, tilt) @ (flip * n)
                b = Rm.T @ q
                b /= np.linalg.norm(b)
                z = np.concatenate([n, b])
                check_linearization(one(S.F_ATT, [ROT3], 2, [Rm.reshape(9)], z), f"attitude rot3 {ref} {flip} {tilt}")
                check_linearization(one(S.F_ATT, [P3], 2, [R.pose3_state(Rm, [1.0, -2.0, 3.0])], z, A.NOISE_ISOTROPIC, [0.25]),
                                    f"attitude pose3 {ref} {flip} {tilt}")


@pytest.mark.parametrize("angle", [0.0, 1e-10, math.pi - 1e-7])
def test_rot3_between_and_prior_edges(angle):
    rng = np.random.default_rng(10)
    R1 = S.big_rot3(rng)
    R2 = R1 @ axis_angle([0.3, -0.5, 0.8], angle)
    check_linearization(one(A.F_PRIOR, [ROT3], 3, [R1.reshape(9)], R2.reshape(9)), f"prior rot3 at {angle}")
    check_linearization(one(A.F_BETWEEN, [ROT3, ROT3], 3, [R1.reshape(9), R2.reshape(9)], np.eye(3).reshape(9)),
                        f"between rot3 at {angle}")
    check_linearization(one(S.F_ROT, [P3], 3, [R.pose3_state(R2, [1.0, 2.0, 3.0])], R1.reshape(9)), f"rotation prior at {angle}")


@pytest.mark.parametrize("d", [math.pi - 1e-12, -math.pi + 1e-12])
def test_pose2_rotation_prior_at_the_wrap(d):
    check_linearization(one(S.F_ROT, [P2], 1, [np.array([1.0, 2.0, 0.4 + d])], [0.4]), f"rot2 prior at {d}")


def test_gps_with_and_without_arm_side_by_side():
    """The two single-key forms are told apart by the length of the measurement."""
    rng = np.random.default_rng(12)
    var_list, values, factors = [], [], []
    for i in range(40):
        x = S.random_state(rng, P3)
        var_list.append((i, P3, 6))
        values.append(x)
        form = "gps_arm" if i % 2 else "gps"
        factors.append((S.F_GPS, [i], 3, S.random_meas(rng, form, [x]), A.NOISE_ISOTROPIC, [0.5]))
    arr = R.make_arrays(var_list, factors, np.concatenate(values))
    assert sorted({int(arr.f_meas_ptr[f + 1] - arr.f_meas_ptr[f]) for f in range(40)}) == [3, 6]
    check_linearization(arr, "gps | gps arm interleaved")


# ---- 4. testRot3Optimization.cpp --------------------------------------------------------------------------------------------
def test_rot3_optimization_circle():
    """gtsam/slam/tests/testRot3Optimization.cpp: six rotations about z at multiples of 2 pi / 6, a prior on the first,
    BetweenFactor<Rot3> of Rz(2 pi / 6) around the circle, started 0.1 rad off; Gauss-Newton recovers the truth to 1e-5."""
    fg, truth, initial = G.NonlinearFactorGraph(), G.Values(), G.Values()
    model = G.noiseModel.Unit.Create(3)
    fg.add(G.PriorFactorRot3(0, G.Rot3(), model))
    step = 2.0 * math.pi / 6.0
    for j in range(6):
        truth.insert(j, G.Rot3.RzRyRx(0.0, 0.0, step * j))
        initial.insert(j, G.Rot3.RzRyRx(0.0, 0.0, step * j + 0.1 * (j % 2)))
        fg.add(G.BetweenFactorRot3(j, (j + 1) % 6, G.Rot3.RzRyRx(0.0, 0.0, step), model))
    be = backend(fg.to_arrays(initial))
    res = be.gn_optimize(max_iterations=100)
    final = G.Values.unpack(truth.keys(), [ROT3] * 6, [3] * 6, be.get_values())
    be.close()
    assert res["final_error"] < 1e-12, res
    for j in range(6):
        assert np.allclose(final.atRot3(j).matrix(), truth.atRot3(j).matrix(), atol=1e-5), j


# ---- 5. Rot3 through the layers, and a pose chain with every absolute factor ------------------------------------------------
def test_rot3_through_solve_retract_and_marginals():
    arr = S.rot3_graph()
    check_linearization(arr, "rot3 graph")
    be = backend(arr)
    be.linearize()
    J, b = MS.dense_system(arr, arr.values)
    H, g = J.T @ J, J.T @ b
    want = np.linalg.solve(H, g)
    got = be.solve(0.0, False)
    assert np.linalg.norm(got - want) <= 1e-6 * np.linalg.norm(want)
    cov = np.linalg.inv(H)
    to = arr.tangent_offsets()
    for v in (0, 17, 39):
        blk = be.marginal_covariance(int(arr.var_keys[v]))
        assert np.max(np.abs(blk - cov[to[v]:to[v] + 3, to[v]:to[v] + 3])) <= 1e-7
    allm = be.marginal_covariances()
    for v in range(arr.n_vars):
        assert np.max(np.abs(allm[int(arr.var_keys[v])] - cov[to[v]:to[v] + 3, to[v]:to[v] + 3])) <= 1e-7
    be.solve(0.0, False)
    be.retract(commit=True, want_error=False)
    moved = be.get_values()
    want_values = MS.retract_values(arr, arr.values, got)
    assert np.max(np.abs(moved - want_values)) <= 1e-14 * 10      # one 3 x 3 product of entries <= 1: a few ulp
    be.close()


def test_pose_chain_with_every_absolute_factor():
    """60 poses: betweens, a GPS fix every third pose, attitude on every pose, a robust magnetometer on every fifth, one
    translation and one rotation prior.  Blocks, error, the damped steps against a dense solve, marginals; and LM lowers
    the error to what the restated Gauss-Newton system calls a minimum."""
    arr = S.chain_graph()
    check_linearization(arr, "pose chain")
    be = backend(arr)
    be.linearize()
    J, b = MS.dense_system(arr, arr.values)
    H, g = J.T @ J, J.T @ b
    for lam in (0.0, 1e-3):
        want = np.linalg.solve(H + lam * np.eye(H.shape[0]), g)
        got = be.solve(lam, False)
        assert np.linalg.norm(got - want) <= 1e-6 * np.linalg.norm(want), lam
    cov = np.linalg.inv(H)
    to = arr.tangent_offsets()
    be.solve(0.0, False)
    for v in (0, 31, 59):
        assert np.max(np.abs(be.marginal_covariance(int(arr.var_keys[v])) - cov[to[v]:to[v] + 6, to[v]:to[v] + 6])) <= 1e-7
    be.close()


def subgraph(arr, n_vars):
    """The first n_vars variables of `arr` with the factors that touch only them; and, per factor of `arr`, its index in
    that graph (-1: not in it) — the factor_origin of the gsx_update that grows the one into the other."""
    so = arr.state_offsets()
    var_list = [(int(arr.var_keys[v]), int(arr.var_types[v]), int(arr.var_dims[v])) for v in range(n_vars)]
    factors, origin = [], []
    for f in range(arr.n_factors):
        ftype, vs, z = R.factor_parts(arr, f)
        if max(vs) < n_vars:
            origin.append(len(factors))
            factors.append((ftype, vs, int(arr.f_rows[f]), z, int(arr.f_noise_kind[f]),
                            arr.noise[arr.f_noise_ptr[f]:arr.f_noise_ptr[f + 1]]))
        else:
            origin.append(-1)
    return R.make_arrays(var_list, factors, arr.values[:so[n_vars]]), origin


# the project's bounds of an LM run against its restatement (tests/test_gpu_boundary.py, tests/test_gpu_shard.py): the same
# decisions, lambdas to 1e-9, trial errors to 1e-8, final values to 1e-7, all relative
def check_lm_run(arr, p, what):
    trace, want_values, want_error = S.restated_lm(arr, p)
    be = backend(arr)
    res = be.lm_optimize(p)
    got_values = be.get_values()
    be.close()
    acc = [t[2] for t in trace]
    print(f"{what}: {len(trace)} trials, accepted {acc}, final error {res['final_error']:.12g} vs {want_error:.12g}")
    assert res["trace_accepted"].tolist() == acc, (what, res["trace_accepted"].tolist(), acc)
    assert np.allclose(res["trace_lambda"], [t[1] for t in trace], rtol=1e-9, atol=0), what
    assert np.allclose(res["trace_error"], [t[0] for t in trace], rtol=1e-8, atol=0), what
    assert abs(res["final_error"] - want_error) <= 1e-8 * want_error, what
    assert np.max(np.abs(got_values - want_values)) <= 1e-7 * np.max(np.abs(want_values)), what
    return acc


def test_pose_chain_lm_trace_and_final_values_match_the_restated_lm():
    """The accept / reject trace, the lambdas, the trial errors and the final values of gsx_lm_optimize on the 60-pose chain
    against tests/_absolute_restatement.restated_lm (dense numpy): the default policy from the chain's start, where every
    trial is taken; the Ceres-style policy (diagonal damping); and a start ten times as far off under a model-fidelity
    threshold of 0.9, where trials are rejected and lambda climbs before it falls."""
    p = A.lm_params_legacy()
    p.max_iterations = 30
    assert all(check_lm_run(S.chain_graph(), p, "chain, legacy"))
    q = A.lm_params_ceres()
    q.max_iterations = 30
    check_lm_run(S.chain_graph(), q, "chain, ceres")
    p.min_model_fidelity = 0.9
    acc = check_lm_run(S.chain_graph(spread=10.0), p, "chain from afar, fidelity 0.9")
    assert 0 in acc and 1 in acc


def test_pose_chain_with_a_hard_gps_fix():
    """The chain with a zero-sigma GPS fix on pose 0 — three hard-constraint rows through the constraint path — against a
    dense KKT solve of the restated rows (tests/test_gpu_constraints.dense_kkt_step), undamped and damped."""
    from tests.test_gpu_constraints import constraint_rows, dense_kkt_step
    arr = S.chain_graph(hard_gps=True)
    con = constraint_rows(arr)
    assert [(f, r) for f, r, _ in con] == [(int(np.flatnonzero(arr.f_type == S.F_GPS)[0]), r) for r in range(3)]
    check_linearization(arr, "chain, hard GPS fix")
    be = backend(arr)
    assert be.stats()["n_constraint_rows"] == 3
    be.linearize()
    jac = MS.jacobians(arr, arr.values)[0]
    n = int(arr.var_dims.sum())
    for lam in (0.0, 1e-3):
        want = dense_kkt_step(arr, jac, con, lam, np.ones(n))
        got = be.solve(lam, False)
        rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
        print(f"hard GPS fix: lambda {lam:g}, |step - KKT| / |KKT| = {rel:.3e}")
        assert rel <= 1e-6, (lam, rel)
        # the step satisfies the fix to first order: t_0 + R_0 v_0 = nT
        f0 = con[0][0]
        Ab = MS.linearized(arr, arr.values, f0)[0]
        assert np.max(np.abs(Ab[:, :6] @ got[:6] - Ab[:, 6])) <= 1e-9 * max(1.0, float(np.max(np.abs(Ab))))
    be.close()


def test_pose_chain_sharded_two_ways_over_gloo():
    """The chain on two ranks (tests/_absolute_shard_worker.py, as tests/test_gpu_shard.py runs its worker) against the
    single handle in the same process: error, Hessian diagonal, steps, an LM run — the bounds of tests/test_gpu_shard.py."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = 29600 + (os.getpid() % 2000) + 7
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "tests", "_absolute_shard_worker.py")]
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
    # between them the ranks evaluate every absolute factor (upload_factor_lists with the owned mask, the list re-sorted)
    owned = set(res["ranks"][0]["owned_absolute"]) | set(res["ranks"][1]["owned_absolute"])
    assert len(owned) == res["ranks"][0]["n_absolute"] > 0


# ---- 5b. the incremental paths ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["rot3", "chain"])
def test_pcg_matches_the_direct_solve(which):
    """gsx_solve_pcg (block-Jacobi, run to a relative gamma of 1e-24: a residual of 1e-12) against gsx_solve on the same
    handle: 1e-6 relative, the step bound."""
    arr = S.rot3_graph() if which == "rot3" else S.chain_graph()
    be = backend(arr)
    be.linearize()
    prm = _lib.pcg_params_default()
    prm.max_iterations, prm.epsilon_rel, prm.epsilon_abs = 2000, 1e-24, 0.0
    for lam in (0.0, 1e-3):
        want = be.solve(lam, False)
        got, st = be.solve_pcg(lam, False, params=prm)
        rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
        print(f"{which}: lambda {lam:g}, PCG {st['iterations']} iterations, |pcg - direct| / |direct| = {rel:.3e}")
        assert st["converged"] == 1 and rel <= 1e-6, (which, lam, st, rel)
    be.close()


@pytest.mark.parametrize("which", ["rot3", "chain"])
def test_relinearize_partial_is_bit_identical_to_the_full_path(which):
    """gsx_relinearize_partial moves a few variables (Rot3 states; poses that carry GPS, attitude, magnetometer and the
    pose-part priors) and redoes only their factors and cliques: [A b] and the step are the bits of a full linearize and
    solve at the same values."""
    arr = S.rot3_graph() if which == "rot3" else S.chain_graph()
    P, F = backend(arr, A.ORDER_ND), backend(arr, A.ORDER_ND)
    for be in (P, F):
        be.linearize()
        be.solve(0.0, False)
    F.retract(None, commit=True)
    x1 = F.get_values()
    so = arr.state_offsets()
    current = arr.values.copy()
    rng = np.random.default_rng(3)
    for round_, idx in enumerate([np.array([0, 1]), np.sort(rng.choice(arr.n_vars, 6, replace=False)),
                                  np.arange(arr.n_vars - 4, arr.n_vars)]):
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


@pytest.mark.parametrize("which", ["rot3", "chain"])
def test_update_grows_a_graph_with_the_new_types(which):
    """gsx_update from the first three quarters of the graph to the whole of it (new Rot3 variables; new poses with their
    absolute factors) against a fresh handle on the whole graph with the same ordering: the bounds of
    tests/test_gpu_update.py — error 1e-12, [A b] 1e-12 of its largest entry, step 1e-9, all relative."""
    arr = S.rot3_graph() if which == "rot3" else S.chain_graph()
    n0 = (3 * arr.n_vars) // 4
    first, origin = subgraph(arr, n0)
    assert first.n_factors < arr.n_factors and -1 in origin
    so = arr.state_offsets()
    be = backend(first, A.ORDER_ND)
    be.linearize()
    be.solve(0.0, False)
    st = be.update(arr, origin, arr.values[so[n0]:])
    assert st["n_factors_added"] == origin.count(-1) and st["n_vars_added"] == arr.n_vars - n0
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


# ---- 5c. the example ------------------------------------------------------------------------------------------------------------
def test_gps_factor_example_end_to_end():
    """examples/GPSFactorExample.py: a prior at the origin (sigma 0.25) and one GPS fix (sigma 0.1) on one pose.  The
    optimizer's trace and result against the restated LM; the rotation stays the identity (the GPS Jacobian has no rotation
    columns, the prior pulls nothing), the translation is the weighted mean of the origin and the fix; and the program prints
    what the reference's prints: the graph, the initial estimate, the final result."""
    import GPSFactorExample as ex
    graph, initial = ex.build()
    arr = graph.to_arrays(initial)
    assert arr.f_type.tolist() == [A.F_PRIOR, S.F_GPS] and arr.var_types.tolist() == [P3]
    p = G.LevenbergMarquardtParams().c_params()
    check_lm_run(arr, p, "GPSFactorExample")
    result = G.LevenbergMarquardtOptimizer(graph, initial, G.LevenbergMarquardtParams()).optimize()
    pose = result.atPose3(1)
    w_prior, w_gps = 1.0 / 0.25 ** 2, 1.0 / 0.1 ** 2
    want_t = w_gps * np.array([ex.lat0, ex.lon0, ex.h0]) / (w_prior + w_gps)
    assert np.max(np.abs(pose.rotation().matrix() - np.eye(3))) <= 1e-12
    assert np.max(np.abs(pose.translation() - want_t)) <= 1e-7 * np.max(np.abs(want_t))
    text = run_example("GPSFactorExample.py")
    for piece in ("Factor Graph:", "NonlinearFactorGraph: size: 2", "PriorFactor on 1", "GPSFactor on 1",
                  "GPS measurement:    33.87 -84.3063      274", "Initial Estimate:", "Values with 1 values:",
                  "Value 1: (gtsam::Pose3)", "Final Result:"):
        assert piece in text, (piece, text)
    import re
    t = re.findall(r"t: ([-+0-9.eE]+) ([-+0-9.eE]+) ([-+0-9.eE]+)", text)
    # the prior mean inside the graph, the initial estimate, the result
    assert len(t) == 3 and np.allclose([[float(x) for x in row] for row in t[:2]], 0.0)
    assert np.allclose([float(x) for x in t[2]], want_t, rtol=1e-5)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def last_call_error():
    lib = _lib.load()
    lib.gsx_last_error.restype = ctypes.c_char_p
    lib.gsx_last_error.argtypes = [ctypes.c_void_p]
    return (lib.gsx_last_error(None) or b"").decode()


def create_status(arr):
    """gsx_last_error(NULL) after gsx_create refused `arr`; "" when it took it."""
    try:
        be = _lib.ProductBackend(arr)
    except A.GsxError as ex:
        assert ex.status == A.GSX_E_INVALID
        return last_call_error()
    be.close()
    return ""


def test_malformed_absolute_factors_are_refused():
    x3, x2, xr = R.pose3_state(np.eye(3), [1.0, 2.0, 3.0]), np.array([1.0, 2.0, 0.3]), np.eye(3).reshape(9)
    up = [0.0, 0.0, 1.0]
    bad = [one(S.F_GPS, [P2], 3, [x2], [1, 2, 3]), one(S.F_GPS, [P3], 3, [x3], [1, 2, 3, 4]),
           one(S.F_GPS, [P3], 2, [x3], [1, 2, 3]), one(S.F_TRANS, [ROT3], 3, [xr], [1, 2, 3]),
           one(S.F_TRANS, [P2], 3, [x2], [1, 2, 3]), one(S.F_ROT, [P3], 3, [x3], [1, 2, 3]),
           one(S.F_ROT, [P2], 1, [x2], [1, 2]), one(S.F_ATT, [P2], 2, [x2], up + up),
           one(S.F_ATT, [P3], 3, [x3], up + up, A.NOISE_UNIT), one(S.F_MAG, [P2], 3, [x2], [0.0] * 9),
           one(S.F_MAG, [ROT3], 3, [xr], [0.0] * 6), one(A.F_BETWEEN, [ROT3, P3], 3, [xr, x3], xr),
           one(A.F_PRIOR, [ROT3], 3, [xr], [1, 2, 3])]
    for arr in bad:
        msg = create_status(arr)
        assert "malformed factor 0" in msg, msg
    for z, name in ((up + [0.0, 0.0, 1.0 + 1e-8], "bMeasured"), ([0.0, 0.0, 0.5] + up, "nRef")):
        msg = create_status(one(S.F_ATT, [ROT3], 2, [xr], z))
        assert name in msg and "unit length" in msg, (name, msg)
    assert create_status(one(S.F_ATT, [ROT3], 2, [xr], up + [0.0, 0.0, 1.0 + 1e-10])) == ""


def test_calls_that_know_no_rot3_refuse_it_by_name(tmp_path):
    """The writers, the Pose3 initializer, lago, landmark triangulation and smart factors answer a problem that holds a
    GSX_VAR_ROT3 variable with GSX_E_INVALID and a line that names the variable."""
    arr = R.make_arrays([(5, P3, 6), (7, ROT3, 3)],
                        [(A.F_PRIOR, [0], 6, R.pose3_state(np.eye(3), np.zeros(3)), A.NOISE_UNIT, ()),
                         (A.F_PRIOR, [1], 3, np.eye(3).reshape(9), A.NOISE_UNIT, ())],
                        np.concatenate([R.pose3_state(np.eye(3), np.zeros(3)), np.eye(3).reshape(9)]))
    last = last_call_error
    for name, call in (("gsx_write_g2o", lambda: _lib.write_g2o(str(tmp_path / "a.g2o"), arr, arr.values)),
                       ("gsx_write_bal", lambda: _lib.write_bal(str(tmp_path / "a.bal"), arr, arr.values)),
                       ("gsx_save2d", lambda: _lib.save2d(str(tmp_path / "a.graph"), arr, arr.values, [1.0, 1.0, 1.0])),
                       ("gsx_initialize_pose3", lambda: _lib.initialize_pose3(arr)),
                       ("gsx_lago_initialize", lambda: _lib.lago_initialize(arr)),
                       ("gsx_triangulate_landmarks", lambda: _lib.triangulate_landmarks(arr, arr.values))):
        with pytest.raises(Exception):
            call()
        assert last().startswith(name + ":") and "variable 1 (key 7) is a GSX_VAR_ROT3" in last(), (name, last())
    smart = R.make_arrays([(5, P3, 6), (7, ROT3, 3)],
                          [(A.F_SMART_PROJECTION, [0, 1], 1, [500.0, 500.0, 0.0, 320.0, 240.0, 1.0, 0.0, -1.0, -1.0, 1e-3, 1.0,
                                                             1.0, 2.0, 3.0, 4.0], A.NOISE_UNIT, ())], arr.values)
    msg = create_status(smart)
    assert "GSX_F_SMART_PROJECTION on variable 1, a GSX_VAR_ROT3" in msg, msg
    # a call that goes through clears the line of the refusal before it
    plain = R.make_arrays([(5, P3, 6)], [(A.F_PRIOR, [0], 6, R.pose3_state(np.eye(3), np.zeros(3)), A.NOISE_UNIT, ())],
                          R.pose3_state(np.eye(3), np.zeros(3)))
    _lib.write_g2o(str(tmp_path / "b.g2o"), plain, plain.values)
    assert last() == ""
