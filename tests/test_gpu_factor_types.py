"""RangeFactor, BearingFactor<Pose2,Point2> and GenericStereoFactor<Pose3,Point3> on the device (GSX_F_RANGE / _BEARING /
_STEREO), through the C ABI, against the numpy restatement of tests/_factor_restatement.py (the CPU oracle does not know
these types; tests/test_host_factor_types.py pins the restatement with the reference's known answers).

Bounds.  [A b] and the graph error: the project's [A b] parity bound (tests/test_gpu_parity.py: atol 1e-13 for O(1) entries)
scaled by the largest expected entry, atol = 1e-13 max(1, max |expected|) — stereo entries are O(fx).  Steps against a
dense solve of the restated normal equations: 1e-6 relative, the bound of the step comparisons of
tests/test_gpu_constraints.py.  Marginal blocks: the 1e-7 of tests/test_gpu_all_marginals.py.  In every stereo test but the
cheirality one the restatement must count ZERO factors behind their camera where results are compared.

Not here: a world-2 sharded run of these graphs — the workers of tests/test_gpu_shard.py run a fixed set of problems and
cannot be pointed at another graph without editing them."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from gtsam_petercdev_amd import _abi as A, _lib
from gtsam_petercdev_amd import graph as G
from tests import _factor_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "examples"))
pytestmark = pytest.mark.gpu

P2, P3, V = A.VAR_POSE2, A.VAR_POSE3, A.VAR_VECTOR


def backend(arr, order=A.ORDER_MINDEGREE):
    assert _lib.device_count() > 0, "no GPU visible: the HIP path has no fallback"
    be = _lib.ProductBackend(arr)
    be.set_ordering(be.compute_ordering(order))
    return be


def error_bound(arr, scale, err):
    """What the [A b] bound allows the graph error: every whitened residual r_i is off by at most d = 1e-13 scale, the
    error sum 1/2 r_i^2 (a robust loss grows no faster) therefore by at most sum |r_i| d <= sqrt(rows) sqrt(2 err) d
    (Cauchy-Schwarz), plus the rounding of the sum itself, 1e-13 relative."""
    return 1e-13 * scale * math.sqrt(float(arr.f_rows.sum())) * math.sqrt(2.0 * err) + 1e-13 * err


def check_linearization(arr, what):
    """gsx_get_jacobians and gsx_error of `arr` at its values against the restatement; returns the restated count of
    cheirality factors."""
    be = backend(arr)
    be.linearize()
    got = be.jacobians()
    want, n_cheir = R.jacobians(arr, arr.values)
    scale = max(1.0, float(np.max(np.abs(want))))
    worst = float(np.max(np.abs(got - want)))
    eg, ew = be.error(), R.graph_error(arr, arr.values)
    print(f"{what}: {arr.n_factors} factors, max |[A b] - restated| = {worst:.3e} (largest entry {scale:.3e}), "
          f"error {eg:.12g} vs {ew:.12g} (diff {abs(eg - ew):.3e})")
    assert got.shape == want.shape
    assert worst <= 1e-13 * scale, (what, worst, scale)
    assert abs(eg - ew) <= error_bound(arr, scale, ew), (eg, ew)
    be.close()
    return n_cheir


@pytest.mark.parametrize("noise", ["unit", "isotropic", "diagonal", "gaussian", "huber"])
@pytest.mark.parametrize("variant", R.VARIANTS)
def test_jacobians_and_error_match_the_restatement(variant, noise):
    """A few hundred factors of one variant between random poses and points: every noise kind and one robust loss."""
    arr = R.random_graph(variant, 300, noise, seed=11 + R.VARIANTS.index(variant))
    assert arr.n_factors >= 200
    assert check_linearization(arr, f"{variant}/{noise}") == 0


def test_all_new_types_in_one_graph_with_the_old_ones():
    """A planar graph that holds range (both variants), bearing, bearing-range, odometry and priors at once: every list of
    the linearize / error launches non-empty side by side."""
    rng = np.random.default_rng(7)
    n = 40
    poses = [np.array([1.5 * i, math.sin(0.3 * i), 0.2 * i]) for i in range(n)]
    pts = [rng.uniform(-3, 60, 2) for _ in range(25)]
    var_list = [(i, P2, 3) for i in range(n)] + [(1000 + j, V, 2) for j in range(25)]
    factors = [(A.F_PRIOR, [0], 3, poses[0], A.NOISE_DIAGONAL, [0.1, 0.1, 0.05])]
    for i in range(n - 1):
        factors.append((A.F_BETWEEN, [i, i + 1], 3, R.pose2_between(poses[i], poses[i + 1]) + rng.normal(0, 0.01, 3),
                        A.NOISE_ISOTROPIC, [0.1]))
        factors.append((A.F_RANGE, [i, i + 1], 1, [R.range_pose2(poses[i], poses[i + 1], True)[0] + 0.05], A.NOISE_ISOTROPIC, [0.2]))
    for j in range(25):
        for i in rng.choice(n, 4, replace=False):
            i = int(i)
            th, r = R.bearing_pose2(poses[i], pts[j])[0], R.range_pose2(poses[i], pts[j], False)[0]
            factors.append((A.F_RANGE, [i, n + j], 1, [r + 0.1], A.NOISE_UNIT, ()))
            factors.append((A.F_BEARING, [i, n + j], 1, [th - 0.02], A.NOISE_ISOTROPIC | A.NOISE_ROBUST_CAUCHY, [0.1, 0.5]))
            factors.append((A.F_BEARINGRANGE, [i, n + j], 2, [th + 0.01, r - 0.1], A.NOISE_DIAGONAL, [0.1, 0.3]))
    arr = R.make_arrays(var_list, factors, np.concatenate(poses + pts))
    # (BEARINGRANGE is not restated: compare the rest factor by factor, and its bearing row with the BEARING factor's)
    be = backend(arr)
    be.linearize()
    got, off = be.jacobians(), arr.jacobian_offsets()
    for f in range(arr.n_factors):
        if arr.f_type[f] == A.F_BEARINGRANGE:
            continue
        want = R.linearized(arr, arr.values, f)[0].reshape(-1, order="F")
        assert np.max(np.abs(got[off[f]:off[f + 1]] - want)) <= 1e-13 * max(1.0, np.max(np.abs(want))), f
    br = [f for f in range(arr.n_factors) if arr.f_type[f] == A.F_BEARINGRANGE][0]
    blk = got[off[br]:off[br + 1]].reshape(2, 6, order="F")
    _, H1, H2 = R.bearing_pose2(*[arr.values[arr.state_offsets()[v]:arr.state_offsets()[v + 1]] for v in R.factor_parts(arr, br)[1]])
    assert np.allclose(blk[0, :5] * 0.1, np.concatenate([H1, H2]), atol=1e-13)
    p = A.lm_params_legacy()
    r = be.lm_optimize(p)
    assert r["final_error"] < r["initial_error"]
    be.close()


def test_known_answers_through_the_device():
    """testRangeFactor.cpp:121-137,163-179 and testStereoFactor.cpp:88-153 through gsx_error / gsx_get_jacobians."""
    from tests.test_host_factor_types import WELL_FORMED, K9, two_var_graph
    for variant in ("range_pose2_point2", "range_pose2_pose2", "range_pose3_point3", "range_pose3_pose3"):
        be = backend(two_var_graph(*WELL_FORMED[variant]))
        assert abs(be.error() - 0.5 * 0.295630141 ** 2) < 1e-9
        be.linearize()
        assert abs(be.jacobians()[-1] + 0.295630141) < 1e-9          # b = -e
        be.close()
    pose = list(R.pose3_state(np.eye(3), np.array([0.0, 0.0, -6.25])))
    be = backend(two_var_graph(P3, 6, pose, V, 3, [0.0, 0.0, 0.0], A.F_STEREO, 3, K9))
    assert abs(be.error() - 7.0) < 1e-9                               # (9 + 4 + 1) / 2
    be.linearize()
    Ab = be.jacobians().reshape(3, 10, order="F")
    H1 = [[0.0, -625.0, 0.0, -100.0, 0.0, 0.0], [0.0, -625.0, 0.0, -100.0, 0.0, -8.0], [625.0, 0.0, 0.0, 0.0, -100.0, 0.0]]
    H2 = [[100.0, 0.0, 0.0], [100.0, 0.0, 8.0], [0.0, 100.0, 0.0]]
    assert np.allclose(Ab[:, :6], H1, atol=1e-3) and np.allclose(Ab[:, 6:9], H2, atol=1e-3)
    assert np.allclose(Ab[:, 9], [3.0, -2.0, 1.0], atol=1e-9)
    be.close()


def test_range_at_zero_distance_on_the_device():
    """norm2 / norm3's row of ones at r <= 1e-10, not a division by zero."""
    from tests.test_host_factor_types import POSE2, POSE3, two_var_graph
    for arr in (two_var_graph(P2, 3, POSE2, V, 2, POSE2[:2], A.F_RANGE, 1, [0.5]),
                two_var_graph(P3, 6, POSE3, V, 3, POSE3[9:], A.F_RANGE, 1, [0.5]),
                two_var_graph(P3, 6, POSE3, P3, 6, POSE3, A.F_RANGE, 1, [0.5])):
        be = backend(arr)
        be.linearize()
        got, want = be.jacobians(), R.jacobians(arr, arr.values)[0]
        assert np.all(np.isfinite(got)) and np.max(np.abs(got - want)) <= 1e-13
        assert abs(be.error() - 0.125) < 1e-15
        be.close()


@pytest.mark.parametrize("noise", ["unit", "diagonal", "huber"])
def test_stereo_cheirality_on_the_device(noise):
    """A point behind its camera: a zero block, the right-hand side -(2fx, 2fx, 2fx) whitened, that constant's error —
    among factors that are in front, which stay what they were."""
    arr = R.random_graph("stereo", 60, noise, seed=3)
    so = arr.state_offsets()
    behind = [0, 7]
    for f in behind:   # put the factor's landmark 2 m behind its camera (the restatement says which factors that flags)
        _, (a, b), _ = R.factor_parts(arr, f)
        Rm, t = R.pose3_of(arr.values[so[a]:so[a + 1]])
        arr.values[so[b]:so[b + 1]] = t + Rm @ np.array([0.3, -0.2, -2.0])
    be = backend(arr)
    be.linearize()
    got, off = be.jacobians(), arr.jacobian_offsets()
    want, n_cheir = R.jacobians(arr, arr.values)
    flagged = [f for f in range(arr.n_factors) if R.evaluate(arr, arr.values, f)[2]]
    assert set(behind) <= set(flagged) and n_cheir == len(flagged) and n_cheir < arr.n_factors // 2
    for f in flagged:
        blk = got[off[f]:off[f + 1]].reshape(3, 10, order="F")
        W, loss, k = R.whitener(arr, f)
        rhs = W @ np.full(3, -2.0 * R.STEREO_K[0])
        if loss:
            rhs = rhs * math.sqrt(R.robust_weight(loss, k, float(np.linalg.norm(rhs))))
        assert not np.any(blk[:, :9]) and np.allclose(blk[:, 9], rhs, rtol=1e-14, atol=0)
    assert np.max(np.abs(got - want)) <= 1e-13 * max(1.0, np.max(np.abs(want)))
    eg, ew = be.error(), R.graph_error(arr, arr.values)
    assert abs(eg - ew) <= error_bound(arr, max(1.0, float(np.max(np.abs(want)))), ew), (eg, ew)
    be.close()


# ---- solve parity ------------------------------------------------------------------------------------------------------
def vo_arrays(max_pose, first_pose_model):
    """The stereo graph of the VO fixture restricted to the poses x1 .. x<max_pose> (a dense solve of the whole one would
    need a 24 573 x 8 058 matrix), first pose held by `first_pose_model`; and the whole one for max_pose = None."""
    import StereoVOExample_large as ex
    graph, initial = ex.build(first_pose_model=first_pose_model, verbose=False)
    if max_pose is not None:
        keep = {G.X(i) for i in range(1, max_pose + 1)}
        sub = G.NonlinearFactorGraph()
        for f in graph.factors:
            if f.keys_[0] in keep:
                sub.add(f)
        vals = G.Values()
        for k in sub.keys():
            vals.insert(k, initial.at(k))
        graph, initial = sub, vals
    return graph.to_arrays(initial)


def check_steps(arr, what, order):
    be = backend(arr, order)
    be.linearize()
    J, b = R.dense_system(arr, arr.values)
    H, g = J.T @ J, J.T @ b
    worst = 0.0
    for lam in (0.0, 1e-3):
        want = np.linalg.solve(H + lam * np.eye(H.shape[0]), g)
        got = be.solve(lam, False)
        rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
        print(f"{what}: lambda {lam:g}, dim {H.shape[0]}, |step - dense| / |dense| = {rel:.3e}")
        worst = max(worst, rel)
        assert rel <= 1e-6, (what, lam, rel)
    be.close()
    return worst


def test_stereo_vo_step_matches_a_dense_solve():
    """The VO fixture's first six poses and their landmarks, soft prior on x1: the damped step at lambda 0 and 1e-3 against
    a dense numpy solve of the restated normal equations, 1e-6 relative."""
    arr = vo_arrays(6, G.noiseModel.Isotropic.Sigma(6, 0.01))
    n_cheir = sum(R.evaluate(arr, arr.values, f)[2] for f in range(arr.n_factors))
    assert n_cheir == 0 and int((arr.f_type == A.F_STEREO).sum()) > 1500
    check_steps(arr, "stereo VO (6 poses)", A.ORDER_SCHUR_ND)


@pytest.mark.parametrize("three_d", [False, True])
def test_range_plus_odometry_step_matches_a_dense_solve(three_d):
    rng = np.random.default_rng(21)
    n, n_l = 60, 20
    if three_d:
        poses = [R.pose3_state(R.so3_expmap(np.array([0.02 * i, -0.01 * i, 0.05 * i])), np.array([1.0 * i, 0.3 * math.sin(i), 0.1 * i]))
                 for i in range(n)]
        pts = [rng.uniform(-5, 60, 3) * np.array([1, 0.2, 0.2]) + np.array([0, 3, 2]) for _ in range(n_l)]
        ptype, pdim, ldim = P3, 6, 3
        rng_fn = R.range_pose3
    else:
        poses = [np.array([1.0 * i, math.sin(0.2 * i), 0.1 * i]) for i in range(n)]
        pts = [np.array([rng.uniform(-5, 60), rng.uniform(2, 8)]) for _ in range(n_l)]
        ptype, pdim, ldim = P2, 3, 2
        rng_fn = R.range_pose2
    var_list = [(i, ptype, pdim) for i in range(n)] + [(1000 + j, V, ldim) for j in range(n_l)]
    factors = [(A.F_PRIOR, [0], pdim, poses[0], A.NOISE_ISOTROPIC, [0.05])]
    for i in range(n - 1):
        if three_d:
            Ra, ta = R.pose3_of(poses[i])
            Rb, tb = R.pose3_of(poses[i + 1])
            z = R.pose3_state(Ra.T @ Rb @ R.so3_expmap(rng.normal(0, 0.01, 3)), Ra.T @ (tb - ta) + rng.normal(0, 0.02, 3))
        else:
            z = R.pose2_between(poses[i], poses[i + 1]) + rng.normal(0, 0.02, 3)
        factors.append((A.F_BETWEEN, [i, i + 1], pdim, z, A.NOISE_ISOTROPIC, [0.1]))
        if i % 3 == 0 and i + 5 < n:
            factors.append((A.F_RANGE, [i, i + 5], 1, [rng_fn(poses[i], poses[i + 5], True)[0] + rng.normal(0, 0.1)],
                            A.NOISE_ISOTROPIC, [0.2]))
    for j in range(n_l):
        for i in rng.choice(n, 6, replace=False):
            factors.append((A.F_RANGE, [int(i), n + j], 1, [rng_fn(poses[int(i)], pts[j], False)[0] + rng.normal(0, 0.1)],
                            A.NOISE_ISOTROPIC, [0.2]))
    arr = R.make_arrays(var_list, factors, np.concatenate(poses + [p + rng.normal(0, 0.2, ldim) for p in pts]))
    check_steps(arr, "range + odometry " + ("Pose3" if three_d else "Pose2"), A.ORDER_MINDEGREE)


# ---- optimizers end to end ---------------------------------------------------------------------------------------------
def test_lm_on_the_stereo_vo_example():
    """examples/StereoVOExample.py: the measurements are exact for x2 = (I, (0, 0, 1)) and the landmarks (1, 1, 5),
    (-1, 1, 5), (0, -0.5, 5) — disparity 40 is depth 5 from x1, disparity 50 depth 4 from x2."""
    import StereoVOExample as ex
    graph, initial = ex.build()
    opt = G.LevenbergMarquardtOptimizer(graph, initial)
    result = opt.optimize()
    print("StereoVOExample: LM", opt.result["iterations"], "iterations, final error", opt.result["final_error"])
    assert opt.result["final_error"] < 1e-9
    x1, x2 = result.at(1), result.at(2)
    assert np.array_equal(x1.state(), G.Pose3().state())
    assert np.allclose(x2.rotation().matrix(), np.eye(3), atol=1e-6) and np.allclose(x2.translation(), [0, 0, 1], atol=1e-6)
    for key, want in ((3, [1, 1, 5]), (4, [-1, 1, 5]), (5, [0, -0.5, 5])):
        assert np.allclose(result.at(key), want, atol=1e-6), key


def test_lm_on_the_large_stereo_vo_example():
    """examples/StereoVOExample_large.py in process: LM returns, lowers the error, leaves the constrained x1 where it was
    (1e-12), and a second run from the result gains no more than the LM relative tolerance."""
    import StereoVOExample_large as ex
    graph, initial = ex.build(verbose=False)
    params = G.LevenbergMarquardtParams()
    params.orderingType = "METIS"
    opt = G.LevenbergMarquardtOptimizer(graph, initial, params)
    result = opt.optimize()
    r = opt.result
    print("StereoVOExample_large: LM", r["iterations"], "iterations,", r["initial_error"], "->", r["final_error"])
    assert r["final_error"] < r["initial_error"]
    assert np.max(np.abs(result.at(G.X(1)).state() - initial.at(G.X(1)).state())) <= 1e-12
    arr = graph.to_arrays(result)
    assert sum(R.evaluate(arr, arr.values, f)[2] for f in range(arr.n_factors - 1)) == 0
    again = G.LevenbergMarquardtOptimizer(graph, result, params)
    again.optimize()
    assert again.result["initial_error"] - again.result["final_error"] <= params.relativeErrorTol * again.result["initial_error"]


def run_example(script):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", script)], capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    return out.stdout


def test_the_stereo_examples_run_as_programs():
    text = run_example("StereoVOExample.py")
    assert "Final result:" in text and "Values with 5 values:" in text and "Value 2: (gtsam::Pose3)" in text
    t = re.search(r"Value 2: \(gtsam::Pose3\)\nR: \[[^\]]*\]\nt: ([-+0-9.eE]+) ([-+0-9.eE]+) ([-+0-9.eE]+)", text)
    assert np.allclose([float(x) for x in t.groups()], [0, 0, 1], atol=1e-5)
    text = run_example("StereoVOExample_large.py")
    for line in ("Reading calibration info", "Reading camera poses", "Reading stereo factors", "Optimizing",
                 "Final result sample:", "Final camera poses:", "Values with 26 values:"):
        assert line in text, line
    e0 = float(re.search(r"initial error=([-+0-9.eE]+)", text).group(1))
    e1 = float(re.search(r"final error=([-+0-9.eE]+)", text).group(1))
    assert e1 < e0


# ---- the rest of the machinery sees the new types ----------------------------------------------------------------------
def stereo_plus_range_arrays():
    """The VO fixture's first five poses with a soft prior on x1 and range factors between consecutive poses and from
    poses to landmarks."""
    arr = vo_arrays(5, G.noiseModel.Isotropic.Sigma(6, 0.01))
    so = arr.state_offsets()
    poses = [v for v in range(arr.n_vars) if arr.var_types[v] == P3]
    lms = [v for v in range(arr.n_vars) if arr.var_types[v] == V]
    st = lambda v: arr.values[so[v]:so[v + 1]]
    for a, b in zip(poses[:-1], poses[1:]):
        arr = arr.with_factor(A.F_RANGE, [a, b], 1, [R.range_pose3(st(a), st(b), True)[0] + 0.01], A.NOISE_ISOTROPIC, [0.05])
    for i, l in enumerate(lms[::40]):
        a = poses[i % len(poses)]
        arr = arr.with_factor(A.F_RANGE, [a, l], 1, [R.range_pose3(st(a), st(l), False)[0] - 0.02], A.NOISE_ISOTROPIC, [0.1])
    return arr


def test_partial_relinearization_is_bit_identical_on_a_stereo_plus_range_graph():
    """gsx_relinearize_partial after moving a few variables against a full gsx_linearize + gsx_solve(0) at the same values."""
    arr = stereo_plus_range_arrays()
    so = arr.state_offsets()
    rng = np.random.default_rng(4)
    ranged = sorted({int(arr.f_vars[arr.f_key_ptr[f] + 1]) for f in range(arr.n_factors) if arr.f_type[f] == A.F_RANGE} &
                    {int(v) for v in np.nonzero(arr.var_types == V)[0]})
    moved = ranged[:6]   # landmarks that carry stereo AND range factors: both families go through the partial lists
    assert len(moved) == 6
    new_states = [R.retract(int(arr.var_types[v]), arr.values[so[v]:so[v + 1]], rng.normal(0, 0.01, int(arr.var_dims[v])))
                  for v in moved]
    be = backend(arr, A.ORDER_SCHUR_ND)
    be.linearize()
    be.solve(0.0, False)
    stats = be.relinearize_partial([int(arr.var_keys[v]) for v in moved], np.concatenate(new_states))
    d_partial, j_partial = be.solve(0.0, False), be.jacobians()
    vals = be.get_values()
    full = backend(arr, A.ORDER_SCHUR_ND)
    full.set_values(vals)
    full.linearize()
    d_full, j_full = full.solve(0.0, False), full.jacobians()
    print("partial relinearization:", stats)
    assert 0 < stats["n_factors_relinearized"] < arr.n_factors and stats["n_fronts_reeliminated"] < stats["n_fronts"]
    assert np.array_equal(j_partial, j_full) and np.array_equal(d_partial, d_full)
    want, n_cheir = R.jacobians(arr, vals)
    assert n_cheir == 0 and np.max(np.abs(j_full - want)) <= 1e-13 * max(1.0, np.max(np.abs(want)))
    be.close()
    full.close()


def test_marginal_covariances_match_the_restated_dense_inverse():
    arr = stereo_plus_range_arrays()
    be = backend(arr, A.ORDER_SCHUR_ND)
    be.linearize()
    blocks = be.marginal_covariances()
    J, _ = R.dense_system(arr, arr.values)
    C = np.linalg.inv(J.T @ J)
    to = arr.tangent_offsets()
    worst = 0.0
    for i, k in enumerate(arr.var_keys):
        co = C[to[i]:to[i + 1], to[i]:to[i + 1]]
        err = float(np.max(np.abs(blocks[int(k)] - co)) / np.max(np.abs(co)))
        worst = max(worst, err)
        assert err <= 1e-7, (int(k), err)
    print(f"marginals of a stereo + range graph: {arr.n_vars} blocks, worst relative error {worst:.3e}")
    be.close()
