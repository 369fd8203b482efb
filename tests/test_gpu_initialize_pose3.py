"""InitializePose3 on the device, through the C ABI (include/gsx.h: gsx_initialize_pose3 and its stages), against the
reference's known answers (gtsam/slam/tests/testInitializePose3.cpp) and against tests/_init_pose3_restatement.py, which
tests/test_host_initialize_pose3.py pins on those same answers.  Where a bound is not the reference's own it is derived in
the test that uses it."""
import functools

import numpy as np
import pytest

import gtsam_petercdev_amd as gt
from gtsam_petercdev_amd import _abi as A, _lib
from tests import _factor_restatement as FR
from tests import _init_pose3_cases as CS
from tests import _init_pose3_restatement as IR

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
# seeds of the random graphs: chosen so that the restatement meets the conditions the bounds below are derived from
# (cond of the relaxed normal matrix <= 1e4, sigma_2 + sigma_3 >= 0.5 at every pose; for the 70-pose graph also the margins
# of the gradient's stopping test) — each test asserts them again.  The 70-pose graph takes all 10 loop closures and takes
# them between poses at least 15 apart along the chain: with short closures the largest gradient norm falls by about 1 % per
# iteration where it crosses 5e-3, which leaves no room for a 1 % margin on either side of the threshold.
SEEDS = {5: 1, 24: 2, 70: 37}
PERTURBATION_SEEDS = {24: 124, 70: 8}


@functools.lru_cache(maxsize=None)
def graph(n):
    if n == 70:
        return CS.random_pose_graph(n, SEEDS[n], max_angle=2.5, min_span=15, loops=10)
    return CS.random_pose_graph(n, SEEDS[n], max_angle=2.5)


@functools.lru_cache(maxsize=None)
def chordal_reference(n):
    return IR.chordal(graph(n)[0], want_details=True)


@functools.lru_cache(maxsize=None)
def perturbed_truth(n):
    arr, _ = graph(n)
    rng = np.random.default_rng(PERTURBATION_SEEDS[n])
    given = arr.values.copy()
    so = arr.state_offsets()
    for v in range(arr.n_vars):
        w = rng.normal(size=3)
        R = given[so[v]:so[v] + 9].reshape(3, 3) @ FR.so3_expmap(0.2 * w / np.linalg.norm(w))
        given[so[v]:so[v] + 9] = R.reshape(9)
    return given


@functools.lru_cache(maxsize=None)
def gradient_reference(n, max_iter):
    return IR.orientations_gradient(graph(n)[0], perturbed_truth(n), max_iter, False)


# ---- 1. gsx_closest_rotations ----------------------------------------------------------------------------------------------
def test_closest_rotations_against_50_digits():
    """Per matrix: 8 x max(distance of numpy's float64 LAPACK answer from the 50-digit answer, 2^-52) — the float64 SVD
    route stands in for Eigen's JacobiSVD, the factor is the room between two correct float64 SVDs.  Distances are the
    largest absolute entry."""
    Ms = CS.closest_rotation_cases()
    assert 390 <= len(Ms) <= 420 and len(Ms) % 256 != 0 and len(Ms) > 256   # more than one block, ragged last one
    R = _lib.closest_rotations(Ms)
    worst, worst_lapack, n_neg = 0.0, 0.0, 0
    for M, Rd in zip(Ms, R):
        Rm, S, d = IR.closest_rotation_mp(M)
        s1, s2, s3 = (float(x) for x in S)
        if d > 0:
            assert s2 + s3 > 0.05 * s1
        else:
            assert s2 - s3 > 0.05 * s1
            n_neg += 1
        Rm = IR.mp_to_np(Rm)
        e_lapack = np.abs(IR.closest_rotation_np(M) - Rm).max()
        e_dev = np.abs(Rd - Rm).max()
        worst = max(worst, e_dev / (8 * max(e_lapack, EPS)))
        worst_lapack = max(worst_lapack, e_lapack / EPS)
        assert np.abs(Rd.T @ Rd - np.eye(3)).max() <= 32 * EPS
        assert np.linalg.det(Rd) > 0
    print(f"closest rotations: worst device error / bound {worst:.3f}; worst LAPACK error {worst_lapack:.1f} eps")
    assert n_neg >= 5
    assert worst <= 1.0


# ---- 2. chordal: the reference's answers ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("second", [False, True], ids=["orientations", "orientationsPrecisions"])
def test_chordal_reference_answers(second):
    R = _lib.pose3_orientations_chordal(CS.simple_arrays(second))
    for i in range(4):
        assert np.abs(R[i] - CS.SIMPLE_R[i]).max() < 1e-6, i


# ---- 3. chordal against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 24, 70])
def test_chordal_against_restatement(n):
    """1e-9 absolute per rotation entry: the relaxed solution carries about eps x cond, and the projection amplifies an error
    of its input by at most 1 / (sigma_2 + sigma_3); with cond <= 1e4 and sigma_2 + sigma_3 >= 0.5 (asserted) that is about
    5e-12 — two orders of room."""
    arr, _ = graph(n)
    ref, det = chordal_reference(n)
    assert det["cond"] <= 1e4
    assert min(s[1] + s[2] for s in det["sing"].values()) >= 0.5
    R = _lib.pose3_orientations_chordal(arr)
    assert len(ref) == n
    worst = max(np.abs(R[i] - ref[i]).max() for i in range(n))
    print(f"chordal n={n}: cond {det['cond']:.3g}, worst entry error {worst:.3g}")
    assert worst <= 1e-9


# ---- 4. gradient ------------------------------------------------------------------------------------------------------------------
def test_gradient_one_iteration_reference_answer():
    arr = CS.simple_arrays(poses=CS.perturbed_guess())
    R, it = _lib.pose3_orientations_gradient(arr, arr.values, 1, False)
    assert it == 1
    for i in range(4):
        assert np.abs(R[i] - CS.ITERATION_GRADIENT[i]).max() < 1e-5, i


def test_gradient_ten_iterations_reference_fixture():
    arr = CS.simple_arrays(poses=CS.perturbed_guess())
    R, it = _lib.pose3_orientations_gradient(arr, arr.values, 10, False)
    assert it == 10
    for i, (Re, tol) in enumerate(zip(CS.gradient10_expected(), CS.GRADIENT10_TOL)):
        assert np.abs(R[i] - Re).max() < tol, i


@pytest.mark.parametrize("set_ref_frame", [False, True])
def test_gradient_against_restatement(set_ref_frame):
    """The float64 restatement on the 70-pose graph from the truth perturbed by 0.2 rad: the same operations in the same
    order, so the entries agree to 1e-10 after up to 200 iterations and the iteration counts are equal — the count cannot
    hinge on rounding because maxGrad at the stopping iteration and at the one before are each more than 1 % off 5e-3."""
    arr, _ = graph(70)
    given = perturbed_truth(70)
    for f in range(arr.n_factors):   # relative rotations stay off the logarithm's pi
        assert np.linalg.norm(FR.so3_logmap(arr.meas[arr.f_meas_ptr[f]:arr.f_meas_ptr[f] + 9].reshape(3, 3))) <= 2.5
    ref, it_ref, trace, Rref = gradient_reference(70, 200)
    assert 21 < it_ref < 200
    assert trace[it_ref - 1] < 5e-3 <= trace[it_ref - 2]
    assert abs(trace[it_ref - 1] - 5e-3) > 0.01 * 5e-3 and abs(trace[it_ref - 2] - 5e-3) > 0.01 * 5e-3
    R, it = _lib.pose3_orientations_gradient(arr, given, 200, set_ref_frame)
    worst = max(np.abs(R[i] - (Rref @ ref[i] if set_ref_frame else ref[i])).max() for i in range(70))
    print(f"gradient: {it} iterations (restatement {it_ref}), worst entry error {worst:.3g}")
    assert it == it_ref
    assert worst <= 1e-10


@pytest.mark.parametrize("max_iter", [1, 25])
def test_gradient_iteration_limits(max_iter):
    """max_iter = 25 crosses the it > 20 gate inside one batch of launches; neither run stops early."""
    arr, _ = graph(70)
    ref, it_ref, trace, _ = gradient_reference(70, max_iter)
    assert it_ref == max_iter and min(trace[21:] + [1.0]) >= 5e-3 * 1.01
    R, it = _lib.pose3_orientations_gradient(arr, perturbed_truth(70), max_iter, False)
    assert it == max_iter
    assert max(np.abs(R[i] - ref[i]).max() for i in range(70)) <= 1e-10


# ---- 5. computePoses / initialize -----------------------------------------------------------------------------------------------
def test_poses_with_given_guess():
    arr = CS.simple_arrays()
    out, it = _lib.initialize_pose3(arr, arr.values)
    assert it == 0
    assert np.abs(out - arr.values).max() < 1e-6


def test_initialize_poses_grid():
    arr = CS.grid_arrays()
    out, _ = _lib.initialize_pose3(arr)
    assert np.abs(out - arr.values).max() < 0.1


@pytest.mark.parametrize("which", ["grid", "random70"])
def test_compute_poses_against_restatement(which):
    """The Gauss-Newton step from the device's own chordal rotations against the dense system of _factor_restatement on the
    anchor graph + retract: 1e-8 relative, the project's bound for a step."""
    arr = CS.grid_arrays() if which == "grid" else graph(70)[0]
    R = _lib.pose3_orientations_chordal(arr)
    out = _lib.pose3_compute_poses(arr, R)
    ref = IR.compute_poses(arr, {i: R[i] for i in range(len(R))})
    rel = np.linalg.norm(out - ref) / np.linalg.norm(ref)
    print(f"computePoses {which}: relative difference {rel:.3g}")
    assert rel <= 1e-8


@pytest.mark.parametrize("which", ["grid", "random24"])
def test_initialize_is_chordal_then_compute_poses(which):
    arr = CS.grid_arrays() if which == "grid" else graph(24)[0]
    out, _ = _lib.initialize_pose3(arr)
    staged = _lib.pose3_compute_poses(arr, _lib.pose3_orientations_chordal(arr))
    assert np.array_equal(out, staged)


def test_initialize_with_gradient_is_gradient_then_compute_poses():
    arr, _ = graph(24)
    given = perturbed_truth(24)
    p = _lib.init_pose3_params_default()
    p.use_gradient, p.max_gradient_iterations = 1, 40
    out, it = _lib.initialize_pose3(arr, given, p)
    R, it2 = _lib.pose3_orientations_gradient(arr, given, 40, True)
    assert it == it2 and 0 < it <= 40
    assert np.array_equal(out, _lib.pose3_compute_poses(arr, R, fill=given))


# ---- 6. refusals on the device -----------------------------------------------------------------------------------------------
def test_graph_without_prior_is_indeterminate():
    arr = CS.simple_arrays()
    n = arr.n_factors - 1   # (the prior is the last factor)
    bare = A.ProblemArrays(
        arr.var_keys, arr.var_types, arr.var_dims, arr.f_type[:n], arr.f_rows[:n], arr.f_key_ptr[:n + 1],
        arr.f_vars[:arr.f_key_ptr[n]], arr.f_meas_ptr[:n + 1], arr.meas[:arr.f_meas_ptr[n]], arr.f_noise_kind[:n],
        arr.f_noise_ptr[:n + 1], arr.noise[:arr.f_noise_ptr[n]], arr.values.copy())
    for _ in range(2):   # the handle-free call leaves nothing behind
        with pytest.raises(A.IndeterminantLinearSystemException):
            _lib.initialize_pose3(bare)
        with pytest.raises(A.IndeterminantLinearSystemException):
            _lib.pose3_orientations_chordal(bare)
    out, _ = _lib.initialize_pose3(arr)   # and the device still works
    assert np.abs(out - arr.values).max() < 1e-6


# ---- 7. the Python interface ---------------------------------------------------------------------------------------------------
def test_python_interface_on_the_simple_graph():
    """InitializePose3 and Rot3.ClosestTo of the package, on the reference's answers (tolerances as there)."""
    g = CS.simple_graph()
    poses = CS.simple_poses()
    init = gt.InitializePose3.initialize(g, CS.simple_values())
    again = gt.InitializePose3.initialize(g)
    pg = gt.InitializePose3.buildPose3graph(g)
    rot = gt.InitializePose3.computeOrientationsChordal(pg)
    rot2 = gt.InitializePose3.initializeOrientations(g)
    staged = gt.InitializePose3.computePoses(rot, pg)
    for k, p in zip(CS.X, poses):
        assert init.at(k).equals(p, 1e-6) and again.at(k).equals(p, 1e-6) and staged.at(k).equals(p, 1e-6)
        assert np.abs(rot.at(k).matrix() - p.rotation().matrix()).max() < 1e-6
        assert np.array_equal(rot.at(k).matrix(), rot2.at(k).matrix())
    assert init.size() == 4 and not init.exists(A.ANCHOR_KEY)
    guess = CS.simple_values(CS.perturbed_guess())
    one = gt.InitializePose3.computeOrientationsGradient(pg, guess, 1, False)
    for k, Re in zip(CS.X, CS.ITERATION_GRADIENT):
        assert np.abs(one.at(k).matrix() - Re).max() < 1e-5
    # maxIter 10000: runs until the largest gradient norm is below 5e-3, i.e. (a = 6.01, at least two edges a node) rotation
    # errors of some 4e-4 rad, which one Gauss-Newton iteration turns into translation errors of about 1e-3 on this 2 m
    # graph: 1e-2 holds that with room and is far below the 1e-2 rad perturbation's effect on an unconverged run
    by_gradient = gt.InitializePose3.initialize(g, guess, True)
    for k, p in zip(CS.X, poses):
        assert by_gradient.at(k).equals(p, 1e-2)
    M = poses[1].rotation().matrix() + 1e-3 * np.arange(9.0).reshape(3, 3)
    assert np.abs(gt.Rot3.ClosestTo(M).matrix() - IR.closest_rotation_np(M)).max() < 1e-14


def test_stage_timings_are_kept():
    arr, _ = graph(24)
    _lib.initialize_pose3(arr)
    t = _lib.pose3_init_timings()
    assert t["gradient_iterations"] == 0 and t["gradient_ms"] == 0
    assert all(t[k] > 0 for k in ("relaxed_analysis_host_ms", "chordal_blocks_ms", "three_relaxed_solves_ms", "projection_ms",
                                  "anchor_analysis_host_ms", "gauss_newton_ms"))
    _lib.pose3_orientations_gradient(arr, perturbed_truth(24), 7, True)
    t = _lib.pose3_init_timings()
    assert t["gradient_iterations"] == 7 and t["gradient_ms"] > 0 and t["three_relaxed_solves_ms"] == 0
