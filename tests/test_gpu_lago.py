"""lago on the device, through the C ABI (include/gsx.h: gsx_lago_*) and through graph.lago, against the reference's known
answers (gtsam/slam/tests/testLago.cpp, at its tolerances) and against tests/_lago_restatement.py, which
tests/test_host_lago.py holds to the same answers on the CPU.

Tolerances.  Kernel (a), the cumulative orientations by pointer jumping, sums in another order than the reference's walk:
per node |error| <= depth * 2^-53 * sum |delta| over its path (include/gsx.h), evaluated per node.  Kernel (b): the
regularized measurement is the measured angle minus an exact multiple of 2 pi as long as `round` sees the same side of a
half-integer, which the test's inputs guarantee by a margin of 1e-6 turns, checked on the CPU; 1e-12 absolute covers the
one fused multiply-add.  End to end: 1e-8 relative, what DESIGN.md §5 allows the step of a linear solve; the pose stage of
the two larger graphs needs more, because the float64 restatement itself (dense normal equations, anchor prior of variance
1e-8 beside measurement sigmas of 0.02 .. 1) is no closer than that to its own solution in extended precision
(_lago_restatement.initialize(..., extended=True): the normal equations in numpy.longdouble, refined to their rounding
level).  Measured on the CPU, relative in the max norm, the same for both trees: 3.9e-11 (60 poses), 1.04e-8 (400),
3.3e-9 (1 500); ten times that is allowed where it exceeds 1e-8.  No figure of the device enters."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import gtsam_petercdev_amd as gt
from gtsam_petercdev_amd import _abi as A, _lib, datasets
from tests import _lago_cases as CS
from tests import _lago_restatement as LR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANCHOR = A.ANCHOR_KEY
X = CS.X


def _poses_of(arr, packed):
    so = arr.state_offsets()
    return {int(k): packed[so[i]:so[i] + 3] for i, k in enumerate(arr.var_keys) if arr.var_types[i] == A.VAR_POSE2}


def _assert_simple_poses(poses, tol=1e-6):
    for k, p in zip(X, CS.SIMPLE_POSES):
        q = poses[k] if isinstance(poses, dict) else poses.at(k).state()
        assert abs(q[0] - p[0]) < tol and abs(q[1] - p[1]) < tol and abs(LR.wrap(q[2] - p[2])) < tol


# ---- 1. the reference's known answers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [None, "pose", "rot"], ids=["smallGraph", "multiplePosePriors", "multiplePoseAndRotPriors"])
@pytest.mark.parametrize("odometric", [False, True], ids=["mst", "SP"])
def test_orientations_of_the_small_graphs(extra, odometric):
    arr = CS.simple_arrays(extra)
    th = _lib.lago_initialize_orientations(arr, odometric)
    assert np.abs(th - np.array(CS.SIMPLE_THETA)).max() < 1e-6
    vv = gt.lago.initializeOrientations(CS.simple_graph(extra), odometric)
    assert set(vv) == set(X) | {ANCHOR} and vv[ANCHOR][0] == 0.0
    for k, t in zip(X, CS.SIMPLE_THETA):
        assert abs(vv[k][0] - t) < 1e-6


def test_tree_orientations_and_regularized_measurements_of_the_small_graph():
    pg = gt.lago.buildPose2graph(CS.simple_graph())
    tree = gt.lago.findMinimumSpanningTree(pg)
    tree_ids, chord_ids, delta = gt.lago.getSymbolicGraph(tree, pg)
    assert tree_ids == [0, 1, 2, 5] and chord_ids == [3, 4]
    actual = gt.lago.computeThetasToRoot(delta, tree)                       # orientationsOverSpanningTree
    assert actual[ANCHOR] == 0.0
    for k, t in zip(X, CS.SIMPLE_THETA):
        assert abs(actual[k] - t) < 1e-6
    reg = _lib.lago_regularized_measurements(CS.simple_arrays(), False)     # regularizedMeasurements, the reference's rows
    rows = [reg[i] for i in tree_ids + chord_ids][:5]
    assert np.abs(np.array(rows) - np.array([math.pi / 2, math.pi / 2, math.pi / 2, 0.0, -math.pi])).max() < 1e-6


def test_small_graph_values_and_small_graph_2():
    arr = CS.simple_arrays(zero_theta=True)
    _assert_simple_poses(_poses_of(arr, _lib.lago_initialize_with_guess(arr, arr.values)))       # smallGraphValues
    _assert_simple_poses(gt.lago.initialize(CS.simple_graph(), CS.simple_values(zero_theta=True)))
    for odometric in (True, False):
        _assert_simple_poses(_poses_of(arr, _lib.lago_initialize(arr, odometric)))                # smallGraph2
        _assert_simple_poses(gt.lago.initialize(CS.simple_graph(), odometric))
    _assert_simple_poses(gt.lago.initialize(CS.simple_graph()))


def test_large_graph_noisy():
    arr = CS.noisy_toy_arrays()
    th = _lib.lago_initialize_orientations(arr)
    for k, p in CS.read_g2o_poses("orientationsNoisyToyGraph.txt").items():
        assert abs(LR.wrap(th[int(np.searchsorted(arr.var_keys, np.uint64(k)))] - p[2])) < 1e-5, k
    poses = _poses_of(arr, _lib.lago_initialize(arr))
    for k, p in CS.read_g2o_poses("optimizedNoisyToyGraph.txt").items():
        assert np.abs(poses[k][:2] - p[:2]).max() < 1e-2 and abs(LR.wrap(poses[k][2] - p[2])) < 1e-2, k


# ---- 2. kernel (a): the cumulative orientations ---------------------------------------------------------------------------------
def _forest_cases():
    cases = {f"random{n}": CS.random_tree(n, 100 + n) for n in (1, 2, 63, 64, 65, 257, 4097)}
    star = np.zeros(300, np.int32)
    cases["star"] = (star, CS.random_tree(300, 7)[1])
    chain = np.maximum(np.arange(5000, dtype=np.int32) - 1, 0)
    cases["chain5000"] = (chain, np.random.default_rng(8).uniform(-0.5, 3.2, 5000))   # sums of hundreds of radians
    for depth in (64, 65):      # the deepest path exactly a power of two, and one more: 6 rounds are enough, 7 are run
        parent, delta = CS.random_tree(400, 9, max_back=3)
        parent[:depth + 1] = np.maximum(np.arange(depth + 1) - 1, 0)
        parent[depth + 1:] = np.minimum(parent[depth + 1:], 20)                        # the rest hangs off the top of it
        cases[f"depth{depth}"] = (parent.astype(np.int32), delta)
    return cases


FORESTS = _forest_cases()


@pytest.mark.parametrize("case", list(FORESTS))
def test_thetas_to_root_within_the_documented_bound(case):
    parent, delta = FORESTS[case]
    ref, depth, absum = LR.thetas_to_root_arrays(parent, delta)
    if case.startswith("depth"):
        assert depth.max() == int(case[5:])
    if case == "chain5000":
        assert depth.max() == 4999 and np.abs(ref).max() > 300
    got = _lib.lago_thetas_to_root(parent, delta)
    bound = depth * 2.0 ** -53 * absum
    worst = int(np.argmax(np.abs(got - ref) - bound))
    print(f"{case}: max |error| {np.abs(got - ref).max():.3e}, at the worst node {abs(got[worst] - ref[worst]):.3e} "
          f"against {bound[worst]:.3e}")
    assert np.all(np.abs(got - ref) <= bound)


# ---- 3. kernel (b): the regularized measurements ---------------------------------------------------------------------------------
@pytest.mark.parametrize("odometric", [True, False], ids=["odometric", "mst"])
@pytest.mark.parametrize("case", list(CS.SPIRALS))
def test_regularized_measurements_on_spirals(case, odometric):
    arr = CS.spiral_arrays(**CS.SPIRALS[case])
    s = LR.structure(arr, odometric)
    reg, turns = LR.regularized_measurements(s["edges"], list(s["tree_ids"]), list(s["chord_ids"]), s["theta_root"])
    t = np.array([turns[i] for i in s["chord_ids"]])
    # the condition on the inputs: no chord within 1e-6 turns of a half-integer, so `round` cannot differ between the two
    # summation orders
    assert np.abs(t - np.floor(t) - 0.5).min() >= 1e-6
    k = np.round(t)
    assert np.count_nonzero(k) > len(k) // 2 and np.abs(k).max() >= 2 and (k.min() < 0 or case != "right")
    got = _lib.lago_regularized_measurements(arr, odometric)
    ref = np.array([reg[i] for i in range(len(s["edges"]))])
    print(f"{case}: {len(k)} chords, k from {int(k.min())} to {int(k.max())}, max |difference| {np.abs(got - ref).max():.3e}")
    assert np.abs(got - ref).max() <= 1e-12


def test_spirals_have_chords_of_both_signs():
    ks = []
    for case in CS.SPIRALS:
        s = LR.structure(CS.spiral_arrays(**CS.SPIRALS[case]), True)
        _, turns = LR.regularized_measurements(s["edges"], list(s["tree_ids"]), list(s["chord_ids"]), s["theta_root"])
        ks += [round(v) for v in turns.values()]
    assert min(ks) <= -2 and max(ks) >= 2


# ---- 4. end to end against the restatement -----------------------------------------------------------------------------------------
# max(1e-8, 10 x |float64 restatement - extended-precision restatement|) per graph size (the module's docstring)
POSE_TOL = {60: 1e-8, 400: 10 * 1.04e-8, 1500: 10 * 3.4e-9}


@pytest.fixture(scope="module")
def manhattan():
    out = {}
    for n in (60, 400, 1500):
        arr = CS.manhattan_arrays(n)
        out[n] = (arr, {odo: (LR.initialize_orientations(arr, odo), LR.initialize(arr, odo)) for odo in (True, False)})
    return out


@pytest.mark.parametrize("odometric", [True, False], ids=["odometric", "mst"])
@pytest.mark.parametrize("n", [60, 400, 1500])
def test_end_to_end_against_the_restatement(manhattan, n, odometric):
    arr, refs = manhattan[n]
    ref_theta, ref_poses = refs[odometric]
    assert len(set(int(k) & A.NOISE_BASE_MASK for k in arr.f_noise_kind)) == 4          # mixed noise kinds
    keys = [int(k) for k in arr.var_keys]
    theta = _lib.lago_initialize_orientations(arr, odometric)
    rt = np.array([ref_theta[k] for k in keys])
    e_theta = np.abs(theta - rt).max() / np.abs(rt).max()
    poses = _lib.lago_initialize(arr, odometric).reshape(-1, 3)
    rp = np.stack([ref_poses[k] for k in keys])
    d = poses - rp
    d[:, 2] = LR.wrap(d[:, 2])
    e_pose = np.abs(d).max() / np.abs(rp).max()
    print(f"n = {n}, {'odometric' if odometric else 'mst'}: orientations {e_theta:.3e}, poses {e_pose:.3e} (relative, max norm)")
    assert np.abs(rt).max() > math.pi          # the orientations are not wrapped
    assert e_theta <= 1e-8
    assert e_pose <= POSE_TOL[n]
    assert np.all(np.abs(poses[:, 2]) <= math.pi)


# ---- 5. lago::initialize(graph, initialGuess) ---------------------------------------------------------------------------------------
def test_initialize_with_guess_keeps_x_and_y_bit_for_bit(manhattan):
    arr, _ = manhattan[400]
    rng = np.random.default_rng(3)
    given = arr.values.reshape(-1, 3).copy()
    given[:, :2] += rng.normal(0, 1, (given.shape[0], 2))
    given[:, 2] = rng.uniform(-3, 3, given.shape[0])
    out = _lib.lago_initialize_with_guess(arr, given.reshape(-1)).reshape(-1, 3)
    assert np.array_equal(out[:, :2], given[:, :2])
    theta = _lib.lago_initialize_orientations(arr, True)
    assert np.abs(LR.wrap(out[:, 2] - theta)).max() <= 1e-12 and np.all(np.abs(out[:, 2]) <= math.pi)


# ---- 6. what the pose graph does not hold is copied from the guess ---------------------------------------------------------------------
def test_landmarks_and_other_variables_are_copied_from_the_guess():
    for arr in (CS.graph_file_arrays("example.graph"), CS.simple_arrays("rot")):
        other = np.flatnonzero(arr.var_types != A.VAR_POSE2)
        assert other.size > 0
        given = arr.values.copy()
        so = arr.state_offsets()
        for v in other:
            given[so[v]:so[v + 1]] += 0.123
        out = _lib.lago_initialize(arr, True, given)
        for v in other:
            assert np.array_equal(out[so[v]:so[v + 1]], given[so[v]:so[v + 1]])
        ref = LR.initialize(arr, True)
        for k, p in _poses_of(arr, out).items():
            assert np.abs(p[:2] - ref[k][:2]).max() <= 1e-8 * max(1.0, np.abs(ref[k][:2]).max()) and abs(LR.wrap(p[2] - ref[k][2])) <= 1e-8


# ---- 7. the example program --------------------------------------------------------------------------------------------------------------
def test_example_program_on_the_toy_graph(golden_dir, tmp_path):
    exe = os.path.join(ROOT, "examples", "Pose2SLAMExample_lago.py")
    out = subprocess.run([sys.executable, exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Factor 0: BetweenFactor(0,1)" in out.stdout and "Computing LAGO estimate\ndone!\nestimateLago" in out.stdout
    assert "PriorFactor on 0" in out.stdout and "diagonal sigmas [0.001; 0.001; 0.0001];" in out.stdout
    lines = out.stdout.splitlines()
    printed = {}
    for i, line in enumerate(lines):
        if line.startswith("Value "):
            printed[int(line.split()[1].rstrip(":"))] = np.array([float(x) for x in lines[i + 1].strip("()").split(",")])
    expected = CS.read_g2o_poses("optimizedNoisyToyGraph.txt")
    assert set(printed) == set(expected)
    for k, p in expected.items():
        assert np.abs(printed[k][:2] - p[:2]).max() < 1e-2 and abs(LR.wrap(printed[k][2] - p[2])) < 1e-2
    out_file = tmp_path / "lago.g2o"
    out = subprocess.run([sys.executable, exe, os.path.join(golden_dir, "noisyToyGraph.txt"), str(out_file)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "Writing results to file" in out.stdout, out.stderr[-2000:]
    written = CS.read_g2o_poses(str(out_file))
    for k, p in expected.items():
        assert np.abs(written[k][:2] - p[:2]).max() < 1e-2 and abs(LR.wrap(written[k][2] - p[2])) < 1e-2


# ---- 8. usefulness --------------------------------------------------------------------------------------------------------------------------
def _lm_error(arr, values):
    be = _lib.product_backend(arr)
    try:
        be.set_ordering(be.compute_ordering(A.ORDER_MINDEGREE))
        be.set_values(values)
        p = A.lm_params_legacy()
        p.relative_error_tol, p.absolute_error_tol = 1e-12, 1e-12      # to convergence; compared at LM's own 1e-5 below
        return be.lm_optimize(p)["final_error"]
    finally:
        be.close()


def test_lm_from_lago_reaches_the_error_of_lm_from_the_truth():
    arr = datasets.synth_manhattan_pose2(400, seed=21, closure_prob=0.8, init_sigma=0.0)     # values: the ground truth
    bad = arr.values.reshape(-1, 3).copy()
    bad[1:, 2] = np.random.default_rng(22).uniform(-math.pi, math.pi, bad.shape[0] - 1)
    bad = bad.reshape(-1)
    e_truth, e_bad = _lm_error(arr, arr.values), _lm_error(arr, bad)
    e_lago = _lm_error(arr, _lib.lago_initialize(arr, True, bad))
    print(f"LM final error from the truth {e_truth:.9g}, from lago {e_lago:.9g}, from the bad guess {e_bad:.9g}")
    assert abs(e_lago - e_truth) <= 1e-5 * e_truth and not abs(e_bad - e_truth) <= 1e-5 * e_truth
