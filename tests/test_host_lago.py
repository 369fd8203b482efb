"""lago without a GPU: the restatement tests/_lago_restatement.py reproduces the reference's known answers
(gtsam/slam/tests/testLago.cpp, at the reference's own tolerances), and the host side of the C ABI — the pose graph, the
two spanning trees, the tree / chord split, the refusals that come before any device is touched — behaves as include/gsx.h
says."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import gtsam_petercdev_amd as gt
from gtsam_petercdev_amd import _abi as A, _lib
from tests import _lago_cases as CS
from tests import _lago_restatement as LR

ANCHOR = A.ANCHOR_KEY
X = CS.X


@pytest.fixture(scope="module")
def lib():
    from gtsam_petercdev_amd import build
    build.build_lib()
    return _lib.load()


def _simple_edges(extra=None):
    return LR.build_pose_graph(CS.simple_arrays(extra))


# ---- the restatement against the reference's known answers ------------------------------------------------------------
def test_restatement_find_minimum_spanning_tree():
    tree = LR.find_minimum_spanning_tree(_simple_edges())
    assert tree == {ANCHOR: ANCHOR, X[0]: ANCHOR, X[1]: X[0], X[2]: X[1], X[3]: X[2]}


def test_restatement_check_st_and_chords():
    edges = _simple_edges()
    tree_ids, chord_ids, _ = LR.get_symbolic_graph(LR.find_minimum_spanning_tree(edges), edges)
    assert tree_ids[:3] == [0, 1, 2] and tree_ids == [0, 1, 2, 5] and chord_ids == [3, 4]


def test_restatement_orientations_over_spanning_tree():
    edges = _simple_edges()
    tree = LR.find_minimum_spanning_tree(edges)
    _, _, delta = LR.get_symbolic_graph(tree, edges)
    actual = LR.compute_thetas_to_root(delta, tree)
    for k, t in zip(X, CS.SIMPLE_THETA):
        assert abs(actual[k] - t) < 1e-6


def test_restatement_regularized_measurements():
    edges = _simple_edges()
    tree = LR.find_minimum_spanning_tree(edges)
    tree_ids, chord_ids, delta = LR.get_symbolic_graph(tree, edges)
    reg, _ = LR.regularized_measurements(edges, tree_ids, chord_ids, LR.compute_thetas_to_root(delta, tree))
    # the reference's row order: the tree edges (0, 1, 2 and the prior's, id 5), then the chords (3, 4); its test reads the
    # first five rows
    rows = [reg[i] for i in tree_ids + chord_ids]
    expected = [math.pi / 2, math.pi / 2, math.pi / 2, 0.0, -math.pi]
    assert np.abs(np.array(rows[:5]) - np.array(expected)).max() < 1e-6


@pytest.mark.parametrize("extra", [None, "pose", "rot"], ids=["smallGraph", "multiplePosePriors", "multiplePoseAndRotPriors"])
@pytest.mark.parametrize("odometric", [False, True], ids=["mst", "SP"])
def test_restatement_orientations_of_the_small_graphs(extra, odometric):
    th = LR.initialize_orientations(CS.simple_arrays(extra), odometric)
    for k, t in zip(X, CS.SIMPLE_THETA):
        assert abs(th[k] - t) < 1e-6


def _assert_simple_poses(poses, tol=1e-6):
    for k, p in zip(X, CS.SIMPLE_POSES):
        assert abs(poses[k][0] - p[0]) < tol and abs(poses[k][1] - p[1]) < tol
        assert abs(LR.wrap(poses[k][2] - p[2])) < tol


def test_restatement_small_graph_values():
    arr = CS.simple_arrays(zero_theta=True)
    _assert_simple_poses(LR.initialize_with_guess(arr, arr.values))


def test_restatement_small_graph_2():
    _assert_simple_poses(LR.initialize(CS.simple_arrays()))


def test_restatement_large_graph_noisy_orientations():
    th = LR.initialize_orientations(CS.noisy_toy_arrays())
    for k, p in CS.read_g2o_poses("orientationsNoisyToyGraph.txt").items():
        assert abs(LR.wrap(th[k] - p[2])) < 1e-5, k


def test_restatement_large_graph_noisy():
    poses = LR.initialize(CS.noisy_toy_arrays())
    for k, p in CS.read_g2o_poses("optimizedNoisyToyGraph.txt").items():
        assert np.abs(poses[k][:2] - p[:2]).max() < 1e-2 and abs(LR.wrap(poses[k][2] - p[2])) < 1e-2, k


# ---- gsx_lago_structure against the restatement, exactly ----------------------------------------------------------------
STRUCTURE_CASES = {
    "simpleLago-mst": (lambda: CS.simple_arrays(), False),
    "simpleLago-odometric": (lambda: CS.simple_arrays(), True),
    "simpleLago-rot-prior-mst": (lambda: CS.simple_arrays("rot"), False),
    "noisyToyGraph-mst": (lambda: CS.noisy_toy_arrays(), False),
    "noisyToyGraph-odometric": (lambda: CS.noisy_toy_arrays(), True),
    "w100-mst": (lambda: CS.graph_file_arrays("w100.graph"), False),
    "w100-odometric": (lambda: CS.graph_file_arrays("w100.graph"), True),
    "noncontiguous-mst": (lambda: CS.noncontiguous_arrays(), False),
    "two-priors-mst": (lambda: CS.two_prior_arrays(), False),
    "two-priors-odometric": (lambda: CS.two_prior_arrays(), True),
    "duplicate-edge-mst": (lambda: CS.duplicate_edge_arrays(), False),
    "duplicate-edge-odometric": (lambda: CS.duplicate_edge_arrays(), True),
    "example.graph-mst": (lambda: CS.graph_file_arrays("example.graph"), False),
    "example.graph-odometric": (lambda: CS.graph_file_arrays("example.graph"), True),
    "manhattan400-mst": (lambda: CS.manhattan_arrays(400), False),
}


@pytest.mark.parametrize("case", list(STRUCTURE_CASES))
def test_structure_equals_the_restatement(lib, case):
    build, odometric = STRUCTURE_CASES[case]
    arr = build()
    ref = LR.structure(arr, odometric)
    got = _lib.lago_structure(arr, odometric)
    for name in ("edge_from", "edge_to", "parent", "tree_ids", "chord_ids"):
        assert np.array_equal(got[name], ref[name]), name
    assert np.array_equal(got["delta"], ref["delta"])          # bit for bit: a measurement or its negation
    assert got["max_depth"] == ref["max_depth"]
    assert len(got["tree_ids"]) + len(got["chord_ids"]) == len(got["edge_from"])


def test_structure_known_answers(lib):
    s = _lib.lago_structure(CS.simple_arrays(), False)
    assert s["parent"].tolist() == [4, 0, 1, 2, 4] and s["tree_ids"].tolist() == [0, 1, 2, 5] and s["max_depth"] == 4
    assert s["chord_ids"].tolist() == [3, 4] and s["edge_from"].tolist() == [0, 1, 2, 2, 0, 4]
    # a duplicate odometry edge is a tree edge too, and does not overwrite the node's deltaTheta
    arr = CS.duplicate_edge_arrays()
    d = _lib.lago_structure(arr, True)
    assert d["tree_ids"].tolist() == [0, 1, 2, 3, 4, 5, 7] and d["chord_ids"].tolist() == [6]
    assert d["delta"][2] == arr.meas[3 * 1 + 2]
    # example.graph: only the odometry and the prior are edges
    ex = CS.graph_file_arrays("example.graph")
    n_used = int(np.count_nonzero(ex.f_type == A.F_BETWEEN) + 1)
    assert np.count_nonzero(ex.f_type == A.F_BEARINGRANGE) > 0 and len(_lib.lago_structure(ex, True)["edge_from"]) == n_used
    # the package's own names
    tree = gt.lago.findMinimumSpanningTree(gt.lago.buildPose2graph(CS.simple_graph()))
    assert tree == {ANCHOR: ANCHOR, X[0]: ANCHOR, X[1]: X[0], X[2]: X[1], X[3]: X[2]}
    st, ch, delta = gt.lago.getSymbolicGraph(tree, CS.simple_graph())
    assert st == [0, 1, 2] and ch == [3, 4] and set(delta) == {X[1], X[2], X[3]}    # (the raw graph: the prior is unary)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _calls(arr, odometric, device=0):
    return [
        lambda: _lib.lago_initialize(arr, odometric, arr.values, device=device),
        lambda: _lib.lago_initialize_orientations(arr, odometric, device=device),
        lambda: _lib.lago_regularized_measurements(arr, odometric, device=device),
    ]


def _replace_noise(arr, f, kind, params):
    kinds, ptr, noise = arr.f_noise_kind.copy(), [0], []
    for i in range(arr.n_factors):
        p = np.asarray(params, dtype=float) if i == f else arr.noise[arr.f_noise_ptr[i]:arr.f_noise_ptr[i + 1]]
        if i == f:
            kinds[i] = kind
        noise.append(p)
        ptr.append(ptr[-1] + p.size)
    return A.ProblemArrays(arr.var_keys, arr.var_types, arr.var_dims, arr.f_type, arr.f_rows, arr.f_key_ptr, arr.f_vars,
                           arr.f_meas_ptr, arr.meas, kinds, ptr, np.concatenate(noise), arr.values.copy())


def _refused_cases():
    v = gt.Values()
    v.insert(5, gt.Pose2())
    v.insert(ANCHOR, gt.Pose2())
    g = gt.NonlinearFactorGraph()
    g.add(gt.BetweenFactor(5, ANCHOR, gt.Pose2(1, 0, 0), gt.noiseModel.Unit.Create(3)))
    g.addPrior(5, gt.Pose2(), gt.noiseModel.Unit.Create(3))
    base = CS.two_prior_arrays()
    R = np.triu(np.full((3, 3), 0.3) + np.eye(3)).reshape(-1)
    return {
        "anchor-key collision": (g.to_arrays(v), True),
        "Gaussian model": (_replace_noise(base, 2, A.NOISE_GAUSSIAN, R), True),
        "robust model": (_replace_noise(base, 2, A.NOISE_DIAGONAL | A.NOISE_ROBUST_HUBER, [0.1, 0.1, 0.1, 1.345]), True),
        "zero sigma": (_replace_noise(base, 2, A.NOISE_DIAGONAL, [0.1, 0.1, 0.0]), True),
        "zero sigma, Constrained": (_replace_noise(base, 7, A.NOISE_CONSTRAINED, [0.0, 0.0, 0.0, 1e3, 1e3, 1e3]), False),
        "MST without a prior": (CS.no_prior_arrays(), False),
        "odometric path with a key gap": (CS.key_gap_arrays(), True),
        "odometric path over non-contiguous keys": (CS.noncontiguous_arrays(), True),
    }


@pytest.mark.parametrize("case", ["anchor-key collision", "Gaussian model", "robust model", "zero sigma",
                                  "zero sigma, Constrained", "MST without a prior", "odometric path with a key gap",
                                  "odometric path over non-contiguous keys"])
def test_refusals_before_any_device_is_touched(lib, case):
    arr, odometric = _refused_cases()[case]
    # (GSX_E_INVALID with or without a GPU, on a device index that exists or not: the checks come first)
    for device in (0, _lib.device_count()):
        for call in _calls(arr, odometric, device) + [lambda: _lib.lago_initialize_with_guess(arr, arr.values, device=device)] * odometric:
            with pytest.raises(A.GsxError) as e:
                call()
            assert e.value.status == A.GSX_E_INVALID
    with pytest.raises(A.GsxError) as e:
        _lib.lago_structure(arr, odometric)
    assert e.value.status == A.GSX_E_INVALID
    with pytest.raises((ValueError, KeyError)):      # ... and where the restatement, as the reference, throws
        LR.structure(arr, odometric)


def test_refusals_of_sizes_and_missing_guesses(lib):
    arr = CS.simple_arrays()
    desc = arr.desc()
    out = np.zeros(16)
    f = lib.gsx_lago_initialize
    f.restype = C.c_int32
    for n_out in (11, 13):
        assert f(C.byref(desc), C.c_int32(1), None, C.c_int64(0), C.c_int32(0), A._dptr(out), C.c_int64(n_out)) == A.GSX_E_INVALID
    assert f(C.byref(desc), C.c_int32(1), A._dptr(out), C.c_int64(11), C.c_int32(0), A._dptr(out), C.c_int64(12)) == A.GSX_E_INVALID
    f = lib.gsx_lago_initialize_orientations
    f.restype = C.c_int32
    assert f(C.byref(desc), C.c_int32(1), C.c_int32(0), A._dptr(out), C.c_int64(5)) == A.GSX_E_INVALID
    f = lib.gsx_lago_regularized_measurements
    f.restype = C.c_int32
    assert f(C.byref(desc), C.c_int32(1), C.c_int32(0), A._dptr(out), C.c_int64(5)) == A.GSX_E_INVALID
    with pytest.raises(A.GsxError) as e:            # lago::initialize(graph, initialGuess) without a guess
        _lib.lago_initialize_with_guess(arr, None)
    assert e.value.status == A.GSX_E_INVALID
    # a variable that is not POSE2, a pose no used factor holds: there must be a guess to copy them from
    for lonely in (CS.simple_arrays("rot"), CS.graph_file_arrays("example.graph")):
        with pytest.raises(A.GsxError) as e:
            _lib.lago_initialize(lonely, False, None)
        assert e.value.status == A.GSX_E_INVALID
    # the forest of gsx_lago_thetas_to_root: a link out of range, a cycle
    for parent in ([0, 5, 1], [0, 2, 1], [-1, 0]):
        with pytest.raises(A.GsxError) as e:
            _lib.lago_thetas_to_root(np.array(parent, np.int32), np.zeros(len(parent)))
        assert e.value.status == A.GSX_E_INVALID


def test_numeric_entry_points_need_a_device(lib):
    # device 0 where no GPU is visible; where some are, the first index that is none of them
    arr = CS.simple_arrays()
    device = _lib.device_count()
    calls = _calls(arr, True, device) + _calls(arr, False, device) + [
        lambda: _lib.lago_initialize_with_guess(arr, arr.values, device=device),
        lambda: _lib.lago_thetas_to_root(np.array([0, 0, 1], np.int32), np.array([0.0, 1.0, 2.0]), device=device)]
    for call in calls:
        with pytest.raises(A.GsxError) as e:
            call()
        assert e.value.status == A.GSX_E_NO_DEVICE


def test_build_pose2_graph_drops_other_factors_and_anchors_priors():
    g = CS.simple_graph("rot")
    g.add(gt.BetweenFactor(gt.symbol("l", 1), gt.symbol("l", 2), gt.Point2(1, 0), gt.noiseModel.Unit.Create(2)))
    g.add(gt.RangeFactor(X[0], X[1], 2.0, gt.noiseModel.Unit.Create(1)))
    pg = gt.lago.buildPose2graph(g)
    assert pg.size() == 6
    assert [f.keys() for f in pg.factors][:5] == [[X[a], X[b]] for a, b in ((0, 1), (1, 2), (2, 3), (2, 0), (0, 3))]
    last = pg.factors[5]
    assert last.ftype == A.F_BETWEEN and last.keys() == [ANCHOR, X[0]] and last.noise.params[0] == 0.1


def test_lago_host_code_under_address_sanitizer(golden_dir, tmp_path):
    """The host part of lago (csrc/lago_graph.cpp) as a stand-alone program under g++ -fsanitize=address,undefined: both
    trees on the 2-D golden files and on a 100 000-pose chain, the two lowerings, the refusals."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "gtsam_petercdev_amd", "csrc")
    exe = tmp_path / "lago_sanitize"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(root, "tests", "native", "lago_sanitize.cpp")] + \
          [os.path.join(src, f) for f in ("lago_graph.cpp", "init_graph.cpp", "problem.cpp", "io.cpp")] + ["-o", str(exe)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe), golden_dir], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    assert run.stdout.count(" ok") == 5, run.stdout


def test_stage_timings_entry_point_and_probe_host_path(lib):
    """gsx_lago_timings refuses a wrong length or a NULL array and names eight stages; tools/lago_probe.py builds its graph
    and the tree without a device."""
    f = lib.gsx_lago_timings
    f.restype = C.c_int32
    out = np.zeros(8)
    assert f(A._dptr(out), C.c_int32(7)) == A.GSX_E_INVALID and f(None, C.c_int32(8)) == A.GSX_E_INVALID
    assert set(_lib.lago_timings()) == set(_lib.LAGO_TIMING_NAMES) and len(_lib.LAGO_TIMING_NAMES) == 8
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, os.path.join(root, "tools", "lago_probe.py"), "--poses", "300", "--host-only"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    assert rec["n_poses"] == 300 and rec["device"] is None and rec["max_depth"] == 300
    assert rec["n_tree_edges"] + rec["n_chords"] == rec["n_edges"] and rec["rounds"] == 9
