"""InitializePose3 without a GPU: the restatement tests/_init_pose3_restatement.py reproduces the reference's known answers
(gtsam/slam/tests/testInitializePose3.cpp, at the reference's own tolerances), and the host side of the C ABI — the pose
graph structure, the refusals that come before any device is touched — behaves as include/gsx.h says."""
import ctypes as C
import os
import json
import subprocess
import sys

import numpy as np
import pytest

import gtsam_petercdev_amd as gt
from gtsam_petercdev_amd import _abi as A, _lib
from tests import _factor_restatement as FR
from tests import _init_pose3_cases as CS
from tests import _init_pose3_restatement as IR


@pytest.fixture(scope="module")
def lib():
    from gtsam_petercdev_amd import build
    build.build_lib()
    return _lib.load()


def _state_rot(values, arr, v):
    so = arr.state_offsets()
    return values[so[v]:so[v] + 9].reshape(3, 3)


# ---- the restatement against the reference's known answers ------------------------------------------------------------
@pytest.mark.parametrize("second", [False, True], ids=["orientations", "orientationsPrecisions"])
def test_restatement_chordal_orientations(second):
    rot = IR.chordal(CS.simple_arrays(second))
    for i in range(4):
        assert np.abs(rot[i] - CS.SIMPLE_R[i]).max() < 1e-6, i


def test_restatement_single_gradient():
    R2 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    g = IR.gradient_tron(np.eye(3), R2, 6.010534238540223, 1.0)
    assert np.abs(g - np.array([0.0, 0.0, 1.962658662803917])).max() < 1e-6


def test_restatement_iteration_gradient():
    arr = CS.simple_arrays(poses=CS.perturbed_guess())
    rot, it, _, _ = IR.orientations_gradient(arr, arr.values, 1, False)
    assert it == 1
    for i in range(4):
        assert np.abs(rot[i] - CS.ITERATION_GRADIENT[i]).max() < 1e-5, i


def test_restatement_orientations_gradient_ten_iterations():
    arr = CS.simple_arrays(poses=CS.perturbed_guess())
    rot, _, _, _ = IR.orientations_gradient(arr, arr.values, 10, False)
    for i, (R, tol) in enumerate(zip(CS.gradient10_expected(), CS.GRADIENT10_TOL)):
        assert np.abs(rot[i] - R).max() < tol, i


def test_restatement_poses_with_given_guess():
    arr = CS.simple_arrays()
    out = IR.initialize(arr, arr.values)
    assert np.abs(out - arr.values).max() < 1e-6


def test_restatement_initialize_poses_grid():
    arr = CS.grid_arrays()
    out = IR.initialize(arr)
    assert np.abs(out - arr.values).max() < 0.1


# ---- the host side of the C ABI -------------------------------------------------------------------------------------------
def test_init_structure_of_simple_graph(lib):
    ef, et, adj = _lib.pose3_init_structure(CS.simple_arrays())
    assert len(adj) == 5                       # 4 poses and the anchor
    assert adj[0] == [0, 3, 4, 5] and adj[1] == [0, 1] and adj[2] == [1, 2, 3] and adj[3] == [2, 4]
    assert adj[4] == [5]
    assert ef.tolist() == [0, 1, 2, 2, 0, 4] and et.tolist() == [1, 2, 3, 0, 3, 0]   # the prior: from the anchor
    # the same through the Python interface, by key
    m, rots = gt.InitializePose3.createSymbolicGraph(gt.InitializePose3.buildPose3graph(CS.simple_graph()))
    assert m[CS.X[0]] == [0, 3, 4, 5] and m[CS.X[2]] == [1, 2, 3] and len(m) == 5 and m[A.ANCHOR_KEY] == [5]
    assert len(rots) == 6


def test_init_structure_needs_room_for_the_adjacency(lib):
    arr = CS.simple_arrays()
    desc = arr.desc()
    f = lib.gsx_pose3_init_structure
    f.restype = C.c_int32
    adj = np.zeros(12, np.int32)
    st = f(C.byref(desc), None, None, None, None, adj.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int64(11))
    assert st == A.GSX_E_INVALID


def _numeric_calls(arr, given, device=0):
    P = int(np.count_nonzero(arr.var_types == A.VAR_POSE3))
    return [
        lambda: _lib.initialize_pose3(arr, given, device=device),
        lambda: _lib.pose3_orientations_chordal(arr, device=device),
        lambda: _lib.pose3_orientations_gradient(arr, given, 5, True, device=device),
        lambda: _lib.pose3_compute_poses(arr, np.tile(np.eye(3), (P, 1, 1)), device=device),
        lambda: _lib.closest_rotations(np.eye(3).reshape(1, 3, 3), device=device),
    ]


def test_numeric_entry_points_need_a_device(lib):
    # device 0 where no GPU is visible; where some are, the first index that is none of them
    arr = CS.simple_arrays()
    for call in _numeric_calls(arr, arr.values, device=_lib.device_count()):
        with pytest.raises(A.GsxError) as e:
            call()
        assert e.value.status == A.GSX_E_NO_DEVICE


def test_refusals_before_any_device_is_touched(lib):
    # (GSX_E_INVALID with or without a GPU: the checks come first)
    arr = CS.simple_arrays()
    # a variable that carries the anchor's key
    v = gt.Values()
    v.insert(5, gt.Pose3())
    v.insert(A.ANCHOR_KEY, gt.Pose3())
    g = gt.NonlinearFactorGraph()
    g.add(gt.BetweenFactor(5, A.ANCHOR_KEY, gt.Pose3(), gt.noiseModel.Unit.Create(6)))
    g.addPrior(5, gt.Pose3(), gt.noiseModel.Unit.Create(6))
    clash = g.to_arrays(v)
    for call in _numeric_calls(clash, clash.values)[:4]:
        with pytest.raises(A.GsxError) as e:
            call()
        assert e.value.status == A.GSX_E_INVALID
    with pytest.raises(A.GsxError) as e:
        _lib.pose3_init_structure(clash)
    assert e.value.status == A.GSX_E_INVALID
    # the gradient needs a guess
    p = _lib.init_pose3_params_default()
    assert (p.use_gradient, p.max_gradient_iterations, p.set_ref_frame, p.single_iter) == (0, 10000, 1, 1)
    p.use_gradient = 1
    with pytest.raises(A.GsxError) as e:
        _lib.initialize_pose3(arr, None, p)
    assert e.value.status == A.GSX_E_INVALID
    with pytest.raises(A.GsxError) as e:
        _lib.pose3_orientations_gradient(arr, None, 5, True)
    assert e.value.status == A.GSX_E_INVALID
    # a wrong n_out
    desc = arr.desc()
    out = np.zeros(48)
    for n_out in (47, 36):
        f = lib.gsx_initialize_pose3
        f.restype = C.c_int32
        assert f(C.byref(desc), None, C.c_int64(0), None, C.c_int32(0), A._dptr(out), C.c_int64(n_out), None) == A.GSX_E_INVALID
    f = lib.gsx_pose3_orientations_chordal
    f.restype = C.c_int32
    assert f(C.byref(desc), C.c_int32(0), A._dptr(out), C.c_int64(35)) == A.GSX_E_INVALID
    f = lib.gsx_pose3_compute_poses
    f.restype = C.c_int32
    rot = np.tile(np.eye(3).reshape(9), 4)
    assert f(C.byref(desc), A._dptr(rot), C.c_int64(36), C.c_int32(1), C.c_int32(0), A._dptr(out), C.c_int64(47)) == A.GSX_E_INVALID
    assert f(C.byref(desc), A._dptr(rot), C.c_int64(27), C.c_int32(1), C.c_int32(0), A._dptr(out), C.c_int64(48)) == A.GSX_E_INVALID
    # a pose no used factor holds, and no guess to copy it from
    v = CS.simple_values()
    v.insert(gt.symbol("x", 9), gt.Pose3())
    lonely = CS.simple_graph().to_arrays(v)
    with pytest.raises(A.GsxError) as e:
        _lib.initialize_pose3(lonely, None)
    assert e.value.status == A.GSX_E_INVALID


def test_build_pose3_graph_drops_other_factors_and_anchors_priors():
    g = CS.simple_graph()
    g.add(gt.BetweenFactor(gt.symbol("l", 1), gt.symbol("l", 2), gt.Point3(1, 0, 0), gt.noiseModel.Unit.Create(3)))
    g.add(gt.PriorFactor(gt.symbol("l", 1), gt.Point3(0, 0, 0), gt.noiseModel.Unit.Create(3)))
    g.add(gt.RangeFactor(CS.X[0], CS.X[1], 2.0, gt.noiseModel.Unit.Create(1)))
    pg = gt.InitializePose3.buildPose3graph(g)
    assert pg.size() == 6
    assert [f.keys() for f in pg.factors][:5] == [[CS.X[a], CS.X[b]] for a, b in ((0, 1), (1, 2), (2, 3), (2, 0), (0, 3))]
    last = pg.factors[5]
    assert last.ftype == A.F_BETWEEN and last.keys() == [99999999, CS.X[0]]
    assert last.noise.kind == A.NOISE_ISOTROPIC and last.noise.params[0] == 0.1
    assert np.abs(last.meas - FR.pose3_state(CS.SIMPLE_R[0], CS.SIMPLE_P[0])).max() == 0.0


def test_initializer_host_code_under_address_sanitizer(golden_dir, tmp_path):
    """The host lowering of the initializer (csrc/init_graph.cpp) and the arithmetic its kernels run (csrc/init_math.h,
    compiled for the host) as a stand-alone program under g++ -fsanitize=address,undefined on the 3-D golden files; the same
    program's Rot3::ClosestTo holds the bound of the device test (8 x max(LAPACK's float64 error, 2^-52) per matrix)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "gtsam_petercdev_amd", "csrc")
    exe = tmp_path / "init_sanitize"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(root, "tests", "native", "init_sanitize.cpp")] + \
          [os.path.join(src, f) for f in ("init_graph.cpp", "problem.cpp", "io.cpp")] + ["-o", str(exe)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    Ms = CS.closest_rotation_cases()
    np.savetxt(tmp_path / "matrices.txt", Ms.reshape(-1, 9), fmt="%.17g")
    run = subprocess.run([str(exe), golden_dir, str(tmp_path / "matrices.txt")], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    assert run.stdout.count(" ok") == 4
    R = np.array([[float(x) for x in l.split()[1:]] for l in run.stdout.splitlines() if l.startswith("R ")]).reshape(-1, 3, 3)
    assert len(R) == len(Ms)
    for M, Rd in zip(Ms, R):
        Rm = IR.mp_to_np(IR.closest_rotation_mp(M)[0])
        bound = 8 * max(np.abs(IR.closest_rotation_np(M) - Rm).max(), 2.0 ** -52)
        assert np.abs(Rd - Rm).max() <= bound
        assert np.abs(Rd.T @ Rd - np.eye(3)).max() <= 32 * 2.0 ** -52 and np.linalg.det(Rd) > 0


def test_stage_timings_entry_point_and_probe_host_path(lib):
    """gsx_pose3_init_timings refuses a wrong length or a NULL array and names eight stages; tools/init_probe.py builds its
    graph and the pose-graph structure without a device."""
    f = lib.gsx_pose3_init_timings
    f.restype = C.c_int32
    out = np.zeros(8)
    assert f(A._dptr(out), C.c_int32(7)) == A.GSX_E_INVALID and f(None, C.c_int32(8)) == A.GSX_E_INVALID
    assert set(_lib.pose3_init_timings()) == set(_lib.INIT_TIMING_NAMES)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, os.path.join(root, "tools", "init_probe.py"), "--poses", "300", "--host-only"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    assert rec["n_poses"] == 300 and rec["device"] is None and rec["n_edges"] == rec["n_factors"] and rec["max_node_degree"] >= 2
