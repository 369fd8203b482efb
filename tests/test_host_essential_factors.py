"""The restatements of tests/_essential_restatement.py (float64) and tests/_mp_essential_restatement.py (50 digits), pinned
by the reference's own known answers (gtsam/geometry/tests/testUnit3.cpp, testEssentialMatrix.cpp,
gtsam/slam/tests/testEssentialMatrixFactor.cpp) and by the true derivatives of the 50-digit error.  No GPU."""
import math

import numpy as np
import pytest

from gtsam_petercdev_amd import _abi as A
from gtsam_petercdev_amd import graph as G
from tests import _essential_restatement as S
from tests import _factor_restatement as R
from tests import _mp_essential_restatement as MS

TRUE_H = ("essential", "depth", "depth_rotated", "calib")   # the others state an identity for a Local derivative


def test_unit3_basis_and_charts_known_answers():
    """testUnit3.cpp: retract of (1, 0, 0) by (0.5, 0) and by (0, 0) (:363-378); localCoordinates round trips (:437-470);
    the antipode answers (pi, 0) (Unit3.cpp:297)."""
    p = np.array([1.0, 0.0, 0.0])
    assert np.allclose(S.unit3_retract(p, [0.0, 0.0]), p, atol=1e-8)
    q = S.unit3_retract(p, [0.5, 0.0])
    B = S.unit3_basis(p)
    assert np.allclose(q, math.cos(0.5) * p + math.sin(0.5) * B[:, 0], atol=1e-8)
    assert np.allclose(S.unit3_local(p, q), [0.5, 0.0], atol=1e-8)
    assert np.array_equal(S.unit3_local(p, -p), [math.pi, 0.0])
    rng = np.random.default_rng(1)
    for _ in range(20):
        p, v = S.unit(rng), rng.uniform(-1.2, 1.2, 2)
        q = S.unit3_retract(p, v)
        assert abs(np.linalg.norm(q) - 1) < 1e-15
        assert np.allclose(S.unit3_local(p, q), v, atol=1e-12)
        assert np.allclose(MS.local(S.UNIT3, p, MS.retract(S.UNIT3, p, v)), v, atol=1e-14)
        assert np.allclose(G.Unit3(p).retract(v).point3(), q, atol=1e-15)
        assert np.allclose(G.Unit3(p).localCoordinates(G.Unit3(q)), v, atol=1e-12)


def test_essential_matrix_known_answers():
    """testEssentialMatrix.cpp: E = [t]x R (:43-49); retract by zero is the identity and retract / localCoordinates round
    trip (:63-83); FromPose3 normalises the translation (:98-113); rotate (:117-141): the rotated matrix is cRb E cRb'."""
    Rm = G.Rot3.Ypr(0.1, -0.2, 0.3)
    E = G.EssentialMatrix(Rm, G.Unit3(0.1, 0.0, 0.0))
    assert np.allclose(E.matrix(), R.skew([1.0, 0, 0]) @ Rm.matrix(), atol=1e-8)
    assert E.retract(np.zeros(5)).equals(E, 1e-8)
    xi = np.array([0.1, -0.2, 0.3, 0.2, -0.1])
    assert np.allclose(E.localCoordinates(E.retract(xi)), xi, atol=1e-8)
    assert np.allclose(S.local(S.ESSENTIAL, E.state(), S.retract(S.ESSENTIAL, E.state(), xi)), xi, atol=1e-8)
    assert np.allclose(MS.local(S.ESSENTIAL, E.state(), MS.retract(S.ESSENTIAL, E.state(), xi)), xi, atol=1e-12)
    assert np.allclose(E.retract(xi).state(), MS.retract(S.ESSENTIAL, E.state(), xi), atol=1e-14)
    assert G.EssentialMatrix.FromPose3(G.Pose3(Rm, [0.1, 0, 0])).equals(E, 1e-8)
    cRb = G.Rot3.Ypr(0.5, 0.3, -0.2)
    assert np.allclose(E.rotate(cRb).matrix(), cRb.matrix() @ E.matrix() @ cRb.matrix().T, atol=1e-8)


def five_point_graph(state):
    trueE, pA, pB, _ = S.bal_two_view("18pointExample1.txt")
    facs = [(S.F_E, [0], 1, np.concatenate([pA[i], [1.0], pB[i], [1.0]]), A.NOISE_ISOTROPIC, [0.01]) for i in range(5)]
    return R.make_arrays([(1, S.ESSENTIAL, 5)], facs, trueE if state is None else state), trueE, pA, pB


def test_five_point_data_and_graph_errors():
    """testEssentialMatrixFactor.cpp:56-79 (the data), :166-184: with Isotropic::Sigma(1, 0.01) the graph error is 0 at truth
    within 1e-8 and 643.26 within 1e-2 at trueE.retract((0.1, -0.1, 0.1, 0.1, -0.1)) (the Expmap-chart value)."""
    arr, trueE, pA, pB = five_point_graph(None)
    assert np.allclose(R.skew(0.1 * trueE[9:12]) @ trueE[:9].reshape(3, 3), [[0, 0, 0], [0, 0, -0.1], [0.1, 0, 0]], atol=1e-8)
    assert np.allclose(pA[0], [0, 0], atol=1e-8) and np.allclose(pB[0], [0, 0.1], atol=1e-8)
    assert np.allclose(pA[4], [0, -1], atol=1e-8) and np.allclose(pB[4], [-1, 0.2], atol=1e-8)
    xi = np.array([0.1, -0.1, 0.1, 0.1, -0.1])
    for mod in (S, MS):
        assert abs(mod.graph_error(arr, trueE)) <= 1e-8
        assert abs(mod.graph_error(arr, mod.retract(S.ESSENTIAL, trueE, xi)) - 643.26) <= 1e-2


@pytest.mark.parametrize("form", S.FORMS)
def test_restated_jacobians(form):
    """float64 against 50 digits, and the 50-digit Jacobians against central differences of the 50-digit error where the
    reference states the true derivative (the tolerances of test_host_absolute_factors.py)."""
    arr, _ = S.random_graph([form], 6, "unit", seed=40 + S.FORMS.index(form))
    for f in range(arr.n_factors):
        e, Hs, _ = S.evaluate(arr, arr.values, f)
        em, Hm, _ = MS.evaluate(arr, arr.values, f)
        scale = max(1.0, max(float(np.max(np.abs(H))) for H in Hm))
        assert np.allclose(e, em, rtol=0, atol=1e-13 * max(1.0, float(np.max(np.abs(em)))))
        for H, Hq in zip(Hs, Hm):
            assert H.shape == Hq.shape and np.allclose(H, Hq, rtol=0, atol=1e-13 * scale)
        if form in TRUE_H:
            for Hq, Ht in zip(Hm, MS.true_jacobians(arr, arr.values, f)):
                assert np.allclose(Hq, Ht, rtol=0, atol=1e-12 * scale), (form, f)


def test_factor3_with_identity_is_factor2():
    arr, _ = S.random_graph(["depth"], 4, "unit", seed=7)
    for f in range(4):
        e2, H2, _ = MS.evaluate(arr, arr.values, f)
        rot = R.make_arrays([(0, S.ESSENTIAL, 5), (1, A.VAR_VECTOR, 1)],
                            [(S.F_E_DEPTH, [0, 1], 2, np.concatenate([R.factor_parts(arr, f)[2], np.eye(3).reshape(9)]), A.NOISE_UNIT, [])],
                            arr.values[arr.state_offsets()[2 * f]:arr.state_offsets()[2 * f + 2]])
        e3, H3, _ = MS.evaluate(rot, rot.values, 0)
        assert np.allclose(e2, e3, atol=1e-15) and all(np.allclose(a, b, atol=1e-14) for a, b in zip(H2, H3))


def test_constraint_is_zero_at_truth():
    """testEssentialMatrixConstraint.cpp: the error of the measured E of the relative pose itself is 0."""
    rng = np.random.default_rng(3)
    x1, x2 = (R.pose3_state(S.S.big_rot3(rng), rng.normal(size=3)) for _ in range(2))
    R1, t1 = R.pose3_of(x1)
    R2, t2 = R.pose3_of(x2)
    th = R1.T @ (t2 - t1)
    z = np.concatenate([(R1.T @ R2).reshape(9), th / np.linalg.norm(th)])
    arr = R.make_arrays([(0, A.VAR_POSE3, 6), (1, A.VAR_POSE3, 6)], [(S.F_E_CONSTRAINT, [0, 1], 5, z, A.NOISE_UNIT, [])],
                        np.concatenate([x1, x2]))
    assert np.max(np.abs(MS.evaluate(arr, arr.values, 0)[0])) <= 1e-15


def test_validation_and_chart_header_under_address_sanitizer(tmp_path):
    """tests/native/essential_sanitize.cpp: problem.cpp's validation of the new types and csrc/unit3_math.h (basis, both
    charts, every branch) compiled with g++ -fsanitize=address,undefined as a stand-alone program and run on the CPU."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "essential_sanitize"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(root, "tests", "native", "essential_sanitize.cpp"),
           os.path.join(root, "gtsam_petercdev_amd", "csrc", "problem.cpp"), "-o", str(exe)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert run.returncode == 0 and "essential_sanitize: 0 failures" in run.stdout, (run.stdout[-1500:], run.stderr[-3000:])
