"""The restatements of the absolute-measurement factors and of the Rot3 variable (tests/_absolute_restatement.py, float64;
tests/_mp_absolute_restatement.py, 50 digits) pinned by the reference's own known answers and by the true derivative of the
50-digit error; and the ABI constants and Python classes that carry them.  No device."""
import math
import os
import re

import numpy as np
import pytest

from gtsam_petercdev_amd import _abi as A
from gtsam_petercdev_amd import graph as G
from tests import _absolute_restatement as S
from tests import _factor_restatement as R
from tests import _mp_absolute_restatement as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one_factor(factor, key_values):
    g, v = G.NonlinearFactorGraph(), G.Values()
    g.add(factor)
    for k, x in key_values:
        v.insert(k, x)
    return g.to_arrays(v)


def e_H(arr, evaluate=S.evaluate):
    e, Hs, _ = evaluate(arr, arr.values, 0)
    return e, Hs


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_the_header_and_the_python_mirror_agree_on_the_new_enums():
    text = open(os.path.join(ROOT, "include", "gsx.h")).read()
    for name, value in (("GSX_VAR_ROT3", A.VAR_ROT3), ("GSX_F_GPS", A.F_GPS),
                        ("GSX_F_POSE_TRANSLATION_PRIOR", A.F_POSE_TRANSLATION_PRIOR),
                        ("GSX_F_POSE_ROTATION_PRIOR", A.F_POSE_ROTATION_PRIOR), ("GSX_F_ATTITUDE", A.F_ATTITUDE),
                        ("GSX_F_MAG", A.F_MAG)):
        m = re.search(r"\b%s = (\d+)" % name, text)
        assert m and int(m.group(1)) == value, name
    assert (A.VAR_ROT3, A.F_GPS, A.F_MAG) == (4, 13, 17)
    assert A.STATE_DIM[A.VAR_ROT3] == 9 and A.TANGENT_DIM[A.VAR_ROT3] == 3
    assert (S.ROT3, S.F_GPS, S.F_TRANS, S.F_ROT, S.F_ATT, S.F_MAG) == (
        A.VAR_ROT3, A.F_GPS, A.F_POSE_TRANSLATION_PRIOR, A.F_POSE_ROTATION_PRIOR, A.F_ATTITUDE, A.F_MAG)


def test_rot3_values_round_trip_through_the_arrays():
    v = G.Values()
    v.insert(3, G.Rot3.Rodrigues(0.1, -0.2, 0.3))
    v.insert(1, G.Pose2(1, 2, 0.3))
    g = G.NonlinearFactorGraph()
    g.add(G.PriorFactorRot3(3, G.Rot3(), G.noiseModel.Isotropic.Sigma(3, 0.1)))
    arr = g.to_arrays(v)
    assert list(arr.var_types) == [A.VAR_POSE2, A.VAR_ROT3] and list(arr.state_offsets()) == [0, 3, 12]
    back = G.Values.unpack(arr.var_keys, arr.var_types, arr.var_dims, arr.values)
    assert isinstance(back.atRot3(3), G.Rot3) and np.array_equal(back.atRot3(3).matrix(), v.atRot3(3).matrix())


# ---- known answers --------------------------------------------------------------------------------------------------------
def test_gps_known_answers():
    """testGPSFactor.cpp:54-153: zero error where the translation (plus R bL for the arm forms) equals the fix; H."""
    nRb = G.Rot3.RzRyRx(0.15, -0.30, 0.45)
    nT = np.array([-5.0, 8.0, -11.0])
    bL = np.array([0.3, -0.2, 0.1])
    model = G.noiseModel.Isotropic.Sigma(3, 0.25)
    pose = G.Pose3(nRb, nT)
    e, Hs = e_H(one_factor(G.GPSFactor(1, nT, model), [(1, pose)]))
    assert np.allclose(e, 0, atol=1e-15) and np.allclose(Hs[0], np.hstack([np.zeros((3, 3)), nRb.matrix()]))
    body = G.Pose3(nRb, nT - nRb.matrix() @ bL)
    e, Hs = e_H(one_factor(G.GPSFactorArm(1, nT, bL, model), [(1, body)]))
    assert np.allclose(e, 0, atol=1e-14)
    e2, Hs2 = e_H(one_factor(G.GPSFactorArmCalib(1, 2, nT, model), [(1, body), (2, bL)]))
    assert np.allclose(e2, 0, atol=1e-14) and np.array_equal(Hs2[0], Hs[0]) and np.allclose(Hs2[1], nRb.matrix())
    arr = one_factor(G.GPSFactorArm(1, nT, bL, model), [(1, body)])
    assert len(arr.meas) == 6 and len(one_factor(G.GPSFactor(1, nT, model), [(1, pose)]).meas) == 3


def test_attitude_known_answers():
    """testAttitudeFactor.cpp:33-114: nDown = (0, 0, -1), bMeasured the body Z axis: zero error at the identity, for the
    Rot3 and the Pose3 form, whose translation columns are zero."""
    model = G.noiseModel.Isotropic.Sigma(2, 0.25)
    nDown = G.Unit3(0.0, 0.0, -1.0)
    a0 = one_factor(G.Rot3AttitudeFactor(1, nDown, model), [(1, G.Rot3())])
    a1 = one_factor(G.Rot3AttitudeFactor(1, nDown, model, G.Unit3(0.0, 0.0, 1.0)), [(1, G.Rot3())])
    assert np.array_equal(a0.meas, a1.meas) and np.array_equal(a0.meas, [0, 0, -1, 0, 0, 1])
    e, Hs = e_H(a0)
    assert np.allclose(e, 0, atol=1e-15) and Hs[0].shape == (2, 3)
    p = one_factor(G.Pose3AttitudeFactor(1, nDown, model), [(1, G.Pose3(G.Rot3(), [-5.0, 8.0, -11.0]))])
    e, Hp = e_H(p)
    assert np.allclose(e, 0, atol=1e-15) and Hp[0].shape == (2, 6) and np.array_equal(Hp[0][:, :3], Hs[0])
    assert not Hp[0][:, 3:].any()
    # :51-62, :100-114: the factor's H at that point equals the numerical derivative to 1e-8 — here the true derivative of
    # the 50-digit error — for both forms
    for arr, H in ((a0, Hs[0]), (p, Hp[0])):
        assert np.allclose(H, MS.true_jacobians(arr, arr.values, 0)[0], rtol=0, atol=1e-8)
        assert np.allclose(MS.evaluate(arr, arr.values, 0)[1][0], H, rtol=0, atol=1e-15)


def test_unit3_basis_known_answer():
    """testUnit3.cpp:318-329: the basis of Unit3(0.1, -0.2, 0.9) to 1e-6."""
    n = np.array([0.1, -0.2, 0.9])
    n = n / np.linalg.norm(n)
    want = np.array([[0.0, -0.994169047], [0.97618706, -0.0233922129], [0.216930458, 0.105264958]])
    assert np.allclose(S.unit3_basis(n), want, rtol=0, atol=1e-6)
    assert np.allclose([[float(x) for x in row] for row in MS.unit3_basis(MS.M.vec(n))], want, rtol=0, atol=1e-6)


NM = np.array([22653.29982, -1956.83010, 44202.47862])
SCALE = 255.0 / 50000.0
BIAS = np.array([10.0, -10.0, 50.0])


def test_magfactor1_known_answer():
    """testMagFactor.cpp:67-81: measured = nRb^-1 (scale nM) + bias gives a zero error at nRb = Yaw(-0.1)."""
    nRb = G.Rot3.Ypr(-0.1, 0.0, 0.0)
    measured = nRb.unrotate(SCALE * NM) + BIAS
    f = G.MagFactor1(1, measured, SCALE * np.linalg.norm(NM), G.Unit3(NM), BIAS, G.noiseModel.Isotropic.Sigma(3, 0.25))
    e, _ = e_H(one_factor(f, [(1, nRb)]))
    assert np.allclose(e, 0, atol=1e-5)
    assert abs(nRb.unrotate(NM)[0] - 22735.5) < 1e-1 and abs(nRb.unrotate(NM)[1] - 314.502) < 1e-1   # :60


def test_magposefactor_known_answers():
    """testMagPoseFactor.cpp:74-125: zero error at the true pose, without and with body_P_sensor, 2-D and 3-D."""
    dir3, dir2 = np.array([1.0, 2.0, 3.0]), np.array([1.0, 0.0])
    bias3, bias2 = np.array([0.1, 0.2, 0.3]), np.array([0.1, -0.2])
    scale = 4.0
    n_P3 = G.Pose3(G.Rot3.RzRyRx(-0.4, 0.6, -0.1), [-4.0, 7.0, 3.0])
    n_P2 = G.Pose2(-4.0, 7.0, 0.4)
    m3, m2 = G.noiseModel.Isotropic.Sigma(3, 0.25), G.noiseModel.Isotropic.Sigma(2, 0.25)
    z3 = n_P3.rotation().unrotate(scale * dir3 / np.linalg.norm(dir3)) + bias3
    z2 = R.rot2(0.4).T @ (scale * dir2) + bias2
    assert np.allclose(e_H(one_factor(G.MagPoseFactorPose3(1, z3, scale, dir3, bias3, m3), [(1, n_P3)]))[0], 0, atol=1e-14)
    assert np.allclose(e_H(one_factor(G.MagPoseFactorPose2(1, z2, scale, dir2, bias2, m2), [(1, n_P2)]))[0], 0, atol=1e-14)
    # the sensor measures in its own frame: sensor reading = sRb (body field - 0) with bias in the sensor frame
    bPs3 = G.Pose3(G.Rot3.RzRyRx(0.2, -0.3, 0.5), [1.0, 2.0, 3.0])
    sR = bPs3.rotation().matrix()
    zs3 = sR.T @ n_P3.rotation().unrotate(scale * dir3 / np.linalg.norm(dir3)) + bias3
    f = G.MagPoseFactorPose3(1, zs3, scale, dir3, bias3, m3, bPs3)
    assert np.allclose(e_H(one_factor(f, [(1, n_P3)]))[0], 0, atol=1e-14)
    assert np.allclose(f.meas[:3], sR @ zs3) and np.allclose(f.meas[6:], sR @ bias3)
    bPs2 = G.Pose2(1.0, 2.0, -0.7)
    zs2 = R.rot2(-0.7).T @ (R.rot2(0.4).T @ (scale * dir2)) + bias2
    f = G.MagPoseFactorPose2(1, zs2, scale, dir2, bias2, m2, bPs2)
    assert np.allclose(e_H(one_factor(f, [(1, n_P2)]))[0], 0, atol=1e-14)


def test_pose_part_priors_known_answers():
    """testPoseTranslationPrior.cpp / testPoseRotationPrior.cpp: level, rotated and translated poses."""
    t3, t2 = np.array([1.0, 2.0, 3.0]), np.array([1.0, 2.0])
    rot3 = G.Rot3.RzRyRx(0.1, 0.2, 0.3)
    m3, m2, m1 = (G.noiseModel.Isotropic.Sigma(n, 0.1) for n in (3, 2, 1))
    for pose, want_e in ((G.Pose3(G.Rot3(), t3), np.zeros(3)), (G.Pose3(rot3, t3), np.zeros(3)),
                         (G.Pose3(rot3, t3 + [0.1, -0.2, 0.3]), np.array([0.1, -0.2, 0.3]))):
        e, Hs = e_H(one_factor(G.PoseTranslationPrior3D(1, t3, m3), [(1, pose)]))
        assert np.allclose(e, want_e, atol=1e-15)
        assert np.array_equal(Hs[0], np.hstack([np.zeros((3, 3)), pose.rotation().matrix()]))
    for pose, want_e in ((G.Pose2(1.0, 2.0, 0.0), np.zeros(2)), (G.Pose2(1.0, 2.0, 0.7), np.zeros(2)),
                         (G.Pose2(1.5, 1.0, 0.7), np.array([0.5, -1.0]))):
        e, Hs = e_H(one_factor(G.PoseTranslationPrior2D(1, t2, m2), [(1, pose)]))
        assert np.allclose(e, want_e, atol=1e-15) and np.allclose(Hs[0], np.hstack([R.rot2(pose.theta()), np.zeros((2, 1))]))
    for pose in (G.Pose3(rot3, t3), G.Pose3(rot3, 2 * t3)):
        e, Hs = e_H(one_factor(G.PoseRotationPrior3D(1, rot3, m3), [(1, pose)]))
        assert np.allclose(e, 0, atol=1e-15) and np.array_equal(Hs[0], np.hstack([np.eye(3), np.zeros((3, 3))]))
    e, _ = e_H(one_factor(G.PoseRotationPrior3D(1, rot3, m3), [(1, G.Pose3(rot3.compose(G.Rot3.Rodrigues(0.1, 0.2, 0.3)), t3))]))
    assert np.allclose(e, [0.1, 0.2, 0.3], atol=1e-14)
    e, Hs = e_H(one_factor(G.PoseRotationPrior2D(1, 0.2, m1), [(1, G.Pose2(3.0, 4.0, 0.5))]))
    assert np.allclose(e, [0.3], atol=1e-15) and np.array_equal(Hs[0], [[0.0, 0.0, 1.0]])
    e, _ = e_H(one_factor(G.PoseRotationPrior2D(1, -3.0, m1), [(1, G.Pose2(3.0, 4.0, 3.0))]))   # wrapped
    assert np.allclose(e, [6.0 - 2 * math.pi], atol=1e-14)


# ---- Unit3::basis ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, axis", [((0.1, 0.7, 0.7), 0), ((0.7, 0.1, 0.7), 1), ((0.7, 0.7, 0.1), 2),
                                     ((1, 0, 0), 1), ((0, 1, 0), 0), ((0, 0, 1), 0),
                                     ((1, 1, 2), 0), ((2, 1, 1), 1), ((1, 2, 1), 0), ((1, 1, 1), 0)])
def test_unit3_basis(n, axis):
    """testUnit3.cpp's basis properties with one direction per branch of CalculateBestAxis and its ties: B'B = I, B'n = 0,
    b1 = normalize(n x axis), b2 = n x b1."""
    n = np.array(n, float) / np.linalg.norm(n)
    assert S.best_axis(n) == axis
    B = S.unit3_basis(n)
    assert np.allclose(B.T @ B, np.eye(2), atol=1e-15) and np.allclose(B.T @ n, 0, atol=1e-15)
    a = np.zeros(3)
    a[axis] = 1
    assert np.allclose(B[:, 0], np.cross(n, a) / np.linalg.norm(np.cross(n, a)), atol=1e-15)
    assert np.allclose(B[:, 1], np.cross(n, B[:, 0]), atol=1e-15)
    Bm = np.array([[float(x) for x in row] for row in MS.unit3_basis(MS.M.vec(n))])
    assert np.allclose(B, Bm, atol=1e-15)
    if tuple(n) == (0.0, 0.0, 1.0):     # the x axis is chosen: b1 = e_z x e_x = (0, 1, 0), b2 = e_z x b1 = (-1, 0, 0)
        assert np.array_equal(B, [[0, -1], [1, 0], [0, 0]])


# ---- derivatives ----------------------------------------------------------------------------------------------------------
TRUE_H = ("gps", "gps_arm", "gps_calib", "trans2", "trans3", "att_rot3", "att_pose3", "mag_rot3", "mag_pose3", "mag_pose2")


@pytest.mark.parametrize("form", S.FORMS)
def test_restatements_agree_and_the_analytic_H_is_the_true_derivative(form):
    arr, _ = S.random_graph([form], 6, "unit", seed=5 + S.FORMS.index(form))
    for f in range(arr.n_factors):
        e, Hs, _ = S.evaluate(arr, arr.values, f)
        em, Hm, _ = MS.evaluate(arr, arr.values, f)
        scale = max(1.0, float(np.max(np.abs(arr.meas))))
        assert np.allclose(e, em, rtol=0, atol=1e-13 * scale)
        for H, Hq in zip(Hs, Hm):
            assert H.shape == Hq.shape and np.allclose(H, Hq, rtol=0, atol=1e-13 * scale)
        if form in TRUE_H:
            for Hq, Ht in zip(Hm, MS.true_jacobians(arr, arr.values, f)):
                assert np.allclose(Hq, Ht, rtol=0, atol=1e-12 * scale), (form, f)


def test_stated_approximations_are_the_reference_formulas():
    """The rotation priors' H is the identity in the rotation columns (PoseRotationPrior.h:84-87) and Between's second H the
    identity (BetweenFactor.h:118-123 without the Local derivative), not the derivative of Logmap: at a relative rotation
    of a few tenths the true derivative differs."""
    arr, _ = S.random_graph(["rot3", "prior_rot3", "between_rot3"], 3, "unit", seed=2)
    for f in range(arr.n_factors):
        _, Hs, _ = MS.evaluate(arr, arr.values, f)
        Ht = MS.true_jacobians(arr, arr.values, f)
        assert np.array_equal(Hs[-1][:, :3], np.eye(3))
        assert float(np.max(np.abs(Ht[-1][:, :3] - np.eye(3)))) > 1e-3
    arr, _ = S.random_graph(["between_rot3"], 3, "unit", seed=3)
    so = arr.state_offsets()
    for f in range(3):
        R1, R2 = (arr.values[so[v]:so[v + 1]].reshape(3, 3) for v in R.factor_parts(arr, f)[1])
        assert np.allclose(S.evaluate(arr, arr.values, f)[1][0], -R2.T @ R1, atol=1e-15)


def test_rot3_chart_round_trip():
    rng = np.random.default_rng(4)
    for _ in range(5):
        x, d = S.big_rot3(rng).reshape(9), rng.normal(0, 0.5, 3)
        y = S.retract(S.ROT3, x, d)
        assert np.allclose(R.so3_logmap(x.reshape(3, 3).T @ y.reshape(3, 3)), d, atol=1e-14)
        assert np.allclose(y, MS.retract(S.ROT3, x, d), atol=1e-15)
