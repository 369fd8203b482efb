"""body_P_sensor on GSX_F_PROJECTION / _STEREO / _RANGE and GeneralSFMFactor2 (GSX_F_SFM2) without a device: the numpy
restatement the device tests compare against (tests/_sensor_restatement.py) pinned by the reference's own known answers,
by its plain forms at an identity sensor and by true derivatives of the 50-digit error; what gsx_create accepts and
refuses; the Python mirror's lowering."""
import math

import numpy as np
import pytest

from gtsam_petercdev_amd import _abi as A, _lib
from gtsam_petercdev_amd import graph as G
from tests import _factor_restatement as R
from tests import _mp_sensor_restatement as MS
from tests import _sensor_restatement as S
from tests.test_host_factor_types import K9, POSE2, POSE3, two_var_graph

P2, P3, V = A.VAR_POSE2, A.VAR_POSE3, A.VAR_VECTOR
# the sensor pose of the reference's ...WithTransform tests
SENSOR3 = list(R.pose3_state(G.Rot3.RzRyRx(-math.pi / 2, 0.0, -math.pi / 2).matrix(), np.array([0.25, -0.10, 1.0])))
SENSOR2 = [0.25, -0.10, -math.pi / 2]
ID3 = list(R.pose3_state(np.eye(3), np.zeros(3)))
K_TEST = list(G.Cal3_S2(60, 640, 480).vector())       # testProjectionFactor.cpp:33-35


def pose_at(t):
    return list(R.pose3_state(np.eye(3), np.array(t, float)))


# ---- known answers of the reference ------------------------------------------------------------------------------------
def test_restated_projection_with_transform_known_answers():
    """gtsam/slam/tests/testProjectionFactor.cpp:118-138: error (-3, 0) at 1e-9; :166-189: the two Jacobians at 1e-3."""
    arr = two_var_graph(P3, 6, pose_at([-6.25, 0.10, -1.0]), V, 3, [0.0, 0.0, 0.0], A.F_PROJECTION, 2,
                        [323.0, 240.0] + K_TEST + SENSOR3)
    e, H, cheir = S.evaluate(arr, arr.values, 0)
    assert not cheir and np.allclose(e, [-3.0, 0.0], atol=1e-9)
    H1 = [[-92.376, 0.0, 577.350, 0.0, 92.376, 0.0], [-9.2376, -577.350, 0.0, 0.0, 0.0, 92.376]]
    H2 = [[0.0, -92.376, 0.0], [0.0, 0.0, -92.376]]
    assert np.allclose(H[0], H1, atol=1e-3) and np.allclose(H[1], H2, atol=1e-3)
    # the plain factor of the same file (:96-115, :141-163)
    arr = two_var_graph(P3, 6, pose_at([0.0, 0.0, -6.0]), V, 3, [0.0, 0.0, 0.0], A.F_PROJECTION, 2, [323.0, 240.0] + K_TEST)
    e, H, _ = S.evaluate(arr, arr.values, 0)
    assert np.allclose(e, [-3.0, 0.0], atol=1e-9)
    assert np.allclose(H[0], [[0.0, -554.256, 0.0, -92.376, 0.0, 0.0], [554.256, 0.0, 0.0, 0.0, -92.376, 0.0]], atol=1e-3)


def test_restated_stereo_with_transform_known_answers():
    """gtsam/slam/tests/testStereoFactor.cpp, ErrorWithTransform (:108-126): (-3, 2, -1) at 1e-9; JacobianWithTransform
    (:156-181) at 1e-3."""
    arr = two_var_graph(P3, 6, pose_at([-6.50, 0.10, -1.0]), V, 3, [0.0, 0.0, 0.0], A.F_STEREO, 3, K9 + SENSOR3)
    e, H, cheir = S.evaluate(arr, arr.values, 0)
    assert not cheir and np.allclose(e, [-3.0, 2.0, -1.0], atol=1e-9)
    H1 = [[-100.0, 0.0, 650.0, 0.0, 100.0, 0.0], [-100.0, -8.0, 649.2, -8.0, 100.0, 0.0], [-10.0, -650.0, 0.0, 0.0, 0.0, 100.0]]
    H2 = [[0.0, -100.0, 0.0], [8.0, -100.0, 0.0], [0.0, 0.0, -100.0]]
    assert np.allclose(H[0], H1, atol=1e-3) and np.allclose(H[1], H2, atol=1e-3)


def range_with_transform_graphs():
    """testRangeFactor.cpp:140-160 (2-D) and Error3DWithTransform (:182-203): the body pose that puts the sensor where the
    plain tests have the pose; and the pose-to-pose variants to the same place."""
    t2 = np.array([1.0, 2.0]) - R.rot2(0.57) @ np.array(SENSOR2[:2])
    pose2 = [t2[0], t2[1], 0.57]
    Rm = G.Rot3.RzRyRx(0.2, -0.3, 1.75).matrix()
    pose3 = list(R.pose3_state(Rm, np.array([1.0, 2.0, -3.0]) - Rm @ np.array(SENSOR3[9:])))
    return {
        "range_pose2_point2": two_var_graph(P2, 3, pose2, V, 2, [-4.0, 11.0], A.F_RANGE, 1, [10.0] + SENSOR2),
        "range_pose2_pose2": two_var_graph(P2, 3, pose2, P2, 3, [-4.0, 11.0, 0.3], A.F_RANGE, 1, [10.0] + SENSOR2),
        "range_pose3_point3": two_var_graph(P3, 6, pose3, V, 3, [-2.0, 11.0, 1.0], A.F_RANGE, 1, [10.0] + SENSOR3),
        "range_pose3_pose3": two_var_graph(P3, 6, pose3, P3, 6, POSE3[:9] + [-2.0, 11.0, 1.0], A.F_RANGE, 1, [10.0] + SENSOR3),
    }


def test_restated_range_with_transform_known_answers():
    for variant, arr in range_with_transform_graphs().items():
        e, _, cheir = S.evaluate(arr, arr.values, 0)
        assert e.shape == (1,) and abs(e[0] - 0.295630141) < 1e-9 and not cheir, (variant, e)


# ---- identity sensor ---------------------------------------------------------------------------------------------------
def identity_pairs():
    rng = np.random.default_rng(2)
    pose3 = list(R.pose3_state(R.random_rot3(rng, 1.2), rng.uniform(-2, 2, 3)))
    Rm, t = R.pose3_of(pose3)
    front = list(t + Rm @ np.array([0.4, -0.3, 5.0]))
    behind = list(t + Rm @ np.array([0.4, -0.3, -5.0]))
    z2, z3 = [300.0, 200.0] + list(S.K_S2), [300.0, 280.0, 200.0] + list(R.STEREO_K)
    id2 = [0.0, 0.0, 0.0]
    for pt in (front, behind):
        yield (P3, 6, pose3, V, 3, pt, A.F_PROJECTION, 2), z2, ID3
        yield (P3, 6, pose3, V, 3, pt, A.F_STEREO, 3), z3, ID3
    yield (P3, 6, pose3, V, 3, front, A.F_RANGE, 1), [4.0], ID3
    yield (P3, 6, pose3, V, 3, pose3[9:], A.F_RANGE, 1), [4.0], ID3          # zero distance
    yield (P3, 6, pose3, P3, 6, POSE3, A.F_RANGE, 1), [4.0], ID3
    yield (P2, 3, POSE2, V, 2, [-4.0, 11.0], A.F_RANGE, 1), [4.0], id2
    yield (P2, 3, POSE2, V, 2, POSE2[:2], A.F_RANGE, 1), [4.0], id2          # zero distance
    yield (P2, 3, POSE2, P2, 3, [-4.0, 11.0, 0.3], A.F_RANGE, 1), [4.0], id2


def test_identity_sensor_equals_the_plain_form_exactly():
    n = 0
    for spec, z, ident in identity_pairs():
        plain, sens = two_var_graph(*spec, z), two_var_graph(*spec, z + ident)
        ep, Hp, cp = S.evaluate(plain, plain.values, 0)
        es, Hs, cs = S.evaluate(sens, sens.values, 0)
        assert cp == cs and np.array_equal(ep, es) and all(np.array_equal(a, b) for a, b in zip(Hp, Hs)), spec
        n += 1
    assert n == 10


# ---- derivative check --------------------------------------------------------------------------------------------------
def derivative_cases():
    """(arr, factor) of every restated form at random values, the zero-distance branch of the range variants and the
    cheirality branch of the camera ones included."""
    cases = []
    for k, variant in enumerate(S.VARIANTS):
        arr = S.random_graph(variant, 8, "unit", seed=40 + k)
        cases += [(arr, f) for f in range(arr.n_factors)]
    rng = np.random.default_rng(9)
    s3, s2 = S.random_sensor3(rng), S.random_sensor2(rng)
    body3 = S.body_of(R.pose3_state(R.random_rot3(rng, 1.2), rng.uniform(-2, 2, 3)), s3)
    cam, _ = S.pose3_compose(body3, s3)
    Rc, tc = R.pose3_of(cam)
    # the sensor origin on the landmark (norm3 / norm2's row of ones times the adjoint) ...
    cases.append((two_var_graph(P3, 6, body3, V, 3, tc, A.F_RANGE, 1, [0.5] + list(s3)), 0))
    b2 = np.array([0.7, -1.1, 0.4])
    cases.append((two_var_graph(P2, 3, b2, V, 2, S.pose2_compose(b2, s2)[0][:2], A.F_RANGE, 1, [0.5] + list(s2)), 0))
    # ... and a point behind the SENSOR: constant error, zero Jacobians, for the three camera factors
    behind = tc + Rc @ np.array([0.2, 0.1, -3.0])
    cases.append((two_var_graph(P3, 6, body3, V, 3, behind, A.F_PROJECTION, 2, [300.0, 200.0] + list(S.K_S2) + list(s3)), 0))
    cases.append((two_var_graph(P3, 6, body3, V, 3, behind, A.F_STEREO, 3, [300.0, 280.0, 200.0] + list(R.STEREO_K) + list(s3)), 0))
    cases.append((R.make_arrays([(1, P3, 6), (2, V, 3), (3, V, 5)], [(A.F_SFM2, [0, 1, 2], 2, [300.0, 200.0], A.NOISE_UNIT, ())],
                                np.concatenate([cam, behind, S.K_S2])), 0))
    return cases


def ones_row_truth(arr, f):
    """The zero-distance branch has no derivative to compare with: |d| is not differentiable at d = 0, and what the
    reference hands out there is norm2 / norm3's row of ones in place of d / |d| (Point2.cpp:27-36, Point3.cpp:41-50),
    followed by the chain rule.  The true derivative that row stands on is that of ones . d(x), d the vector whose norm is
    taken — the landmark in the composed sensor frame (Pose3::range, Pose3.cpp:408-431) or the world-frame difference to
    the composed sensor origin (Pose2::range, Pose2.cpp:271-310): central differences of that, in 50 digits."""
    import mpmath as mp
    from tests import _mp_restatement as M
    ftype, vt, st, z = M.factor_inputs(arr, arr.values, f)
    st, z = [M.vec(x) for x in st], M.vec(z)

    def ones_dot_d(states):
        if vt[0] == P2:
            pose, _ = MS.pose2_compose_sensor(states[0], z[1:4])
            return (states[1][0] - pose[0]) + (states[1][1] - pose[1])
        pose, _ = MS.pose3_compose_sensor(states[0], z[1:13])
        Rm, t = M.pose3_of(pose)
        return mp.fsum(M.mv(M.tr3(Rm), M.sub(states[1][:3], t)))
    h, out = mp.mpf("1e-20"), []
    for k, v in enumerate(R.factor_parts(arr, f)[1]):
        d = int(arr.var_dims[v])
        row = []
        for j in range(d):
            vals = []
            for sgn in (1, -1):
                dx = [mp.mpf(0)] * d
                dx[j] = sgn * h
                moved = list(st)
                moved[k] = M.retract_mp(vt[k], st[k], dx)
                vals.append(ones_dot_d(moved))
            row.append(float((vals[0] - vals[1]) / (2 * h)))
        out.append(np.array([row]))
    return out


ZERO_DISTANCE = (-5, -4)     # positions of the two zero-distance cases in derivative_cases()


def true_derivatives(cases):
    n = len(cases)
    return [ones_row_truth(arr, f) if i - n in ZERO_DISTANCE else MS.true_jacobians(arr, arr.values, f)
            for i, (arr, f) in enumerate(cases)]


def worst_derivative_difference(cases, truth):
    """max over cases and keys of |H restated - H true| / max(1, |H true|)."""
    worst = 0.0
    for (arr, f), Ht in zip(cases, truth):
        _, H, _ = S.evaluate(arr, arr.values, f)
        for Ha, Hn in zip(H, Ht):
            worst = max(worst, float(np.max(np.abs(Ha - Hn)) / max(1.0, np.max(np.abs(Hn)))))
    return worst


def test_restated_jacobians_are_the_derivatives_of_the_50_digit_error():
    """Every Jacobian of the restatement — the four sensor forms, all three of SFM2, the zero-distance and the cheirality
    branches — against a central difference of the 50-digit error (step 1e-20: the difference quotient is exact to 1e-30).
    At zero distance the error |d| has no derivative; there the comparison is with the derivative of ones . d, the
    function whose gradient the reference's row of ones is (ones_row_truth).

    The bound is not taken from the restatement's own result: it is a tenth of the largest difference a deliberately wrong
    term causes on the same cases — the adjoint without its translation block [t]x R, and Dcal without its skew column —
    the smaller of the two.  Measured on these 61 cases, each difference relative to max(1, largest entry of the true
    Jacobian) of its block: the restatement 2.6e-15; without the adjoint's translation block 0.64; without the skew column
    of Dcal 0.30; the bound is therefore 3.0e-2."""
    cases = derivative_cases()
    truth = true_derivatives(cases)
    for i in ZERO_DISTANCE:                                # the zero-distance cases are at zero distance
        assert abs(S.evaluate(cases[i][0], cases[i][0].values, cases[i][1])[0][0] + 0.5) < 1e-12
    flagged = sum(bool(S.evaluate(arr, arr.values, f)[2]) for arr, f in cases)
    assert flagged == 3                                    # the three cheirality cases, and no other
    for (arr, f), Ht in zip(cases[-3:], truth[-3:]):
        assert not any(np.any(H) for H in Ht)              # a constant error: the true derivative vanishes
    wrong = {}
    for term in ("adjoint_translation", "dcal_skew"):
        S.WRONG.add(term)
        try:
            wrong[term] = worst_derivative_difference(cases, truth)
        finally:
            S.WRONG.discard(term)
    worst = worst_derivative_difference(cases, truth)
    bound = min(wrong.values()) / 10.0
    print(f"restated Jacobians vs the true derivative over {len(cases)} cases: worst {worst:.3e}; with a wrong term "
          f"{ {k: float(f'{v:.3e}') for k, v in wrong.items()} }; bound {bound:.3e}")
    assert min(wrong.values()) > 1e-3                      # the wrong terms show on these cases
    assert worst <= bound


def test_float64_restatement_against_the_50_digit_one():
    """The numpy restatement's e and H against the 50-digit ones on the derivative cases: 1e-12 relative to the factor's
    largest entry (both evaluate the same formulas; this catches a formula that differs between the two files)."""
    for arr, f in derivative_cases():
        e, H, c = S.evaluate(arr, arr.values, f)
        em, Hm, cm = MS.evaluate(arr, arr.values, f)
        assert c == cm
        scale = max(1.0, float(np.max(np.abs(em))), max(float(np.max(np.abs(h))) for h in Hm))
        assert np.max(np.abs(e - em)) <= 1e-12 * scale
        assert all(np.max(np.abs(a - b)) <= 1e-12 * scale for a, b in zip(H, Hm))


# ---- gsx_create --------------------------------------------------------------------------------------------------------
def sfm2_graph(types=((P3, 6), (V, 3), (V, 5)), rows=2, meas=(300.0, 200.0), kind=A.NOISE_UNIT, noise=()):
    st = {P3: POSE3, P2: POSE2}
    vals = [st[t] if t != V else [1.0 + i for i in range(d)] for t, d in types]
    return R.make_arrays([(k + 1, t, d) for k, (t, d) in enumerate(types)],
                         [(A.F_SFM2, list(range(len(types))), rows, list(meas), kind, noise)], np.concatenate(vals))


ACCEPTED = {
    "projection + sensor (19)": lambda **kw: two_var_graph(P3, 6, POSE3, V, 3, [0.0, 0.0, 0.0], A.F_PROJECTION, 2,
                                                         [323.0, 240.0] + K_TEST + SENSOR3, **kw),
    "stereo + sensor (21)": lambda **kw: two_var_graph(P3, 6, POSE3, V, 3, [0.0, 0.0, 0.0], A.F_STEREO, 3, K9 + SENSOR3, **kw),
    "range pose3-point + sensor (13)": lambda **kw: two_var_graph(P3, 6, POSE3, V, 3, [-2.0, 11.0, 1.0], A.F_RANGE, 1,
                                                                [10.0] + SENSOR3, **kw),
    "range pose3-pose3 + sensor (13)": lambda **kw: two_var_graph(P3, 6, POSE3, P3, 6, POSE3, A.F_RANGE, 1, [10.0] + SENSOR3, **kw),
    "range pose2-point + sensor (4)": lambda **kw: two_var_graph(P2, 3, POSE2, V, 2, [-4.0, 11.0], A.F_RANGE, 1, [10.0] + SENSOR2, **kw),
    "range pose2-pose2 + sensor (4)": lambda **kw: two_var_graph(P2, 3, POSE2, P2, 3, [-4.0, 11.0, 0.3], A.F_RANGE, 1,
                                                               [10.0] + SENSOR2, **kw),
    "sfm2": lambda **kw: sfm2_graph(**kw),
}


@pytest.mark.parametrize("what", sorted(ACCEPTED))
def test_create_accepts_the_sensor_forms_and_sfm2(what):
    """GSX_E_INVALID before these forms existed.  Every noise kind; the symbolic analysis runs; [A b] has the plain
    form's size (the sensor pose adds no column)."""
    rng = np.random.default_rng(1)
    plain = ACCEPTED[what]()
    m = int(plain.f_rows[0])
    for noise in ("unit", "isotropic", "diagonal", "gaussian", "huber"):
        kind, params = R.noise_of(rng, noise, m)
        be = _lib.ProductBackend(ACCEPTED[what](kind=kind, noise=params), host_only=True)
        be.set_ordering(be.compute_ordering(A.ORDER_MINDEGREE))
        assert be.jacobian_size == m * (int(plain.var_dims.sum()) + 1)
        be.close()


REJECTED = {
    "projection with 8": two_var_graph(P3, 6, POSE3, V, 3, [0.0, 0.0, 0.0], A.F_PROJECTION, 2, [323.0, 240.0] + K_TEST + [1.0]),
    "projection with 18": two_var_graph(P3, 6, POSE3, V, 3, [0.0, 0.0, 0.0], A.F_PROJECTION, 2, [323.0, 240.0] + K_TEST + SENSOR3[:11]),
    "projection with 20": two_var_graph(P3, 6, POSE3, V, 3, [0.0, 0.0, 0.0], A.F_PROJECTION, 2, [323.0, 240.0] + K_TEST + SENSOR3 + [0.0]),
    "stereo with 18": two_var_graph(P3, 6, POSE3, V, 3, [0.0, 0.0, 0.0], A.F_STEREO, 3, K9 + SENSOR3[:9]),
    "stereo with 20": two_var_graph(P3, 6, POSE3, V, 3, [0.0, 0.0, 0.0], A.F_STEREO, 3, K9 + SENSOR3[:11]),
    "range with 8": two_var_graph(P3, 6, POSE3, V, 3, [-2.0, 11.0, 1.0], A.F_RANGE, 1, [10.0] + SENSOR3[:7]),
    "a POSE2 range with 13": two_var_graph(P2, 3, POSE2, V, 2, [-4.0, 11.0], A.F_RANGE, 1, [10.0] + SENSOR3),
    "a POSE3 range with 4": two_var_graph(P3, 6, POSE3, V, 3, [-2.0, 11.0, 1.0], A.F_RANGE, 1, [10.0] + SENSOR2),
    "sfm2 on a POSE2": sfm2_graph(types=((P2, 3), (V, 3), (V, 5))),
    "sfm2 to a VECTOR(2)": sfm2_graph(types=((P3, 6), (V, 2), (V, 5))),
    "sfm2 with a pose for a calibration": sfm2_graph(types=((P3, 6), (V, 3), (P3, 6))),
    "sfm2 with a VECTOR(4) calibration": sfm2_graph(types=((P3, 6), (V, 3), (V, 4))),
    "sfm2 with two keys": sfm2_graph(types=((P3, 6), (V, 3))),
    "sfm2 with three rows": sfm2_graph(rows=3),
    "sfm2 with three measurement doubles": sfm2_graph(meas=(1.0, 2.0, 3.0)),
}


@pytest.mark.parametrize("what", sorted(REJECTED))
def test_create_rejects_other_lengths_and_malformed_sfm2(what):
    with pytest.raises(A.GsxError) as ei:
        _lib.ProductBackend(REJECTED[what], host_only=True)
    assert ei.value.status == A.GSX_E_INVALID


# ---- the Python mirror -------------------------------------------------------------------------------------------------
def test_mirror_builds_exactly_these_arrays():
    body_P_sensor = G.Pose3(G.Rot3.RzRyRx(-math.pi / 2, 0.0, -math.pi / 2), [0.25, -0.10, 1.0])
    K = G.Cal3_S2(60, 640, 480)
    unit1, unit2, unit3 = (G.noiseModel.Unit.Create(m) for m in (1, 2, 3))
    g = G.NonlinearFactorGraph()
    g.add(G.GenericProjectionFactor([323.0, 240.0], unit2, G.X(1), G.L(1), K, body_P_sensor))
    g.add(G.GenericProjectionFactor([323.0, 240.0], unit2, G.X(1), G.L(1), K))
    g.add(G.GenericStereoFactor(G.StereoPoint2(323, 268, 241), unit3, G.X(1), G.L(1),
                                G.Cal3_S2Stereo(625, 625, 0, 320, 240, 0.5), body_P_sensor))
    g.add(G.RangeFactorWithTransform(G.X(1), G.L(1), 10.0, unit1, body_P_sensor))
    g.add(G.RangeFactorWithTransform(G.X(1), G.X(2), 10.0, unit1, body_P_sensor))
    g.add(G.GeneralSFMFactor2([300.0, 200.0], unit2, G.X(1), G.L(1), G.symbol("K", 0)))
    g.add(G.PriorFactor(G.symbol("K", 0), G.Cal3_S2(50, 50, 0, 50, 50), G.noiseModel.Diagonal.Sigmas([500, 500, 0.1, 100, 100])))
    v = G.Values()
    v.insert(G.X(1), G.Pose3.from_state(POSE3))
    v.insert(G.X(2), G.Pose3.from_state(POSE3))
    v.insert(G.L(1), G.Point3(-2.0, 11.0, 1.0))
    v.insert(G.symbol("K", 0), G.Cal3_S2(60, 60, 0, 45, 45))
    arr = g.to_arrays(v)
    assert arr.f_type.tolist() == [A.F_PROJECTION, A.F_PROJECTION, A.F_STEREO, A.F_RANGE, A.F_RANGE, A.F_SFM2, A.F_PRIOR]
    assert np.diff(arr.f_meas_ptr).tolist() == [19, 7, 21, 13, 13, 2, 5] and arr.f_rows.tolist() == [2, 2, 3, 1, 1, 2, 5]
    mp_ = arr.f_meas_ptr
    assert arr.meas[mp_[0]:mp_[1]].tolist() == [323.0, 240.0] + K_TEST + SENSOR3
    assert arr.meas[mp_[2]:mp_[3]].tolist() == K9 + SENSOR3
    assert arr.meas[mp_[3]:mp_[4]].tolist() == [10.0] + SENSOR3
    assert arr.meas[mp_[5]:mp_[6]].tolist() == [300.0, 200.0] and arr.meas[mp_[6]:mp_[7]].tolist() == [50, 50, 0, 50, 50]
    kk = list(arr.var_keys).index(G.symbol("K", 0))      # 'K' < 'l' < 'x': the calibration comes first in the Values
    assert kk == 0 and arr.var_types[kk] == V and arr.var_dims[kk] == 5
    assert arr.f_vars[arr.f_key_ptr[5]:arr.f_key_ptr[6]].tolist() == [2, 1, 0]          # (pose, landmark, calibration)
    assert arr.values[:5].tolist() == [60, 60, 0, 45, 45]
    _lib.ProductBackend(arr, host_only=True).close()
    # 2-D
    g2 = G.NonlinearFactorGraph()
    g2.add(G.RangeFactorWithTransform(G.X(1), G.L(1), 10.0, unit1, G.Pose2(*SENSOR2)))
    v2 = G.Values()
    v2.insert(G.X(1), G.Pose2(*POSE2))
    v2.insert(G.L(1), G.Point2(-4.0, 11.0))
    arr2 = g2.to_arrays(v2)
    assert arr2.meas.tolist() == [10.0] + SENSOR2
    _lib.ProductBackend(arr2, host_only=True).close()
    bad = G.NonlinearFactorGraph()
    bad.add(G.RangeFactorWithTransform(G.X(1), G.L(1), 10.0, unit1, body_P_sensor))    # a Pose3 sensor on a Pose2
    with pytest.raises(ValueError):
        bad.to_arrays(v2)
    with pytest.raises(ValueError):
        G.GenericProjectionFactor([1.0, 2.0], unit2, G.X(1), G.L(1), K, G.Pose2())
