"""Translation averaging without a device: the restatements of tests/_translation_restatement.py against the reference's
known answers, gsx_translation_recovery_problem against the restated graph, the validation of the new entry points, and the
input conditions of the device tests (tests/test_gpu_translation.py) asserted on the CPU."""
import ctypes as C
import math

import numpy as np
import pytest

from gtsam_petercdev_amd import _abi as A
from gtsam_petercdev_amd import _lib
from gtsam_petercdev_amd import graph as G
from tests import _factor_restatement as R
from tests import _translation_cases as Cs
from tests import _translation_restatement as T

V = A.VAR_VECTOR


def one_factor(ftype, states, z):
    var_list = [(i, V, len(s)) for i, s in enumerate(states)]
    return R.make_arrays(var_list, [(ftype, list(range(len(states))), 3, z, A.NOISE_UNIT, [])], np.concatenate(states))


# ---- the restatements against the reference's known answers -------------------------------------------------------------
def test_factor_known_answers():
    """testTranslationFactor.cpp:42-71, :109-140."""
    s = 1 / math.sqrt(2)
    z = np.array([1.0, 0.0, 0.0])
    for evaluate in (T.evaluate, T.evaluate_50):
        arr = one_factor(A.F_TRANSLATION, [np.array([1.0, 0, 0]), np.array([2.0, 0, 0])], z)
        assert np.max(np.abs(evaluate(arr, arr.values, 0)[0])) <= 1e-9
        arr = one_factor(A.F_TRANSLATION, [np.array([0.0, 1, 1]), np.array([0.0, 2, 2])], z)
        assert np.max(np.abs(evaluate(arr, arr.values, 0)[0] - [-1, s, s])) <= 1e-9
        arr = one_factor(A.F_BILINEAR_TRANSLATION, [np.array([1.0, 0, 0]), np.array([2.0, 0, 0]), np.array([1.0])], z)
        assert np.max(np.abs(evaluate(arr, arr.values, 0)[0])) <= 1e-9
        arr = one_factor(A.F_BILINEAR_TRANSLATION, [np.array([0.0, 1, 1]), np.array([0.0, 2, 2]), np.array([s])], z)
        assert np.max(np.abs(evaluate(arr, arr.values, 0)[0] - [-1, s, s])) <= 1e-9


@pytest.mark.parametrize("family", ["translation", "bata"])
def test_jacobians_against_central_differences(family):
    for mode in Cs.SCALE_MODES[:2] if family == "bata" else ("positive",):
        arr = Cs.factor_graph(family, 5, "unit", seed=3, scale_mode=mode)
        for f in range(arr.n_factors):
            num = T.numerical_jacobians(arr, arr.values, f)
            for evaluate in (T.evaluate, T.evaluate_50):
                for H, Hn in zip(evaluate(arr, arr.values, f)[1], num):
                    assert np.max(np.abs(H - Hn)) <= 1e-9
    if family == "bata":        # s == 0 takes the >= branch: H3 = Tb - Ta
        arr = one_factor(A.F_BILINEAR_TRANSLATION, [np.zeros(3), np.array([1.0, 2, 3]), np.array([0.0])], np.zeros(3))
        for evaluate in (T.evaluate, T.evaluate_50):
            assert np.array_equal(evaluate(arr, arr.values, 0)[1][2].ravel(), [1.0, 2, 3])
            assert np.array_equal(evaluate(arr, arr.values, 0)[1][1], np.zeros((3, 3)))


def test_mfas_known_answers():
    """testMFAS.cpp:25-97."""
    w2, w1 = dict(zip(Cs.MFAS_EDGES, Cs.MFAS_WEIGHTS2)), dict(zip(Cs.MFAS_EDGES, Cs.MFAS_WEIGHTS1))
    assert T.mfas_ordering(w2)[0] == [0, 1, 3, 2] and T.mfas_ordering(w1)[0] == [3, 0, 1, 2]
    for e, w in T.mfas_outlier_weights(w2).items():
        assert abs(w - (0.5 if e == (3, 0) else 0.0)) <= 1e-6
    assert all(abs(w) <= 1e-6 for w in T.mfas_outlier_weights(w1).values())


def test_the_draws_are_those_of_mt19937_and_uniform_real():
    assert T.mt19937_uniform_draws(42, 3) == [0.59308596857569196, -0.63313042421326304, 0.5593819952253225]


# ---- gsx_translation_recovery_problem against the restated graph ---------------------------------------------------------
def assert_same_problem(arr, want):
    for n in ("var_keys", "var_types", "var_dims", "f_type", "f_rows", "f_key_ptr", "f_vars", "f_meas_ptr", "f_noise_kind",
              "f_noise_ptr", "values"):
        assert np.array_equal(getattr(arr, n), getattr(want, n)), n
    nm, nn = int(want.f_meas_ptr[-1]), int(want.f_noise_ptr[-1])
    assert np.array_equal(arr.meas[:nm], want.meas[:nm]) and np.array_equal(arr.noise[:nn], want.noise[:nn])


@pytest.mark.parametrize("bilinear", [False, True])
@pytest.mark.parametrize("name", list(Cs.RECOVERY_CASES))
def test_recovery_problem_matches_the_restated_graph(name, bilinear):
    unit, scale, between, _, _ = Cs.recovery_inputs(name)
    p = _lib.translation_params_default()
    assert (p.seed, p.prior_sigma, p.use_bilinear, p.lm.max_iterations, p.lm.lambda_initial) == (42, 0.01, 0, 100, 1e-5)
    p.use_bilinear = int(bilinear)
    arr, merged = _lib.translation_recovery_problem(unit, scale, between, None, p)
    g = T.translation_graph(unit, scale, between, None, bilinear)
    assert_same_problem(arr, T.graph_arrays(g))
    assert merged == g["merged"]
    if name == "all_zero":
        assert arr.n_factors == 0 and arr.n_vars == 1 and np.array_equal(arr.values, np.zeros(3)) and len(merged) == 2
    if name == "three_with_zero_edge":
        assert merged == {2: 1} and arr.n_factors == 3


def test_recovery_problem_given_values_seed_and_mirror():
    unit, scale, between, _, _ = Cs.recovery_inputs("between_only_node")
    given = {3: np.array([0.5, 0.25, -1.0])}
    p = _lib.translation_params_default()
    p.seed = 7
    arr, _ = _lib.translation_recovery_problem(unit, scale, between, given, p)
    assert_same_problem(arr, T.graph_arrays(T.translation_graph(unit, scale, between, given, False, seed=7)))
    assert np.array_equal(arr.values[6:9], given[3])
    # the Python mirror builds the same graph from the reference's building blocks
    pos = Cs.RECOVERY_CASES["between_only_node"][0]
    ms = [G.BinaryMeasurementUnit3(a, b, G.Unit3(np.array(pos[b], float) - np.array(pos[a], float)),
                                   G.noiseModel.Isotropic.Sigma(3, 0.01)) for a, b, _, _, _ in unit]
    unit = G.TranslationRecovery._edges(ms)
    bs = [G.BinaryMeasurementPoint3(0, 1, [2.0, 0, 0], G.noiseModel.Constrained.All(3, 1e2)),
          G.BinaryMeasurementPoint3(0, 4, [1.0, 2, 1])]
    tr = G.TranslationRecovery()
    graph = tr.buildGraph(ms)
    assert graph.size() == 3
    tr.addPrior(ms, scale, bs, graph)
    initial = tr.initializeRandomly(ms, bs)
    arr0, _ = _lib.translation_recovery_problem(unit, scale, between)
    assert_same_problem(graph.to_arrays(initial), arr0)


def test_unit3_mirror():
    u = G.Unit3(np.array([3.0, 0.0, 4.0]))
    assert np.allclose(u.point3(), [0.6, 0, 0.8], atol=1e-15) and abs(u.dot(G.Unit3(1, 0, 0)) - 0.6) <= 1e-15
    assert np.array_equal(G.Unit3(0.0, 0.0, 0.0).point3(), np.zeros(3)) and G.Unit3(0, 0, 0).equals(G.Unit3())  is False
    assert not u.equals(G.Unit3(1, 0, 0))
    f = G.TranslationFactor(1, 2, [0.0, 0.0, 2.0], G.noiseModel.Isotropic.Sigma(3, 0.1))
    assert f.ftype == A.F_TRANSLATION and np.array_equal(f.meas, [0, 0, 1.0]) and f.rows == 3
    b = G.BilinearAngleTranslationFactor(1, 2, G.symbol("S", 0), G.Unit3(0, 2, 0))
    assert b.ftype == A.F_BILINEAR_TRANSLATION and b.keys() == [1, 2, (ord("S") << 56)]


# ---- validation -------------------------------------------------------------------------------------------------------------
def _create_status(arr):
    lib = _lib.load()
    lib.gsx_create.restype = C.c_int32
    h, desc = C.c_void_p(), arr.desc()
    st = lib.gsx_create(C.byref(desc), C.c_int32(0), C.byref(h))
    if st == A.GSX_OK:
        lib.gsx_destroy(h)
    return st


def test_bad_shapes_are_invalid():
    z, v3 = np.array([1.0, 0, 0]), np.zeros(3)
    bad = [
        R.make_arrays([(0, V, 3), (1, V, 2)], [(A.F_TRANSLATION, [0, 1], 3, z, A.NOISE_UNIT, [])], np.zeros(5)),
        R.make_arrays([(0, V, 3), (1, V, 3)], [(A.F_TRANSLATION, [0, 1], 3, [1.0, 0], A.NOISE_UNIT, [])], np.zeros(6)),
        R.make_arrays([(0, V, 3), (1, V, 3)], [(A.F_TRANSLATION, [0, 1], 2, z, A.NOISE_UNIT, [])], np.zeros(6)),
        R.make_arrays([(0, V, 3), (1, A.VAR_POSE2, 3)], [(A.F_TRANSLATION, [0, 1], 3, z, A.NOISE_UNIT, [])], np.zeros(6)),
        R.make_arrays([(0, V, 3), (1, V, 3), (2, V, 1)], [(A.F_TRANSLATION, [0, 1, 2], 3, z, A.NOISE_UNIT, [])], np.zeros(7)),
        R.make_arrays([(0, V, 3), (1, V, 3)], [(A.F_BILINEAR_TRANSLATION, [0, 1], 3, z, A.NOISE_UNIT, [])], np.zeros(6)),
        R.make_arrays([(0, V, 3), (1, V, 3), (2, V, 2)], [(A.F_BILINEAR_TRANSLATION, [0, 1, 2], 3, z, A.NOISE_UNIT, [])], np.zeros(8)),
        R.make_arrays([(0, V, 3), (1, V, 3), (2, V, 1)], [(A.F_BILINEAR_TRANSLATION, [0, 1, 2], 3, [1.0, 0, 0, 0], A.NOISE_UNIT, [])], np.zeros(7)),
        R.make_arrays([(0, V, 3), (1, V, 3), (2, V, 1)], [(A.F_BILINEAR_TRANSLATION, [0, 1, 2], 3, z, A.NOISE_ISOTROPIC, [])], np.zeros(7)),
    ]
    for i, arr in enumerate(bad):
        assert _create_status(arr) == A.GSX_E_INVALID, i
    del v3


def _mfas_status(key1, key2, weights):
    with pytest.raises(A.GsxError) as e:
        _lib.mfas_outlier_weights(key1, key2, weights=weights)
    return e.value.status


def test_mfas_validation_comes_before_the_device():
    assert _mfas_status([1, 2, 2], [2, 3, 1], np.ones((1, 3))) == A.GSX_E_INVALID           # a pair in both orders
    assert _mfas_status([1, 2], [2, 2], np.ones((1, 2))) == A.GSX_E_INVALID                 # a self edge
    n = A.MFAS_MAX_NODES + 1
    assert _mfas_status(np.arange(n - 1), np.arange(1, n), np.ones((1, n - 1))) == A.GSX_E_INVALID   # too many nodes
    hdr = open(__file__.replace("tests/test_host_translation.py", "include/gsx.h")).read()
    assert f"#define GSX_MFAS_MAX_NODES {A.MFAS_MAX_NODES}" in hdr and A.MFAS_MAX_NODES >= 4096
    # a repeated ordered pair is taken (the last entry counts: tests/test_gpu_translation.py); without a device the call
    # gets as far as the device check
    if _lib.device_count() == 0:
        assert _mfas_status([1, 1], [2, 2], np.ones((1, 2))) == A.GSX_E_NO_DEVICE
    w = T.mfas_edge_weights([1, 1], [2, 2], [[1.0, 0, 0], [-1.0, 0, 0]], [1.0, 0, 0])
    assert w == {(1, 2): -1.0}


# ---- the input conditions of the device tests ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", Cs.MFAS_SHAPES)
def test_mfas_cases_keep_their_margins(shape):
    case = Cs.mfas_case(*shape)
    print(shape, "seed", case["seed"], case["margins"])
    assert case["margins"]["heuristic"] >= Cs.HEURISTIC_MARGIN and case["margins"]["root"] >= Cs.ROOT_MARGIN
    n_nodes = np.unique(np.concatenate([case["key1"], case["key2"]])).size
    assert n_nodes == shape[0] and len(case["weights"]) == shape[1]
    if shape[0] > 5:
        assert 5.0 <= 2.0 * case["key1"].size / n_nodes <= 7.0      # average degree about 6


def _separation_ok(arr):
    so = arr.state_offsets()
    for f in range(arr.n_factors):
        if int(arr.f_type[f]) not in (A.F_TRANSLATION, A.F_BILINEAR_TRANSLATION):
            continue
        _, vs, _ = R.factor_parts(arr, f)
        ta, tb = arr.values[so[vs[0]]:so[vs[0] + 1]], arr.values[so[vs[1]]:so[vs[1] + 1]]
        if np.linalg.norm(tb - ta) < Cs.MIN_SEPARATION * max(np.linalg.norm(ta), np.linalg.norm(tb)):
            return False
    return True


def test_factor_cases_keep_their_separation():
    """Every seeded factor case of tests/test_gpu_translation.py: the shared list, the mixed graph and the 12-node graph."""
    for case in Cs.FACTOR_CASES:
        assert _separation_ok(Cs.factor_case(case)), case
    assert len(Cs.FACTOR_CASES) == 40
    assert _separation_ok(Cs.mixed_graph()) and _separation_ok(Cs.noisy_graph())


def test_noisy_pipeline_case_keeps_its_margins():
    """The 30-node pipeline of the device test: both MFAS margins on every sampled direction, no restated mean on the
    threshold 0.1, and the restated filter fed with the bits Unit3 makes of the measured directions."""
    case = Cs.noisy_pipeline_case()
    print(case["margins"], case["threshold_gap"])
    assert case["margins"]["heuristic"] >= Cs.HEURISTIC_MARGIN and case["margins"]["root"] >= Cs.ROOT_MARGIN
    assert case["threshold_gap"] > 1e-9 and len(case["proj"]) == 40 and len(case["meas"]) == 120
    assert 0 < int(np.sum(case["want_mean"] >= 0.1)) < len(case["meas"])
    assert all(np.array_equal(G.Unit3(z).point3(), d) for (_, _, z, _, _), d in zip(case["meas"], case["dirs"]))
