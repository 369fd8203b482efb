"""Smart projection factors without a GPU: the restatement against the known answers of the reference's
testSmartProjectionPoseFactor.cpp, the per-factor arithmetic of the kernels (csrc/smart_math.h) as a stand-alone host program
under the sanitizers, judged like the device, the refusals of gsx_create, the Python classes and the condition on the seeded
inputs that the GPU tests rely on."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import gtsam_petercdev_amd as gt
from gtsam_petercdev_amd import _abi as A, _lib
from tests import _smart_cases as CS
from tests import _smart_restatement as R
from tests._triangulation_restatement import well_separated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LEVEL = CS.state(CS.rot_ypr(-math.pi / 2, 0.0, -math.pi / 2), [0, 0, 1])
RIGHT = CS.compose(LEVEL, CS.state(np.eye(3), [1, 0, 0]))
ABOVE = CS.compose(LEVEL, CS.state(np.eye(3), [0, -1, 0]))
LANDMARKS = [np.array([5, 0.5, 1.2]), np.array([5, -0.5, 1.2]), np.array([3, 0, 3.0])]
K_FOV = gt.Cal3_S2(60, 640, 480).vector()   # vanillaPose::sharedK


def exact_spec(poses, landmark, K, **kw):
    px = np.array([CS.project(p, K, landmark) for p in poses])
    return R.Spec(K=np.asarray(K, float), pixels=px, views=list(range(len(poses))), **kw)


@pytest.fixture(scope="module")
def lib():
    from gtsam_petercdev_amd import build
    build.build_lib()
    return _lib.load()


@pytest.mark.parametrize("X", [R.FLOAT, R.MP], ids=["float64", "mp50"])
def test_restatement_noiseless(X):
    """TEST(SmartProjectionPoseFactor, noiseless): error 0 to 1e-7, the point is the landmark"""
    f = R.SmartFactor(exact_spec([LEVEL, RIGHT], LANDMARKS[0], K_FOV, sigma=0.1), X)
    assert abs(float(f.error([LEVEL, RIGHT]))) < 1e-7
    assert f.status == R.VALID and np.allclose(f.point_float(), LANDMARKS[0], atol=1e-7)


@pytest.mark.parametrize("X", [R.FLOAT, R.MP], ids=["float64", "mp50"])
def test_restatement_factors(X):
    """TEST(SmartProjectionPoseFactor, Factors): the Hessian is 0.5 [A1 A2]'[A1 A2] with the A of the test, and the linearized
    error at the all-ones delta is 2500 for the Hessian form and (the same normal equations) the SVD form, to 1e-6"""
    c1, c2 = CS.state(np.eye(3), [0, 0, 0]), CS.state(np.eye(3), [1, 0, 0])
    f = R.SmartFactor(exact_spec([c1, c2], np.array([0, 0, 10.0]), [100, 100, 0, 0, 0], sigma=0.1), X)
    H, _, _ = f.hessian([c1, c2])
    assert f.status == R.VALID and np.allclose(f.point_float(), [0, 0, 10], atol=1e-9)
    A12 = np.array([[-10, 0, 0, 0, 1, 0, 10, 0, 1, 0, -1, 0]], float) * (10.0 / 0.1)
    Hf = np.array(H, dtype=float)
    assert np.allclose(Hf[:12, :12], 0.5 * A12.T @ A12, atol=1e-6)
    assert np.allclose(Hf[12, :], 0, atol=1e-6)
    d = np.ones(12)
    assert abs(0.5 * d @ Hf[:12, :12] @ d - d @ Hf[:12, 12] + 0.5 * Hf[12, 12] - 2500) < 1e-6
    assert abs(0.5 * Hf[12, 12]) < 1e-6   # error at the zero delta


@pytest.mark.parametrize("X", [R.FLOAT, R.MP], ids=["float64", "mp50"])
def test_restatement_landmark_distance_and_outlier(X):
    """landmarkDistance (threshold 2: every factor disabled, FAR_POINT) and dynamicOutlierRejection (the fourth factor, whose
    first pixel is moved by (10, 10), is an OUTLIER under a threshold of 1; the others are VALID with error 0)"""
    poses = [LEVEL, RIGHT, ABOVE]
    for lm in LANDMARKS:
        f = R.SmartFactor(exact_spec(poses, lm, K_FOV, sigma=0.1, landmark_distance_threshold=2.0), X)
        H, _, _ = f.hessian(poses)
        assert f.status == 4 and not np.any(np.array(H, dtype=float)) and float(f.error(poses)) == 0.0
    for i, lm in enumerate(LANDMARKS + [np.array([5, -0.5, 1.0])]):
        s = exact_spec(poses, lm, K_FOV, sigma=0.1, landmark_distance_threshold=1e10, outlier_threshold=1.0)
        if i == 3:
            s.pixels[0] += 10.0
        f = R.SmartFactor(s, X)
        e = float(f.error(poses))
        assert (f.status, e == 0.0 or e < 1e-12) == ((3 if i == 3 else R.VALID), True)


def test_restatement_cache():
    """decideIfTriangulate: a move below the threshold keeps the point, one above re-triangulates; threshold 0 re-triangulates
    whenever a pose differs"""
    _, spec, poses = CS.track_cases()[4]
    own = [poses[v] for v in spec.views]
    f = R.SmartFactor(spec, R.FLOAT)
    small = [CS.expmap_small(p, 0.1 * spec.retriangulation_threshold * np.ones(6)) for p in own]
    big = [CS.expmap_small(p, 10 * spec.retriangulation_threshold * np.ones(6)) for p in own]
    assert [f.triangulate_safe(own), f.triangulate_safe(small), f.triangulate_safe(big), f.triangulate_safe(own)] == \
        [True, False, True, True]


def _create(arr):
    h = C.c_void_p()
    f = _lib.load().gsx_create
    f.restype = C.c_int32
    d = arr.desc()
    st = f(C.byref(d), C.c_int32(0), C.byref(h))
    if h:
        _lib.load().gsx_destroy(h)
    return st


def test_create_refusals(lib):
    """section 1 of the header: every refusal is GSX_E_INVALID from gsx_create, before a device is touched"""
    cams = CS.camera_poses()
    lm = CS.landmarks(1)[0]
    good = CS.make_spec([0, 1, 2], lm, cams)

    def arrays(spec=good, poses=cams, **edit):
        a = CS.graph_arrays([spec], poses)
        for k, v in edit.items():
            getattr(a, k)[...] = v if np.ndim(v) else getattr(a, k) * 0 + v
        return a
    assert _create(arrays()) == A.GSX_OK   # (a handle is made without a device too: only the numeric calls need one)
    # one view / nine views
    one = CS.graph_arrays([CS.make_spec([0, 1], lm, cams)], cams)
    one.f_key_ptr[1:] -= 1
    one.f_vars = np.ascontiguousarray(one.f_vars[1:])
    assert _create(one) == A.GSX_E_INVALID
    nine = CS.camera_poses() + [cams[0]]
    s9 = CS.make_spec(list(range(8)), lm, cams)
    s9.pixels = np.concatenate([s9.pixels, s9.pixels[:1]])
    s9.views = list(range(9))
    assert _create(CS.graph_arrays([s9], nine)) == A.GSX_E_INVALID
    # rows, noise kinds, robust bit, degeneracy modes, a key that is no pose
    a = arrays(); a.f_rows[0] = 4; assert _create(a) == A.GSX_E_INVALID
    for kind, npar in ((A.NOISE_DIAGONAL, 3), (A.NOISE_GAUSSIAN, 9), (A.NOISE_ISOTROPIC | A.NOISE_ROBUST_HUBER, 2)):
        a = CS.graph_arrays([good], cams, prior_on=())
        a.f_noise_kind[0] = kind
        a.noise = np.ones(npar)
        a.f_noise_ptr[1] = npar
        assert _create(a) == A.GSX_E_INVALID
    for mode in (0.0, 2.0):
        a = arrays()
        a.meas[10] = mode
        assert _create(a) == A.GSX_E_INVALID
    a = arrays(); a.var_types[1] = A.VAR_VECTOR; assert _create(a) == A.GSX_E_INVALID
    # a wrong measurement length
    a = arrays(); a.f_meas_ptr[1:] += 1; a.meas = np.concatenate([a.meas, [0.0]]); assert _create(a) == A.GSX_E_INVALID


def test_python_classes_and_lowering():
    p = gt.SmartProjectionParams()
    assert (p.linearizationMode, p.degeneracyMode, p.triangulation.rankTolerance, p.triangulation.enableEPI,
            p.retriangulationThreshold, p.triangulation.landmarkDistanceThreshold,
            p.triangulation.dynamicOutlierRejectionThreshold) == (gt.HESSIAN, gt.IGNORE_DEGENERACY, 1.0, False, 1e-5, -1.0, -1.0)
    p.setRetriangulationThreshold(1e-3)
    assert p.getRetriangulationThreshold() == 1e-3
    K = gt.Cal3_S2(*CS.K_CAL)
    cams = CS.camera_poses()
    f = gt.SmartProjectionPose3Factor(gt.noiseModel.Isotropic.Sigma(2, 0.1), K, None, p)
    v = gt.Values()
    for i in range(3):
        f.add(gt.Point2(100.0 + i, 50.0), gt.X(i))
        v.insert(gt.X(i), gt.Pose3(gt.Rot3(cams[i][:9].reshape(3, 3)), cams[i][9:]))
    g = gt.NonlinearFactorGraph()
    g.add(f)
    with pytest.raises(ValueError, match="ZERO_ON_DEGENERACY"):
        g.to_arrays(v)
    p.setDegeneracyMode(gt.ZERO_ON_DEGENERACY)
    a = g.to_arrays(v)
    assert a.f_type.tolist() == [A.F_SMART_PROJECTION] and a.f_rows.tolist() == [3] and a.meas.size == 11 + 6
    assert a.meas[:11].tolist() == list(CS.K_CAL) + [1.0, 0.0, -1.0, -1.0, 1e-3, 1.0] and a.noise[0] == 0.1
    with pytest.raises(ValueError, match="isotropic"):
        gt.SmartProjectionPose3Factor(gt.noiseModel.Diagonal.Sigmas(np.array([1.0, 2.0])), K)
    with pytest.raises(ValueError, match="duplicate"):
        f.add(gt.Point2(1, 1), gt.X(0))
    assert not f.point().valid()


def test_stats_struct_matches_the_header():
    assert [n for n, _ in A.SmartStats._fields_] == ["n_smart_invalid", "n_smart_retriangulated"]
    assert C.sizeof(A.SmartStats) == C.sizeof(A.Stats) + 16 and A.SmartStats.n_smart_invalid.offset == C.sizeof(A.Stats)
    assert set(A.SmartStats().as_dict()) == {n for n, _ in A.Stats._fields_} | {"n_smart_invalid", "n_smart_retriangulated"}
    text = open(os.path.join(ROOT, "include", "gsx.h")).read()
    body = text[text.index("typedef struct gsx_stats {"):text.index("} gsx_stats;")]
    assert body.index("n_pcg_solves") < body.index("n_smart_invalid") < body.index("n_smart_retriangulated")
    assert "gsx_smart_points" in text and "GSX_F_SMART_PROJECTION = 10" in text


def test_seeded_inputs_keep_clear_of_every_threshold():
    """no decision of the 50-digit restatement within a relative 1e-6 of its threshold, on every seeded case"""
    for name, spec, poses in CS.track_cases():
        assert well_separated(CS.reference(spec, poses, R.MP)["decisions"]), name
        assert CS.reference(spec, poses, R.MP)["status"] == CS.reference(spec, poses, R.FLOAT)["status"] == R.VALID, name
    for name, spec, poses, expect in CS.invalid_cases():
        r = CS.reference(spec, poses, R.MP)
        assert r["status"] == expect == CS.reference(spec, poses, R.FLOAT)["status"], (name, r["status"])
        if name != "identical_poses":   # (two identical cameras: the third singular value is exactly the threshold's side by construction)
            assert well_separated([d for d in r["decisions"] if d[0] != "singular_value" or d[1] > 1e-3]), name


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    exe = tmp_path_factory.mktemp("smart") / "smart_native"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "smart_native.cpp"), "-o", str(exe)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]

    def run(jobs):
        """jobs: [(spec, [(kind, own poses)])] -> per job, per step: (status, retri, point, error, [serial, lanes] blocks)"""
        lines = [str(len(jobs))]
        for spec, steps in jobs:
            m = CS.meas_of(spec)
            lines.append(f"{spec.nk} {m.size} {spec.sigma!r}")
            lines.append(" ".join(repr(float(x)) for x in m))
            lines.append(str(len(steps)))
            for kind, poses in steps:
                lines.append(str(kind) + " " + " ".join(repr(float(x)) for x in np.concatenate(poses)))
        path = exe.parent / "case.txt"
        path.write_text("\n".join(lines) + "\n")
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        rows = iter(r.stdout.splitlines())
        out = []
        for spec, steps in jobs:
            res = []
            for kind, _ in steps:
                w = next(rows).split()
                blocks = []
                if kind == 0:
                    for _ in range(2):
                        b = next(rows).split()
                        blocks.append((int(b[0]), np.array([float(x) for x in b[1:]])))
                res.append((int(w[0]), int(w[1]), np.array([float(x) for x in w[2:5]]), float(w[5]), blocks))
            out.append(res)
        return out
    return run


def test_header_on_the_cpu_seeded(native):
    """The header, serially and in the column-per-lane order, on every track case: status equal to the restatement's, the
    augmented Hessian [A b]'[A b] within CS.hessian_bound of the 50-digit one, the error within CS.error_bound.
    Observed on the CPU (both orders alike): |D - H|_F / bound at most 0.0012, |e - e_ref| / bound at most 0.47."""
    cases = CS.track_cases()
    out = native([(spec, [(0, [poses[v] for v in spec.views])]) for _, spec, poses in cases])
    worst_h = worst_e = 0.0
    for (name, spec, poses), res in zip(cases, out):
        status, retri, point, err, blocks = res[0]
        rmp = CS.reference(spec, poses, R.MP)
        assert status == rmp["status"] == R.VALID and retri == 1, name
        bound, d64, backward = CS.hessian_bound(spec, poses)
        m, ncols = 2 * spec.nk - 3, 6 * spec.nk + 1
        for zero, blk in blocks:
            assert zero == 0 and blk.size == m * ncols
            dist = CS.hessian_distance(blk, m, ncols, rmp)
            print(f"{name}: |D-H| {dist:.3e} d64 {d64:.3e} backward {backward:.3e}")
            worst_h = max(worst_h, dist / bound)
            assert dist <= bound, (name, dist, bound)
        eb, e64 = CS.error_bound(spec, poses)
        worst_e = max(worst_e, abs(err - float(rmp["error"])) / eb)
        assert abs(err - float(rmp["error"])) <= eb, (name, err, float(rmp["error"]), eb)
    print("worst ratios", worst_h, worst_e)


def test_header_on_the_cpu_invalid_and_cache(native):
    """no valid point: the restatement's status, the all-zero block, the error 0; and one cache through
    linearize X / error X + 0.1 thr / error X + 10 thr / linearize X, then the same at threshold 0"""
    inv = CS.invalid_cases()
    out = native([(spec, [(0, [poses[v] for v in spec.views])]) for _, spec, poses, _ in inv])
    for (name, spec, poses, expect), res in zip(inv, out):
        status, retri, point, err, blocks = res[0]
        assert status == expect and err == 0.0 and np.all(np.isnan(point)), name
        for zero, blk in blocks:
            assert zero == 1 and not np.any(blk), name
    _, spec, poses = CS.track_cases()[9]
    own = [poses[v] for v in spec.views]
    for thr, expect in ((spec.retriangulation_threshold, [1, 0, 1, 1]), (0.0, [1, 1, 1, 1])):
        s = R.Spec(**{**spec.__dict__, "retriangulation_threshold": thr})
        base = spec.retriangulation_threshold
        seq = [(0, own), (1, [CS.expmap_small(p, 0.1 * base * np.ones(6)) for p in own]),
               (1, [CS.expmap_small(p, 10 * base * np.ones(6)) for p in own]), (0, own)]
        res = native([(s, seq)])[0]
        ref = R.SmartFactor(s, R.FLOAT)
        for (kind, ps), (status, retri, point, err, _) in zip(seq, res):
            r = ref.triangulate_safe(ps)
            assert (status, bool(retri)) == (ref.status, r)
            assert np.allclose(point, ref.point_float(), rtol=0, atol=1e-9)
        assert [r[1] for r in res] == expect
