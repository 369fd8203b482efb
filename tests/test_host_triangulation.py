"""Triangulation without a GPU: the restatement against the reference's known answers, the per-track arithmetic of the
kernels (csrc/triangulate_math.h) as a stand-alone host program under the sanitizers against the restatement, the track
grouping, the exports, and the condition on the seeded inputs that the GPU tests rely on."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gtsam_petercdev_amd as gt
from gtsam_petercdev_amd import _abi as A, _lib, datasets
from tests import _triangulation_cases as CS
from tests import _triangulation_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from gtsam_petercdev_amd import build
    build.build_lib()
    return _lib.load()


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tri") / "triangulate_native"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "triangulate_native.cpp"), "-o", str(exe)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]

    def run(params, cams, tracks, sensors=None):
        path = exe.parent / "case.txt"
        path.write_text(CS.native_input(params, cams, tracks, sensors))
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        rows = [l.split() for l in r.stdout.splitlines()]
        assert len(rows) == 2 * len(tracks)
        return [(int(w[0]), np.array([float(x) for x in w[1:4]]), int(w[4]), int(w[5])) for w in rows]
    return run


def test_restatement_reproduces_the_reference_known_answers():
    for name, cams, meas, P, expect in CS.known_answers():
        for X in (R.FLOAT, R.MP):
            r = R.triangulate(cams, meas, P, X)
            CS.check_expectation(name, expect, r.status, r.point)
    ka = {n: (c, m, p) for n, c, m, p, _ in CS.known_answers()}
    lost = R.triangulate(*ka["twoCamerasLOSTvsDLT_lost"]).point
    dlt = R.triangulate(*ka["twoCamerasLOSTvsDLT_dlt"]).point
    lm = np.array([0.0, 0.0, 1.0])
    assert np.linalg.norm(lm - lost) <= np.linalg.norm(lm - dlt)
    # :373 / :418 — the non-robust refinement stays close to DLT
    for n in ("threePoses", "fourPoses"):
        c, m, p = ka[n + "_robust_outlier_dlt"]
        a2 = R.triangulate(c, m, p).point
        a3 = R.triangulate(c, m, R.Params(optimize=True)).point
        assert np.max(np.abs(a2 - a3)) <= 0.1


def test_header_on_the_cpu_known_answers(native):
    for name, cams, meas, P, expect in CS.known_answers():
        tr = [[(i, z[0], z[1]) for i, z in enumerate(meas)]]
        serial, wave = native(P, cams, tr)
        for st, pt, _, _ in (serial, wave):
            CS.check_expectation(name, expect, st, pt)
            assert (st == R.VALID) == bool(np.all(np.isfinite(pt)))


@pytest.mark.parametrize("use_lost", [False, True])
@pytest.mark.parametrize("kind", [0, 1])
def test_header_on_the_cpu_seeded(native, use_lost, kind):
    """statuses equal the restatement's; the linear point holds the forward bound and the backward bound of
    tests/_triangulation_cases.py, for the serial and for the merged (wave) order, at every length class"""
    P = R.Params(use_lost=use_lost, noise=CS.LINEAR_NOISE)
    cases = [CS.linear_case(use_lost, kind, m) for m in CS.LENGTHS]
    cams = [c for cs, _, _, _, _ in cases for c in cs]
    tracks, base = [], 0
    for cs, ms, _, _, _ in cases:
        tracks.append([(base + i, z[0], z[1]) for i, z in enumerate(ms)])
        base += len(cs)
    out = native(P, cams, tracks)
    for k, (cs, ms, fl, mp, _) in enumerate(cases):
        for st, pt, _, _ in out[2 * k:2 * k + 2]:
            assert st == mp.status == fl.status
            if st != R.VALID:
                continue
            x = np.array([float(v) for v in mp.point])
            assert np.linalg.norm(pt - x) <= CS.forward_bound(cs, ms, fl, mp), (len(cs), use_lost, kind)
            assert CS.backward_residual(mp, pt) <= CS.backward_bound(cs, ms, mp), (len(cs), use_lost, kind)


@pytest.mark.parametrize("noise_index", range(len(CS.REFINE_NOISES)))
def test_header_on_the_cpu_refinement(native, noise_index):
    """LM iteration and trial counts equal the 50-digit restatement's; the refined point holds CS.refined_bound"""
    P = CS.refine_params(CS.REFINE_NOISES[noise_index])
    for m, px in CS.REFINE_SHAPES:
        cs, ms, fl, mp, _ = CS.refine_case(noise_index, m, px)
        out = native(P, cs, [[(i, z[0], z[1]) for i, z in enumerate(ms)]])
        for st, pt, it, tr in out:
            assert st == mp.status
            assert (it, tr) == (mp.iterations, mp.trials) == (fl.iterations, fl.trials)
            if st == R.VALID:
                x = np.array([float(v) for v in mp.point])
                assert np.linalg.norm(pt - x) <= CS.refined_bound(cs, ms, fl, mp), (noise_index, m)


def test_header_on_the_cpu_edges(native):
    """0 and 1 observations, collinear LOST partners (fallback search, and none usable), body_P_sensor, a Cal3Bundler loop
    that does not converge: statuses, NaN-free VALID points"""
    c0 = CS.cam(CS.IDENTITY, [1000.0, 1000, 0, 0, 0])
    P = R.Params()
    out = native(P, [c0], [[], [(0, 1.0, 2.0)]])
    assert [o[0] for o in out] == [R.DEGENERATE] * 4
    # cameras 0 and 1 coincide (baseline 0: den == 0 for the pair), camera 2 is apart: the search finds k = 2
    point = np.array([0.3, -0.2, 6.0])
    ca = CS.cam((np.eye(3), np.zeros(3)), [1000.0, 1000, 0, 0, 0])
    cb = CS.cam((np.eye(3), np.array([1.5, 0.2, 0.0])), [1000.0, 1000, 0, 0, 0])
    cams, meas = [ca, ca, cb], [CS.project(ca, point), CS.project(ca, point), CS.project(cb, point)]
    PL = R.Params(use_lost=True)
    ref = R.triangulate(cams, meas, PL, R.MP)
    assert ref.status == R.VALID
    out = native(PL, cams, [[(i, z[0], z[1]) for i, z in enumerate(meas)]])
    for st, pt, _, _ in out:
        assert st == R.VALID and np.linalg.norm(pt - point) < 1e-9
    # every partner collinear: three coincident cameras
    cams, meas = [ca, ca, ca], [CS.project(ca, point)] * 3
    assert R.triangulate(cams, meas, PL, R.MP).status == R.DEGENERATE
    assert [o[0] for o in native(PL, cams, [[(i, z[0], z[1]) for i, z in enumerate(meas)]])] == [R.DEGENERATE] * 2
    # body_P_sensor: the same answer as with the composed pose
    sensor = (CS.ypr(0.05, -0.02, 0.03), np.array([0.1, 0.0, -0.05]))
    body = [CS.cam(p) for p in (CS.POSE1, CS.POSE2, CS.POSE3)]
    composed = [CS.cam(CS.compose((b.R, b.t), sensor)) for b in body]
    meas = [CS.project(c, CS.LANDMARK) + [0.2, -0.1] for c in composed]
    tr = [[(i, z[0], z[1]) for i, z in enumerate(meas)]]
    a = native(P, body, tr, [sensor] * 3)
    ref = R.triangulate(body, meas, P, R.MP, sensors=[sensor] * 3)
    ref2 = R.triangulate(composed, meas, P, R.FLOAT)
    for st, pt, _, _ in a:
        assert st == R.VALID
        assert np.linalg.norm(pt - np.array([float(v) for v in ref.point])) <= CS.forward_bound(composed, meas, ref2, ref)
    # a distortion the fixed-point loop cannot undo
    bad = CS.cam(CS.IDENTITY, [1000.0, 40.0, 0.0, 0.0, 0.0], 1)
    meas = [np.array([900.0, 800.0]), np.array([850.0, 790.0])]
    assert R.triangulate([bad, bad], meas, P, R.MP).status == R.CALIBRATION_FAILED
    assert [o[0] for o in native(P, [bad, bad], [[(0, *meas[0]), (1, *meas[1])]])] == [R.CALIBRATION_FAILED] * 2


def test_seeded_inputs_keep_clear_of_every_threshold():
    """In the 50-digit restatement no decision quantity lies within a relative 1e-6 of its threshold, on every seeded
    case the host and GPU tests draw (CS.linear_case, CS.refine_case) and on a further family of short tracks; a seed that
    violates this is replaced by the next one, and fewer than 5 % of the drawn seeds are"""
    drawn = replaced = 0
    cases = [CS.linear_case(l, k, m) for l in (False, True) for k in (0, 1) for m in CS.LENGTHS]
    cases += [CS.refine_case(n, m, px) for n in range(len(CS.REFINE_NOISES)) for m, px in CS.REFINE_SHAPES]
    for use_lost in (False, True):
        for optimize in (False, True):
            P = R.Params(use_lost=use_lost, optimize=optimize, noise=(R.N_ISOTROPIC, [0.5]), safe=True,
                         landmark_distance_threshold=50.0, outlier_threshold=40.0)
            cases += [CS.seeded_track(10 * m + s, m, P, s % 2) for m in (2, 3, 4, 5, 8, 12) for s in range(4)]
    for _, _, fl, mp, k in cases:
        drawn += 1 + k
        replaced += k
        assert R.well_separated(mp.decisions)
        assert fl.status == mp.status and (fl.iterations, fl.trials) == (mp.iterations, mp.trials)
    print(f"seeds drawn {drawn}, replaced {replaced}")
    assert replaced < 0.05 * drawn, (replaced, drawn)


def test_track_grouping(lib):
    arr = datasets.synth_bal_arrays(8, 60, 200, seed=1)
    lm, ptr, of = _lib.triangulation_tracks(arr)
    rlm, rptr, rof = R.group_tracks(arr)
    assert lm.tolist() == rlm and ptr.tolist() == list(rptr) and of.tolist() == rof
    # a mixed graph: projection factors (one with a sensor), other factor types ignored, factor order kept per landmark
    g, v = gt.NonlinearFactorGraph(), gt.Values()
    K = gt.Cal3_S2(1500, 1200, 0.1, 640, 480)
    for j, p in enumerate((CS.POSE1, CS.POSE2, CS.POSE3)):
        v.insert(gt.X(j), gt.Pose3(gt.Rot3(p[0]), p[1]))
    for l in range(2):
        v.insert(gt.L(l), gt.Point3(5, 0.5 + l, 1.2))
    g.add(gt.PriorFactor(gt.X(0), v.at(gt.X(0)), gt.noiseModel.Isotropic.Sigma(6, 0.1)))
    for j in (2, 0, 1):
        for l in (1, 0):
            g.add(gt.GenericProjectionFactor(gt.Point2(600 + j, 400 + l), None, gt.X(j), gt.L(l), K,
                                             gt.Pose3() if j == 1 else None))
    arr = g.to_arrays(v)
    lm, ptr, of = _lib.triangulation_tracks(arr)
    rlm, rptr, rof = R.group_tracks(arr)
    assert lm.tolist() == rlm and ptr.tolist() == list(rptr) == [0, 3, 6] and of.tolist() == rof == [2, 4, 6, 1, 3, 5]
    # a landmark seen by both camera kinds
    bal = datasets.synth_bal_arrays(3, 5, 10, seed=2)
    pose_var = None
    f = _lib.load().gsx_triangulation_tracks
    f.restype = C.c_int32
    bad = A.ProblemArrays(bal.var_keys, bal.var_types.copy(), bal.var_dims, bal.f_type.copy(), bal.f_rows, bal.f_key_ptr,
                          bal.f_vars, bal.f_meas_ptr, bal.meas, bal.f_noise_kind, bal.f_noise_ptr, bal.noise)
    first_sfm = int(np.flatnonzero(bad.f_type == A.F_SFM)[0])
    bad.f_type[first_sfm] = A.F_PROJECTION
    d = bad.desc()
    assert f(C.byref(d), None, None, None, None, None) == A.GSX_E_INVALID
    del pose_var


def test_numeric_entries_need_a_device(lib):
    cams, meas = [CS.cam(CS.POSE1), CS.cam(CS.POSE2)], [np.array([600.0, 400.0])] * 2
    c, k, ptr, oc, xy = CS.pack([(cams, meas)])
    if _lib.device_count() == 0:
        with pytest.raises(A.GsxError) as e:
            _lib.triangulate(A.CAMERA_POSE3_CAL3_S2, c, k, ptr, oc, xy)
        assert e.value.status == A.GSX_E_NO_DEVICE
        with pytest.raises(A.GsxError) as e:
            _lib.triangulate_landmarks(datasets.synth_bal_arrays(3, 5, 10, seed=2))
        assert e.value.status == A.GSX_E_NO_DEVICE
    # refusals come before the device: constrained noise, a zero sigma, a camera index out of range
    p = _lib.triangulation_params_default()
    assert (p.rank_tol, p.optimize, p.use_lost, p.noise_kind, p.safe) == (1e-9, 0, 0, -1, 0)
    for kind, sig in ((A.NOISE_CONSTRAINED, [1.0, 1.0]), (A.NOISE_ISOTROPIC, [0.0]), (A.NOISE_DIAGONAL, [1.0, 0.0])):
        p.noise_kind = kind
        for i, s in enumerate(sig):
            p.noise[i] = s
        with pytest.raises(A.GsxError) as e:
            _lib.triangulate(A.CAMERA_POSE3_CAL3_S2, c, k, ptr, oc, xy, p)
        assert e.value.status == A.GSX_E_INVALID
    with pytest.raises(A.GsxError) as e:
        _lib.triangulate(A.CAMERA_POSE3_CAL3_S2, c, k, ptr, oc + 5, xy)
    assert e.value.status == A.GSX_E_INVALID
    out = np.zeros(5)
    f = _lib.load().gsx_triangulate_timings
    f.restype = C.c_int32
    assert f(A._dptr(out), C.c_int32(4)) == A.GSX_E_INVALID
    assert set(_lib.triangulate_timings()) == set(_lib.TRIANGULATE_TIMING_NAMES)
    assert gt.TriangulationParameters().rankTolerance == 1.0 and not gt.TriangulationResult(1).valid()
