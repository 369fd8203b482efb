"""Cases for the triangulation tests: the constants of gtsam/geometry/tests/testTriangulation.cpp (lines 38-59 and the tests
below them), typed in as data, and seeded random tracks.  Test infrastructure."""
from __future__ import annotations

import math

import numpy as np

from . import _triangulation_restatement as R

K_SHARED = np.array([1500.0, 1200.0, 0.1, 640.0, 480.0])     # kSharedCal
K_BUNDLER = np.array([1500.0, 0.1, 0.2, 640.0, 480.0])       # twoPosesBundler
LANDMARK = np.array([5.0, 0.5, 1.2])                          # kLandmark
HUBER_UNIT = (R.N_UNIT | R.HUBER, [1.345])


def ypr(y, p, r):
    """Rot3::Ypr = Rz(y) Ry(p) Rx(r)"""
    cy, sy, cp, sp, cr, sr = math.cos(y), math.sin(y), math.cos(p), math.sin(p), math.cos(r), math.sin(r)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    Ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    Rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return Rz @ Ry @ Rx


def compose(a, b):
    return a[0] @ b[0], a[1] + a[0] @ b[1]


UPRIGHT = ypr(-math.pi / 2, 0.0, -math.pi / 2)
POSE1 = (UPRIGHT, np.array([0.0, 0.0, 1.0]))
POSE2 = compose(POSE1, (np.eye(3), np.array([1.0, 0.0, 0.0])))
POSE3 = compose(POSE1, (ypr(0.1, 0.2, 0.1), np.array([0.1, -2.0, -0.1])))
POSE4 = (ypr(math.pi / 2, 0.0, -math.pi / 2), np.array([0.0, 0.0, 1.0]))   # facing the wrong way
IDENTITY = (np.eye(3), np.zeros(3))


def cam(pose, K=K_SHARED, kind=0):
    return R.Camera(np.array(pose[0], float), np.array(pose[1], float), np.array(K, float), kind)


def project(c, p):
    """camera.project(point) in float64 (None behind the camera)"""
    r = R._Cam(c, R.FLOAT).project(np.array([float(x) for x in p], dtype=object))
    return None if r is None else np.array([float(r[0]), float(r[1])])


def known_answers():
    """(name, cameras, measurements, Params, expectation): expectation = ("point", xyz, tol) | ("status", code) |
    ("near", lo, hi) distance from kLandmark"""
    out = []
    c1, c2, c3, c4 = cam(POSE1), cam(POSE2), cam(POSE3), cam(POSE4)
    z1, z2, z3 = project(c1, LANDMARK), project(c2, LANDMARK), project(c3, LANDMARK)
    n1, n2 = z1 + [0.1, 0.5], z2 + [-0.2, 0.3]
    noisy = np.array([4.995, 0.499167, 1.19814])
    P = R.Params
    out += [
        ("twoPoses_1", [c1, c2], [z1, z2], P(), ("point", LANDMARK, 1e-7)),
        ("twoPoses_2", [c1, c2], [z1, z2], P(optimize=True), ("point", LANDMARK, 1e-7)),
        ("twoPoses_3", [c1, c2], [n1, n2], P(), ("point", noisy, 1e-4)),
        ("twoPoses_4", [c1, c2], [n1, n2], P(optimize=True), ("point", noisy, 1e-4)),
    ]
    iso4 = (R.N_ISOTROPIC, [1e-4])
    out += [
        ("twoCamerasUsingLOST_1", [c1, c2], [z1, z2], P(use_lost=True, noise=iso4), ("point", LANDMARK, 1e-12)),
        ("twoCamerasUsingLOST_2", [c1, c2], [n1, n2], P(use_lost=True, noise=iso4), ("point", noisy, 1e-4)),
    ]
    ident = np.array([1.0, 1.0, 0.0, 0.0, 0.0])
    l1, l2 = cam(IDENTITY, ident), cam((np.eye(3), np.array([5.0, 0.0, -5.0])), ident)
    lm = np.array([0.0, 0.0, 1.0])
    x1, x2 = project(l1, lm) + [0.00817, 0.00977], project(l2, lm) + [-0.00610, 0.01969]
    out += [
        ("twoCamerasLOSTvsDLT_lost", [l1, l2], [x1, x2], P(use_lost=True, noise=(R.N_ISOTROPIC, [1e-2])),
         ("point", np.array([0.007, 0.011, 0.945]), 1e-3)),
        ("twoCamerasLOSTvsDLT_dlt", [l1, l2], [x1, x2], P(), ("status", R.VALID)),
    ]
    b1, b2 = cam(POSE1, K_BUNDLER, 1), cam(POSE2, K_BUNDLER, 1)
    zb1, zb2 = project(b1, LANDMARK), project(b2, LANDMARK)
    out += [
        ("twoPosesBundler_1", [b1, b2], [zb1, zb2], P(optimize=True), ("point", LANDMARK, 1e-7)),
        ("twoPosesBundler_2", [b1, b2], [zb1 + [0.1, 0.5], zb2 + [-0.2, 0.3]], P(optimize=True),
         ("point", np.array([4.995, 0.499167, 1.19847]), 1e-3)),
    ]
    m3 = z3 + [0.1, -0.1]
    out += [
        ("fourPoses_1", [c1, c2], [z1, z2], P(), ("point", LANDMARK, 1e-2)),
        ("fourPoses_2", [c1, c2], [n1, n2], P(), ("point", LANDMARK, 1e-2)),
        ("fourPoses_3", [c1, c2, c3], [n1, n2, m3], P(), ("point", LANDMARK, 1e-2)),
        ("fourPoses_3_opt", [c1, c2, c3], [n1, n2, m3], P(optimize=True), ("point", LANDMARK, 1e-2)),
        ("fourPoses_4_cheirality", [c1, c2, c3, c4], [n1, n2, m3, np.array([400.0, 400.0])], P(),
         ("status", R.BEHIND_CAMERA)),
    ]
    # fourPoses_distinct_Ks (:430-490): K1, K2, K3 as below
    K1, K2, K3 = [1500.0, 1200, 0, 640, 480], [1600.0, 1300, 0, 650, 440], [700.0, 500, 0, 640, 480]
    d1, d2, d3 = cam(POSE1, K1), cam(POSE2, K2), cam(POSE3, K3)
    w1, w2, w3 = project(d1, LANDMARK), project(d2, LANDMARK), project(d3, LANDMARK)
    out += [
        ("distinctKs_1", [d1, d2], [w1, w2], P(), ("point", LANDMARK, 1e-2)),
        ("distinctKs_2", [d1, d2], [w1 + [0.1, 0.5], w2 + [-0.2, 0.3]], P(), ("point", LANDMARK, 1e-2)),
        ("distinctKs_3_opt", [d1, d2, d3], [w1 + [0.1, 0.5], w2 + [-0.2, 0.3], w3 + [0.1, -0.1]], P(optimize=True),
         ("point", LANDMARK, 1e-2)),
    ]
    o1 = z1 + [100.0, 120.0]
    out += [
        ("threePoses_robust_clean", [c1, c2, c3], [z1, z2, z3], P(), ("point", LANDMARK, 1e-2)),
        ("threePoses_robust_outlier_dlt", [c1, c2, c3], [o1, z2, z3], P(), ("near", 0.2, 0.5)),
        ("threePoses_robust_outlier_huber", [c1, c2, c3], [o1, z2, z3], P(optimize=True, noise=HUBER_UNIT),
         ("point", LANDMARK, 0.05)),
        ("fourPoses_robust_outlier_dlt", [c1, c1, c2, c3], [o1, z1 + [0.1, 0.2], z2 + [0.2, 0.2], z3 + [0.3, 0.1]], P(),
         ("near", 0.1, 0.5)),
        ("fourPoses_robust_outlier_huber", [c1, c1, c2, c3], [o1, z1 + [0.1, 0.2], z2 + [0.2, 0.2], z3 + [0.3, 0.1]],
         P(optimize=True, noise=HUBER_UNIT), ("point", LANDMARK, 0.05)),
    ]
    safe = dict(rank_tol=1.0, safe=True)
    out += [
        ("outliersAndFar_valid", [d1, d2], [w1, w2], P(landmark_distance_threshold=10, **safe), ("point", LANDMARK, 1e-2)),
        ("outliersAndFar_far", [d1, d2], [w1, w2], P(landmark_distance_threshold=4, **safe), ("status", R.FAR_POINT)),
        ("outliersAndFar_loose", [d1, d2, d3], [w1, w2, w3 + [10.0, -10.0]],
         P(landmark_distance_threshold=10, outlier_threshold=100, **safe), ("status", R.VALID)),
        ("outliersAndFar_outlier", [d1, d2, d3], [w1, w2, w3 + [10.0, -10.0]],
         P(landmark_distance_threshold=10, outlier_threshold=5, **safe), ("status", R.OUTLIER)),
        ("twoIdenticalPoses", [c1, c1], [z1, z1], P(), ("status", R.DEGENERATE)),
        ("onePose", [cam(IDENTITY)], [np.zeros(2)], P(), ("status", R.DEGENERATE)),
    ]
    return out


def check_expectation(name, expect, status, point):
    if expect[0] == "status":
        assert status == expect[1], (name, status)
    elif expect[0] == "point":
        assert status == R.VALID, (name, status)
        assert np.max(np.abs(np.asarray(point, float) - expect[1])) <= expect[2], (name, point)
    else:
        assert status == R.VALID, (name, status)
        d = np.linalg.norm(np.asarray(point, float) - LANDMARK)
        assert expect[1] <= d <= expect[2], (name, d)


# ---- seeded tracks ---------------------------------------------------------------------------------------------------------
def _random_rotation(rng, angle):
    w = rng.normal(size=3)
    w *= angle * rng.uniform() / np.linalg.norm(w)
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) if th == 0 else np.eye(3) + math.sin(th) / th * Kx + (1 - math.cos(th)) / th ** 2 * Kx @ Kx


def draw_track(seed, m, kind=0, noise_px=0.5, shared_cal=True):
    """m cameras on a 4 m disc looking roughly along +z at a point about 8 m away, pixel noise noise_px"""
    rng = np.random.default_rng(seed)
    point = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(6, 10)])
    cams, meas = [], []
    for i in range(m):
        t = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-0.5, 0.5)])
        Rm = _random_rotation(rng, 0.15)
        if kind == 1:
            K = np.array([rng.uniform(900, 1100), rng.uniform(-0.05, 0.05), rng.uniform(-0.02, 0.02), 0.0, 0.0])
        elif shared_cal:
            K = np.array([1000.0, 950.0, 0.2, 320.0, 240.0])
        else:
            K = np.array([rng.uniform(900, 1100), rng.uniform(900, 1100), rng.uniform(-0.5, 0.5), 320.0, 240.0])
        c = R.Camera(Rm, t, K, kind)
        cams.append(c)
        meas.append(project(c, point) + rng.normal(scale=noise_px, size=2) if noise_px else project(c, point))
    return cams, meas, point


def seeded_track(seed, m, params, kind=0, noise_px=0.5, shared_cal=True, max_tries=20):
    """the first seed >= `seed` (in steps of 1000) whose 50-digit run keeps every decision away from its threshold;
    returns (cameras, measurements, float64 Result, 50-digit Result, seeds replaced)"""
    for k in range(max_tries):
        cams, meas, _ = draw_track(seed + 1000 * k, m, kind, noise_px, shared_cal)
        mp = R.triangulate(cams, meas, params, R.MP)
        if R.well_separated(mp.decisions):
            return cams, meas, R.triangulate(cams, meas, params, R.FLOAT), mp, k
    raise AssertionError("no well-separated seed found")


def pack(tracks, kind=0):
    """tracks = [(cameras, measurements)] -> the arrays of gsx_triangulate: cameras (n, 12 or 17), calibrations (n, 5),
    track_ptr, obs_camera, obs_xy; one camera entry per observation"""
    cams, cal, ptr, oc, xy = [], [], [0], [], []
    for cs, ms in tracks:
        for c, z in zip(cs, ms):
            oc.append(len(cams))
            st = c.state()
            cams.append(st if kind == 1 else st[:12])
            cal.append(st[12:17])
            xy.append(np.asarray(z, float))
        ptr.append(len(oc))
    w = 17 if kind == 1 else 12
    return (np.array(cams, float).reshape(-1, w), np.array(cal, float).reshape(-1, 5), np.array(ptr, np.int64),
            np.array(oc, np.int32), np.array(xy, float).reshape(-1, 2))


# ---- bounds (no figure of the code under test enters them) ---------------------------------------------------------------------
U = 2.0 ** -53


def gamma(m):
    """Unit-roundoff multiple of the streaming linear stage for a track of m observations: 16 u for forming a row (the
    products of K [R' | -R' t] and p P2 - Pk: at most 8 roundings per entry, doubled for the LOST scale q), 8 u per Givens
    rotation an entry of the triangle can meet (Higham, Accuracy and Stability, Lemma 19.9: 6 sqrt(2) u per rotation) over
    the 2m rows of the track plus the 6 x 4 rows of the pairwise merges plus the 4 columns, and 4 u for each of the 30
    sweeps x 6 rotations the one-sided Jacobi step is capped at (csrc/triangulate_math.h: dlt_finish; the pivoted QR of LOST
    has 3 rotations)."""
    return U * (16 + 8 * (2 * m + 24 + 4) + 4 * 30 * 6)


def _float_matrix(M):
    return np.array([[float(v) for v in row] for row in M])


def forward_bound(cams, meas, fl, mp):
    """ten times the float64 restatement's own distance from the 50-digit point (DESIGN §5's margin), or the first-order
    bound where that is larger.  DLT: gamma sigma_1 / (sigma_3 - sigma_4) (1 + |x|^2).  LOST: the least-squares
    perturbation bound for |dA| <= gamma |A|_F, |db| <= gamma |b| (Higham, Theorem 20.1, first order):
    gamma ((|A|_F |x| + |b|) / sigma_3 + |A|_F |r| / sigma_3^2), r the residual."""
    x = np.array([float(v) for v in mp.linear_point])
    own = np.linalg.norm(np.asarray(fl.linear_point, float) - x)
    s = [float(v) for v in mp.sigma]
    g = gamma(len(cams))
    if len(s) == 4:
        first = g * s[0] / (s[2] - s[3]) * (1 + x.dot(x))
    else:
        A = _float_matrix(mp.A)
        sv = np.linalg.svd(A[:, :3], compute_uv=False)
        nA, r = np.linalg.norm(A[:, :3]), np.linalg.norm(A[:, :3] @ x - A[:, 3])
        first = g * ((nA * np.linalg.norm(x) + np.linalg.norm(A[:, 3])) / sv[2] + nA * r / sv[2] ** 2)
    return max(10 * own, first)


def backward_residual(mp, point):
    """|A [x; 1]| / |[x; 1]| (DLT) or the normal-equations residual |A'(A x - b)| (LOST) in the 50-digit system"""
    A = np.array([[float(v) for v in row] for row in mp.A])
    x = np.asarray(point, float)
    if len(mp.sigma) == 4:
        h = np.append(x, 1.0)
        return np.linalg.norm(A @ h) / np.linalg.norm(h)
    return np.linalg.norm(A[:, :3].T @ (A[:, :3] @ x - A[:, 3]))


def backward_bound(cams, meas, mp):
    """DLT: sigma_4 + gamma |A|_F.  LOST: the normal-equations residual of the solution of a system perturbed by
    |dA| <= gamma |A|_F, |db| <= gamma |b|: 2 gamma |A|_F (|A|_F |x| + |b|), first order"""
    g = gamma(len(cams))
    A = _float_matrix(mp.A)
    if len(mp.sigma) == 4:
        return float(mp.sigma[3]) + g * np.linalg.norm(A)
    x = np.array([float(v) for v in mp.linear_point])
    nA = np.linalg.norm(A[:, :3])
    return g * nA * (nA * np.linalg.norm(x) + np.linalg.norm(A[:, 3])) * 2


def refined_bound(cams, meas, fl, mp):
    """the refined point: ten times the float64 restatement's own distance from the 50-digit refined point, or the
    forward bound of the linear stage where that is larger (an accepted LM step does not amplify an error of its starting
    point: the damped Gauss-Newton map contracts near the minimum)"""
    x = np.array([float(v) for v in mp.point])
    return max(10 * np.linalg.norm(np.asarray(fl.point, float) - x), forward_bound(cams, meas, fl, mp))


# ---- the seeded cases every host and GPU test draws, computed once per process ----------------------------------------------
LENGTHS = (2, 3, 63, 64, 65, 129)   # 64 = the class split (one below / at / above)
LINEAR_NOISE = (R.N_ISOTROPIC, [0.5])
REFINE_NOISES = (None, (R.N_DIAGONAL, [0.5, 0.7]), (R.N_GAUSSIAN, [2.0, 0.3, 0.0, 1.5]), (R.N_UNIT | R.HUBER, [1.345]),
                 (R.N_ISOTROPIC | R.CAUCHY, [0.5, 2.0]), (R.N_UNIT | R.TUKEY, [30.0]))
REFINE_SHAPES = ((2, 0.5), (4, 8.0), (7, 3.0), (65, 2.0))   # (track length, pixel noise)
_cache = {}


def linear_case(use_lost, kind, m):
    """(cameras, measurements, float64 Result, 50-digit Result, seeds replaced) of the linear-stage tests"""
    key = ("linear", use_lost, kind, m)
    if key not in _cache:
        P = R.Params(use_lost=use_lost, noise=LINEAR_NOISE)
        _cache[key] = seeded_track(100 + m, m, P, kind, shared_cal=(m % 2 == 0))
    return _cache[key]


def refine_params(noise):
    return R.Params(optimize=True, noise=noise, safe=True, landmark_distance_threshold=50.0, outlier_threshold=40.0)


def refine_case(noise_index, m, px):
    key = ("refine", noise_index, m, px)
    if key not in _cache:
        _cache[key] = seeded_track(7 + m, m, refine_params(REFINE_NOISES[noise_index]), 0, noise_px=px)
    return _cache[key]


def native_input(params, cams, tracks, sensors=None):
    """the text the stand-alone host program reads; tracks = [[(camera index, u, v)]]"""
    nk, npar = (-1, []) if params.noise is None else (params.noise[0], list(params.noise[1]))
    kind = 0 if nk < 0 else nk
    p = (npar + [0.0] * 5)[:5]
    lines = [" ".join(repr(float(v)) if isinstance(v, float) else str(int(v)) for v in
                      [float(params.rank_tol), int(params.optimize), int(params.use_lost), int(params.safe),
                       float(R.lost_sigma(params.noise)), float(params.landmark_distance_threshold),
                       float(params.outlier_threshold), kind] + [float(x) for x in p]), str(len(cams))]
    for i, c in enumerate(cams):
        s = None if sensors is None else sensors[i]
        row = [str(c.kind), "1" if s is not None else "0"] + [repr(float(v)) for v in c.state()]
        if s is not None:
            row += [repr(float(v)) for v in np.concatenate([np.asarray(s[0], float).reshape(9), np.asarray(s[1], float)])]
        lines.append(" ".join(row))
    lines.append(str(len(tracks)))
    for tr in tracks:
        lines.append(" ".join([str(len(tr))] + [f"{int(c)} {float(u)!r} {float(v)!r}" for c, u, v in tr]))
    return "\n".join(lines) + "\n"
