"""Seeded case generators of the translation-averaging tests (tests/test_host_translation.py asserts their input
conditions on the CPU; tests/test_gpu_translation.py runs them on the device)."""
import math

import numpy as np

from gtsam_petercdev_amd import _abi as A
from tests import _factor_restatement as R
from tests import _translation_restatement as T

V = A.VAR_VECTOR
LIST_LENGTHS = (1, 63, 64, 65, 257)          # a wave and a 256-thread block boundary
NOISES = ("unit", "isotropic", "diagonal", "gaussian", "huber")
SCALE_MODES = ("positive", "negative", "zero")
MIN_SEPARATION = 0.1                         # |Tb - Ta| >= MIN_SEPARATION max(|Ta|, |Tb|)


def unit(v):
    v = np.asarray(v, dtype=float)
    return v / math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def separated_points(rng, n, lo=-3.0, hi=3.0):
    """n points, each apart from the one before it by 4 MIN_SEPARATION of their larger norm.  Pairs that are not consecutive
    (the wrap-around and the longer joins of mixed_graph and noisy_graph) are not covered by this: the host test checks the
    separation of every factor of every graph actually used."""
    pts = []
    while len(pts) < n:
        p = rng.uniform(lo, hi, 3)
        if pts and np.linalg.norm(p - pts[-1]) < 4 * MIN_SEPARATION * max(np.linalg.norm(p), np.linalg.norm(pts[-1])):
            continue
        pts.append(p)
    return pts


def factor_graph(family, n_factors, noise, seed, scale_mode="positive"):
    """n_factors factors of one family on a chain of n_factors + 1 translations; BATA: a scale variable per factor."""
    rng = np.random.default_rng(seed)
    pts = separated_points(rng, n_factors + 1)
    var_list = [(i, V, 3) for i in range(n_factors + 1)]
    values = list(pts)
    factors = []
    for i in range(n_factors):
        z = unit(unit(pts[i + 1] - pts[i]) + rng.normal(0, 0.05, 3))
        kind, params = R.noise_of(rng, noise, 3)
        if family == "translation":
            factors.append((A.F_TRANSLATION, [i, i + 1], 3, z, kind, params))
        else:
            s = {"positive": rng.uniform(0.2, 2.0), "negative": -rng.uniform(0.2, 2.0), "zero": 0.0}[scale_mode]
            var_list.append((1000 + i, V, 1))
            values.append(np.array([s]))
            factors.append((A.F_BILINEAR_TRANSLATION, [i, i + 1, n_factors + 1 + i], 3, z, kind, params))
    return R.make_arrays(var_list, factors, np.concatenate(values))


FAMILIES = [("translation", "positive")] + [("bata", m) for m in SCALE_MODES]
# every seeded single-family case of the device tests, (family, scale mode, factors, noise, seed): 65 factors (a wave and one
# lane) under each noise model, and each list length under a noise model that rotates with it
FACTOR_CASES = ([(fam, mode, 65, noise, 300 + k) for fam, mode in FAMILIES for k, noise in enumerate(NOISES)] +
                [(fam, mode, n, NOISES[n % 5], 400 + n) for fam, mode in FAMILIES for n in LIST_LENGTHS])


def factor_case(case):
    fam, mode, n, noise, seed = case
    return factor_graph(fam, n, noise, seed, scale_mode=mode)


def mixed_graph(with_new=True):
    """Both families beside priors and between factors on VECTOR(3) (and one Pose2 chain, so that a typed list is filled
    too); with_new = False: the same graph without the translation factors."""
    rng = np.random.default_rng(5)
    n = 20
    pts = separated_points(rng, n)
    var_list = [(i, V, 3) for i in range(n)] + [(100 + i, A.VAR_POSE2, 3) for i in range(4)] + [(1000 + i, V, 1) for i in range(n)]
    values = pts + [np.array([1.0 * i, 0.2 * i, 0.1 * i]) for i in range(4)] + [np.array([rng.uniform(-1.5, 1.5)]) for _ in range(n)]
    factors = []

    def add(is_new, *fac):
        if with_new or not is_new:
            factors.append(fac)
    add(False, A.F_PRIOR, [0], 3, pts[0] + 0.01, A.NOISE_ISOTROPIC, [0.1])
    add(False, A.F_PRIOR, [n], 3, values[n], A.NOISE_DIAGONAL, [0.1, 0.1, 0.05])
    for i in range(3):
        add(False, A.F_BETWEEN, [n + i, n + i + 1], 3, R.pose2_between(values[n + i], values[n + i + 1]) + 0.01, A.NOISE_ISOTROPIC, [0.1])
    for i in range(n):
        j = (i + 1) % n
        z = unit(unit(pts[j] - pts[i]) + rng.normal(0, 0.05, 3))
        add(False, A.F_BETWEEN, [i, j], 3, pts[j] - pts[i] + 0.02, A.NOISE_ISOTROPIC, [0.3])
        add(True, A.F_TRANSLATION, [i, j], 3, z, *R.noise_of(rng, NOISES[i % 5], 3))
        add(True, A.F_BILINEAR_TRANSLATION, [i, j, n + 4 + i], 3, z, *R.noise_of(rng, NOISES[(i + 2) % 5], 3))
        add(False, A.F_PRIOR, [n + 4 + i], 1, [1.0], A.NOISE_ISOTROPIC, [0.5])
    return R.make_arrays(var_list, factors, np.concatenate(values))


def noisy_graph(n=12, seed=11, bilinear_share=0.5):
    """The graph of the generic-path tests: n translations, each joined to the next three by a translation factor (half of
    them BATA with a scale variable and a prior on it), noisy directions, priors on two nodes (gauge and scale), the values
    perturbed from the truth."""
    rng = np.random.default_rng(seed)
    pts = separated_points(rng, n, -4.0, 4.0)
    var_list = [(i, V, 3) for i in range(n)]
    values = [p + rng.normal(0, 0.05, 3) for p in pts]
    factors = [(A.F_PRIOR, [0], 3, pts[0], A.NOISE_ISOTROPIC, [0.01]), (A.F_PRIOR, [1], 3, pts[1], A.NOISE_ISOTROPIC, [0.01])]
    ns = 0
    for i in range(n):
        for k in (1, 2, 3):
            j = (i + k) % n
            d = pts[j] - pts[i]
            z = unit(unit(d) + rng.normal(0, 0.01, 3))
            if rng.uniform() < bilinear_share:
                var_list.append((1000 + ns, V, 1))
                values.append(np.array([1.0 / np.linalg.norm(d) * (1 + rng.normal(0, 0.02))]))
                factors.append((A.F_BILINEAR_TRANSLATION, [i, j, n + ns], 3, z, A.NOISE_ISOTROPIC, [0.05]))
                ns += 1
            else:
                factors.append((A.F_TRANSLATION, [i, j], 3, z, A.NOISE_ISOTROPIC, [0.05]))
    return R.make_arrays(var_list, factors, np.concatenate(values))


# ---- MFAS ----------------------------------------------------------------------------------------------------------------
# (nodes, directions): every n and every D of the issue; then D = 2500, more than the 256 x 8 workgroups a launch takes at
# most, so that the grid-stride runs with no cap; and 5003 nodes, 85 KB of LDS: beyond the default dynamic limit, one
# workgroup per CU
MFAS_SHAPES = ((2, 2), (5, 1), (64, 48), (65, 300), (300, 2), (5, 2500), (5003, 2))
# GSX_MFAS_MAX_GRID of the capped reruns (tests/test_gpu_translation.py): 300 directions on 7 workgroups (43 directions
# each, the last two 42), both directions of the 85 KB case in one workgroup
MFAS_GRID_CAPS = {(65, 300): 7, (5003, 2): 1, (5, 2500): 3}
HEURISTIC_MARGIN, ROOT_MARGIN = 1e-9, 1e-10
_mfas_cache = {}


def _mfas_draw(n, n_dirs, seed):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-5, 5, (n, 3))
    pairs = {(i, (i + 1) % n) if i < (i + 1) % n else ((i + 1) % n, i) for i in range(n)} if n > 2 else {(0, 1)}
    want = min(3 * n, n * (n - 1) // 2)       # average degree about 6
    while len(pairs) < want:
        a, b = (int(x) for x in rng.choice(n, 2, replace=False))
        pairs.add((a, b) if a < b else (b, a))
    key1, key2, dirs = [], [], []
    for a, b in sorted(pairs):
        if rng.uniform() < 0.5:
            a, b = b, a
        d = unit(pos[b] - pos[a]) + rng.normal(0, 0.05, 3)
        if rng.uniform() < 0.15:              # an outlier
            d = rng.normal(0, 1, 3)
        key1.append(10 * a + 3)               # (keys that are not the node indices)
        key2.append(10 * b + 3)
        dirs.append(unit(d))
    proj = np.array([unit(rng.normal(0, 1, 3)) for _ in range(n_dirs)])
    return np.array(key1, np.uint64), np.array(key2, np.uint64), np.array(dirs), proj


def mfas_case(n, n_dirs):
    """A seeded random graph with its restated result, computed once: dict(key1, key2, dirs, proj, weights [D][pair],
    ordering [D], outlier [D][pair], margins).  The first seed whose restated run keeps both margins on every direction is
    used: a seed is left out HERE, never at comparison time."""
    if (n, n_dirs) in _mfas_cache:
        return _mfas_cache[(n, n_dirs)]
    for seed in range(1000 * n + n_dirs, 1000 * n + n_dirs + 50):
        key1, key2, dirs, proj = _mfas_draw(n, n_dirs, seed)
        weights, orderings, outlier, heur, root = [], [], [], math.inf, math.inf
        for d in range(n_dirs):
            w = T.mfas_edge_weights(key1, key2, dirs, proj[d])
            order, m = T.mfas_ordering(w)
            heur, root = min(heur, m["heuristic"]), min(root, m["root"])
            if heur < HEURISTIC_MARGIN or root < ROOT_MARGIN:
                break
            weights.append(w)
            orderings.append(order)
            outlier.append(T.mfas_weights_for_ordering(w, order))
        else:
            case = dict(seed=seed, key1=key1, key2=key2, dirs=dirs, proj=proj, weights=weights, ordering=orderings,
                        outlier=outlier, margins=dict(heuristic=heur, root=root))
            _mfas_cache[(n, n_dirs)] = case
            return case
    raise AssertionError(f"no seed with the margins for n = {n}, D = {n_dirs}")


# the reference's two 4-node cases (gtsam/sfm/tests/testMFAS.cpp:25-97)
MFAS_EDGES = [(3, 2), (0, 1), (3, 1), (1, 2), (0, 2), (3, 0)]
MFAS_WEIGHTS1 = [2, 1.5, 0.5, 0.25, 1, 0.75]
MFAS_WEIGHTS2 = [0.5, 0.75, -0.25, 0.75, 1, 0.5]


# ---- TranslationRecovery: the topologies of tests/testTranslationRecovery.cpp --------------------------------------------
def simulate(positions, edges, sigma=0.01):
    """TranslationRecovery::SimulateMeasurements: Unit3(Tb - Ta) — (0, 0, 0) stays — with Isotropic::Sigma(3, 0.01)."""
    out = []
    for a, b in edges:
        d = np.asarray(positions[b], dtype=float) - np.asarray(positions[a], dtype=float)
        n = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        out.append((a, b, d / n if n > 0 else d, A.NOISE_ISOTROPIC, [sigma]))
    return out


_P3 = {0: (0, 0, 0), 1: (2, 0, 0), 3: (1, -1, 0)}
_HARD = (0, 1, (2.0, 0.0, 0.0), A.NOISE_CONSTRAINED, [0.0, 0.0, 0.0, 1e2, 1e2, 1e2])      # Constrained::All(3, 1e2)
# name: (positions, unit edges, scale, between edges, expected {key: point}, tolerance)
RECOVERY_CASES = {
    "two_poses": ({0: (0, 0, 0), 1: (2, 0, 0)}, [(0, 1)], 3.0, [], {0: (0, 0, 0), 1: (3, 0, 0)}, 1e-8),
    "three_poses": (_P3, [(0, 1), (1, 3), (3, 0)], 3.0, [], {0: (0, 0, 0), 1: (3, 0, 0), 3: (1.5, -1.5, 0)}, 1e-8),
    "three_with_zero_edge": ({0: (0, 0, 0), 1: (2, 0, 0), 2: (2, 0, 0)}, [(0, 1), (1, 2)], 3.0, [],
                             {0: (0, 0, 0), 1: (3, 0, 0), 2: (3, 0, 0)}, 1e-8),
    "four_with_zero_edge": ({0: (0, 0, 0), 1: (2, 0, 0), 2: (2, 0, 0), 3: (1, -1, 0)}, [(0, 1), (1, 2), (1, 3), (3, 0)], 4.0, [],
                            {0: (0, 0, 0), 1: (4, 0, 0), 2: (4, 0, 0), 3: (2, -2, 0)}, 1e-8),
    "all_zero": ({0: (0, 0, 0), 1: (0, 0, 0), 2: (0, 0, 0)}, [(0, 1), (1, 2), (2, 0)], 4.0, [],
                 {0: (0, 0, 0), 1: (0, 0, 0), 2: (0, 0, 0)}, 1e-8),
    "soft_between": (_P3, [(0, 1), (0, 3), (1, 3)], 0.0, [(0, 3, (1.0, -1.0, 0.0), A.NOISE_ISOTROPIC, [1e-2])],
                     {0: (0, 0, 0), 1: (2, 0, 0), 3: (1, -1, 0)}, 1e-4),
    "hard_between": (_P3, [(0, 1), (0, 3), (1, 3)], 0.0, [_HARD], {0: (0, 0, 0), 1: (2, 0, 0), 3: (1, -1, 0)}, 1e-4),
    "between_only_node": (_P3, [(0, 1), (0, 3), (1, 3)], 0.0, [_HARD, (0, 4, (1.0, 2.0, 1.0), A.NOISE_UNIT, [])],
                          {0: (0, 0, 0), 1: (2, 0, 0), 3: (1, -1, 0), 4: (1, 2, 1)}, 1e-4),
}


def recovery_inputs(name):
    positions, edges, scale, between, expected, tol = RECOVERY_CASES[name]
    return simulate(positions, edges), scale, list(between), {k: np.array(v, dtype=float) for k, v in expected.items()}, tol


def noisy_recovery_case(n=30, seed=3):
    """The noisy graph of the pipeline test: n cameras, every camera joined to the next four, directions perturbed by 1e-2,
    10 % of the edges replaced by random directions.  Returns (positions, measurements [(a, b, z, kind, params)])."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-10, 10, (n, 3))
    meas = []
    for i in range(n):
        for k in (1, 2, 3, 4):
            j = (i + k) % n
            a, b = (i, j) if i < j else (j, i)
            z = unit(unit(pos[b] - pos[a]) + rng.normal(0, 1e-2, 3))
            if rng.uniform() < 0.10:
                z = unit(rng.normal(0, 1, 3))
            meas.append((a, b, z, A.NOISE_ISOTROPIC, [0.01]))
    return pos, meas


_pipeline_cache = {}


def noisy_pipeline_case():
    """noisy_recovery_case with the restated MFAS filter, computed once: dict(pos, meas, dirs (what Unit3 makes of the
    measured directions: the filter's input), proj (the projection directions: every
    third measurement, at most 48), want_mean, margins, threshold_gap = the smallest distance of a restated mean from 0.1)."""
    if not _pipeline_cache:
        pos, meas = noisy_recovery_case()
        # the directions as Unit3's constructor leaves them (it normalises once more: the last bit may move)
        k1, k2, ed = [m[0] for m in meas], [m[1] for m in meas], np.array([unit(m[2]) for m in meas])
        proj = ed[::3][:48]
        want_mean, heur, root = np.zeros(len(meas)), math.inf, math.inf
        for d in proj:
            w = T.mfas_edge_weights(k1, k2, ed, d)
            order, m = T.mfas_ordering(w)
            heur, root = min(heur, m["heuristic"]), min(root, m["root"])
            ow = T.mfas_weights_for_ordering(w, order)
            want_mean += np.array([ow[p] for p in zip(k1, k2)]) / len(proj)
        _pipeline_cache.update(pos=pos, meas=meas, dirs=ed, proj=proj, want_mean=want_mean, margins=dict(heuristic=heur, root=root),
                               threshold_gap=float(np.min(np.abs(want_mean - 0.1))))
    return _pipeline_cache
