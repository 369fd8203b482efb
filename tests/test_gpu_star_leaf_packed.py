"""Star leaves eliminated several to a wave (kernels.hip: front_star_leaf_packed_kernel; the host's rule:
star_leaf_pack_class) against the wave form, which a handle created under GSX_STAR_LEAF_PACK=0 keeps for every clique, and
against the two-step path of a handle created under GSX_FUSED_STAR=0: bit for bit.

The three handles see the same arrays and the same ordering, so every comparison is np.array_equal (or ==), never a
tolerance: the solution at lambda I and with diagonal damping, lm_trial's three errors, the conditionals of the landmark
cliques.  The problems are hand-built stars over a ring of cameras (datasets.synth_bal's cameras and points, the
observation lists made here): every landmark's factor count is chosen, so the classes of a launch are known —
lanes_of (test_host_star_leaf_partition.py) restates the rule, and the library's own counts per launch group
(gsxtest_star_leaf_classes) are held to it.  Landmark 0 carries the prior of bal_arrays: it is no star variable.
"""
import ctypes as C

import numpy as np
import pytest

from gtsam_petercdev_amd import _abi as A
from gtsam_petercdev_amd import datasets

from ._switches import switches
from .test_gpu_fused_star import _huber, _landmark_cliques, _sfm_pairs
from .test_host_star_leaf_partition import lanes_of

pytestmark = pytest.mark.gpu

# 1 ... 65 factors mixed in one launch: the 16-lane class takes 1 2 3 4 5 7 3 2 6 1 4 2 3 in this order (the groups of its
# first wave take 1, 2, 2 and 3 passes over their partner rows), the 32-lane class 9 12 8 14 10, the wave form the others
MIXED = [2, 1, 2, 3, 4, 15, 16, 17, 31, 32, 33, 64, 65, 5, 9, 7, 12, 3, 2, 6, 8, 1, 4, 14, 10, 2, 3]
CASES = {
    # name: (cameras, factors per landmark, expected cliques (16 lanes, 32 lanes, wave) without landmark 0)
    "mixed": (66, MIXED, (13, 5, 8)),
    "counts_1_3_5": (66, [2, 3, 8, 10, 14, 15, 16, 20, 33, 40], (1, 3, 5)),
    "counts_5_1_0": (66, [2, 1, 2, 3, 4, 5, 9], (5, 1, 0)),          # no clique in the wave form
    "counts_3_0_1": (66, [2, 17, 2, 6, 7], (3, 0, 1)),               # no clique of 32 lanes
}


@pytest.fixture(scope="module")
def gpu():
    from gtsam_petercdev_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the HIP path has no fallback"
    return _lib


def _star_sfm(n_cams, nfs, seed=5, behind=(), late=()):
    """SfmData of len(nfs) landmarks, landmark j seen by nfs[j] consecutive cameras of the ring (the windows tile the ring
    one after the other), and one more landmark seen by EVERY camera: it makes the cameras one clique, which it joins, so
    that no other landmark's separator is a whole clique and every other landmark stays a leaf clique of its own.
    behind: landmarks put behind their cameras in the initial estimate (every factor of theirs fails the cheirality
    test).  late: landmarks whose second observation is moved to the end of the factor list, so that
    their factors are not evenly spaced in [A b]."""
    nfs = np.asarray(list(nfs) + [n_cams], np.int64)
    truth, init = datasets.synth_bal(n_cams, nfs.size, 2 * nfs.size, seed)
    assert nfs.max() <= n_cams
    pt_idx = np.repeat(np.arange(nfs.size), nfs)
    start = np.concatenate([[0], np.cumsum(nfs)[:-1]])
    cam_idx = np.arange(pt_idx.size) % n_cams          # landmark j: cameras start[j] ... start[j] + nfs[j] - 1 of the ring
    assert nfs.sum() >= n_cams
    c = truth.cameras[cam_idx]
    R = c[:, :9].reshape(-1, 3, 3)
    q = np.einsum("nji,nj->ni", R, truth.points[pt_idx] - c[:, 9:12])
    assert np.all(q[:, 2] > 0)
    u, v = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
    r = u * u + v * v
    g = 1 + (c[:, 13] + c[:, 14] * r) * r
    uv = np.stack([c[:, 12] * g * u, c[:, 12] * g * v], axis=1) + np.random.default_rng(seed + 1).normal(0, 0.5, (q.shape[0], 2))
    pts0 = init.points.copy()
    for j in behind:
        pts0[j] = 10.0 * init.cameras[cam_idx[start[j]], 9:12]   # (behind every camera within 80 degrees of the first)
    order = np.arange(pt_idx.size)
    for j in late:
        assert nfs[j] >= 3
        k = start[j] + 1
        order = np.concatenate([order[order != k], [k]])
    return datasets.SfmData(init.cameras, pts0, cam_idx[order], pt_idx[order], uv[order])


def _arrays(name, **kw):
    n_cams, nfs, _ = CASES[name]
    return datasets.bal_arrays(_star_sfm(n_cams, nfs, **kw), priors=True)


def _under(gpu, arr, var, ordering, reference_tree=False):
    """A handle made with `var` set to 0 (None: a default handle) under the ordering; reference_tree: without the relaxed
    amalgamation, which on a bundle of a few landmarks folds some of them into the cliques of their cameras."""
    with switches(**({var: "0"} if var else {})):
        be = gpu.product_backend(arr)
    if reference_tree:
        be.set_amalgamation(0.0, 128)
    be.set_ordering(ordering)
    return be


def _handles(gpu, arr, ordering=None, reference_tree=False):
    """(default handle, wave form only, two-step path) under one ordering (the switches are read when a handle is created)."""
    if ordering is None:
        probe = gpu.product_backend(arr)
        ordering = probe.compute_ordering(A.ORDER_SCHUR)
        probe.close()
    return tuple(_under(gpu, arr, var, ordering, reference_tree) for var in (None, "GSX_STAR_LEAF_PACK", "GSX_FUSED_STAR"))


def _classes(gpu, be):
    """Per launch group (cliques of 16 lanes, of 32 lanes, of a wave, other leaves); [] when the handle does not fuse."""
    hook = gpu.load().gsxtest_star_leaf_classes
    hook.restype = C.c_int
    hook.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int]
    n = hook(be._h, None, 0)
    out = np.zeros((max(n, 1), 4), np.int32)
    assert hook(be._h, out.ctypes.data_as(C.POINTER(C.c_int)), n) == n
    return [tuple(int(x) for x in r) for r in out[:n]]


def _solve(be, lam, diag):
    try:
        return be.solve(lam, diag)
    except A.IndeterminantLinearSystemException as e:
        return (e.key, str(e))


def _same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and np.array_equal(a, b)
    return a == b


def _check(gpu, arr, expect=None, n_other=1):
    hs = _handles(gpu, arr)
    pk, wv, two = hs
    cl = _classes(gpu, pk)
    print("star leaf classes per launch group (16, 32, wave, other):", cl, "wave form only:", _classes(gpu, wv))
    if expect is not None:
        assert len(cl) == 1                                  # ONE launch holds the mix
        assert tuple(sum(g[i] for g in cl) for i in range(3)) == tuple(expect)
        assert sum(g[3] for g in cl) == n_other
        assert tuple(sum(g[i] for g in _classes(gpu, wv)) for i in range(3)) == (0, 0, sum(expect))
    assert _classes(gpu, two) == []
    for be in hs:
        be.linearize()
    for other in (wv, two):
        assert np.array_equal(pk.jacobians(), other.jacobians())
    cliques = _landmark_cliques(pk, arr, 12)
    for lam, diag in ((1.0, False), (1e-2, False), (1e-2, True)):
        ref = _solve(pk, lam, diag)
        if lam == 1.0:
            assert isinstance(ref, np.ndarray)
        for other in (wv, two):
            assert _same(ref, _solve(other, lam, diag)), (lam, diag)
            if isinstance(ref, np.ndarray):
                assert pk.linear_error() == other.linear_error()
                for c in cliques:
                    assert np.array_equal(pk.conditional(c), other.conditional(c)), (lam, diag, c)
    for args, kw in (((True, 1.0), {}), ((False, 1e-1), {}), ((False, 1e-1), dict(diagonal_damping=True))):
        t = pk.lm_trial(*args, **kw)
        assert t == wv.lm_trial(*args, **kw) and t == two.lm_trial(*args, **kw), (args, kw)
    return hs


@pytest.mark.parametrize("name", list(CASES))
def test_classes_bitwise(gpu, name):
    nfs, expect = CASES[name][1], CASES[name][2]
    assert expect == tuple(sum(1 for n in nfs[1:] if lanes_of(n, 9) == g) for g in (16, 32, 64))
    _check(gpu, _arrays(name), expect)


def test_uneven_factor_spacing(gpu):
    # landmarks of the 16-lane class (4 factors), the 32-lane class (9) and the wave form (17) read through their term records
    _check(gpu, _arrays("mixed", late=(4, 14, 7)), CASES["mixed"][2])


def test_robust_noise(gpu):
    _check(gpu, _huber(_arrays("mixed")), CASES["mixed"][2])


def test_repeated_camera_landmark_pair(gpu):
    # the pair's landmark (3 factors, of the 16-lane class) is no star variable: its clique leaves the class
    arr = _arrays("mixed")
    lm = arr.meta["pt_vars"][3]
    c, _, f0 = next(p for p in _sfm_pairs(arr) if p[1] == lm)
    meas = arr.meas[arr.f_meas_ptr[f0]:arr.f_meas_ptr[f0 + 1]] + 0.25
    arr = arr.with_factor(A.F_SFM, [c, lm], 2, meas, int(arr.f_noise_kind[f0]), arr.noise[arr.f_noise_ptr[f0]:arr.f_noise_ptr[f0 + 1]])
    n16, n32, n64 = CASES["mixed"][2]
    _check(gpu, arr, (n16 - 1, n32, n64), n_other=2)


def test_cheirality_failure(gpu):
    # landmark 3 (3 factors) behind its cameras: its factors are zeroed, the damped clique is eliminated as before
    arr = _arrays("mixed", behind=(3,))
    pk, wv, two = _check(gpu, arr, CASES["mixed"][2])
    assert pk.stats()["n_cheirality"] == 3 == wv.stats()["n_cheirality"] == two.stats()["n_cheirality"]


def _fail_count(gpu, be):
    hook = gpu.load().gsxtest_last_fail_count
    hook.restype = C.c_int
    hook.argtypes = [C.c_void_p]
    return hook(be._h)


# name: (cameras, factors per landmark — ascending, so that any order by height keeps them in turn —, the landmark made
# indefinite, the class it sits in).  Six records of 16 lanes: the bad one is the third from one end and the fourth from
# the other — group 2 or 3 of the first wave, lanes 32 or 48 up, healthy groups before and after it.  Five records of 32
# lanes: the second or the fourth — the upper half of its wave, a healthy clique in the lower half.
INDEFINITE = {
    "16_lanes": (30, [2, 2, 3, 4, 5, 6, 7], 3, 0),
    "32_lanes": (40, [5, 8, 9, 10, 11, 12, 3, 4, 5, 6, 7], 2, 1),   # (and a wave and a half of 16-lane cliques beside them)
}


@pytest.mark.parametrize("name", list(INDEFINITE))
def test_one_indefinite_landmark_in_a_shared_wave(gpu, name):
    """Without damping a landmark whose every factor is zeroed (it lies behind its cameras) has a zero own block: its first
    pivot fails.  The landmark sits in a group that does not begin at lane 0 of its wave, with healthy landmarks in the
    wave's other groups, and it is not the lowest front: a report taken from the wave's lane 0 would be missing, and a
    healthy neighbour reporting too would name a lower front or raise the count of failed fronts.  Every handle names the
    landmark's key, and the shared waves count as many failed fronts as the two-step path does.

    What this does NOT see is the neighbours' panels after the failed factorization: they cannot be read back (no
    conditional without a valid factorization).  The agreement checked afterwards is that of the next, damped,
    factorization, which rewrites every panel."""
    n_cams, nfs, bad, cls = INDEFINITE[name]
    mine = [n for n in nfs[1:] if lanes_of(n, 9) == (16, 32)[cls]]
    assert nfs[bad] in mine and mine == sorted(set(mine)) and not any(lanes_of(n, 9) == 64 for n in nfs[1:])
    arr = datasets.bal_arrays(_star_sfm(n_cams, nfs, behind=(bad,)), priors=True)
    hs = _handles(gpu, arr, reference_tree=True)
    cl = _classes(gpu, hs[0])
    print("star leaf classes per launch group:", cl)
    assert len(cl) == 1 and cl[0][cls] == len(mine) and cl[0][1 - cls] == len(nfs) - 1 - len(mine) and cl[0][2] == 0
    pt_vars = [int(v) for v in arr.meta["pt_vars"]]
    _, fronts = hs[0].get_tree()
    front_of = {f[0]: c for c, (f, _) in enumerate(fronts) if len(f) == 1}
    star = [front_of[pt_vars[j]] for j in range(1, len(nfs))]
    assert min(star) < front_of[pt_vars[bad]] < max(star)                    # not the lowest front, nor the last
    assert max(star) < min(c for c, (f, _) in enumerate(fronts) if any(v not in pt_vars for v in f))
    for be in hs:
        be.linearize()
        assert be.stats()["n_cheirality"] == nfs[bad]
    res = [_solve(be, 0.0, False) for be in hs]
    fails = [_fail_count(gpu, be) for be in hs]
    print("failed fronts (shared waves, wave form, two-step):", fails)
    assert not isinstance(res[0], np.ndarray)
    assert res[0][0] == int(arr.var_keys[pt_vars[bad]])
    assert res[0] == res[1] == res[2]
    assert fails[0] == fails[1] == fails[2] >= 1
    d = [be.solve(1.0, False) for be in hs]
    assert np.array_equal(d[0], d[1]) and np.array_equal(d[0], d[2])
    for c in _landmark_cliques(hs[0], arr, 13):
        assert np.array_equal(hs[0].conditional(c), hs[1].conditional(c)) and np.array_equal(hs[0].conditional(c), hs[2].conditional(c))


def test_bal49_schur(gpu):
    arr = datasets.synth_bal_arrays(49, 7776, 31843, seed=42, long_range=0.3)
    pk, wv, two = _check(gpu, arr)
    cl = _classes(gpu, pk)
    assert sum(g[0] + g[1] for g in cl) > 0.9 * 7776          # nearly every landmark shares its wave
    p = A.lm_params_legacy()
    p.max_iterations = 3
    rs = [be.lm_optimize(p) for be in (pk, wv, two)]
    for other in rs[1:]:
        for k in rs[0]:
            if isinstance(rs[0][k], np.ndarray):
                assert np.array_equal(rs[0][k], other[k]), k
            else:
                assert rs[0][k] == other[k], k
    assert np.array_equal(pk.get_values(), wv.get_values()) and np.array_equal(pk.get_values(), two.get_values())
