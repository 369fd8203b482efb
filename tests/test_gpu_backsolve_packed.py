"""The leaf back-substitution with several cliques to a wave (kernels.hip: backsolve_leaf_packed; 16 or 32 lanes a clique
when the separator has at most 64 / 128 rows and the F x F triangle fits the group) against the wave-per-clique form,
which a handle created under GSX_BS_LEAF_PACK=0 keeps: word for word, never a tolerance.

The bundle-adjustment case is synth_bal_arrays' own recipe (synth_bal, then bal_arrays with priors) with each track cut to a
chosen length, so that landmarks with 1, 2, 3, 4, 7, 8, 14 and 15 observations occur: separators of 9 ... 135 rows, that is
the 16-lane class up to 63 rows (one to four register rows a lane in use), the 32-lane class at 72 and 126 rows (three
and four), and the wave form with its tail loop past 128 rows.  A landmark
seen once has a singular block without damping, so that case runs at lambda > 0 only; the runs at lambda = 0 (the
neighbouring-lambda sequence, the wildfire pass) use the same problem with those landmarks seen twice.  The class of every
leaf clique is restated here from gsx_get_tree's sizes; each class must occur, with a count that fills no whole number of
workgroups (16, 8 and 4 cliques).  Pose2 graphs reach backsolve_leaf_kernel<4> (F = 3, all packed) and <8> (F = 3 packed
beside F = 6 a wave each: 36 triangle lanes), a Pose3 chain <8> with F = 6 only — the wave form within its 128 register
rows.

The packed results are also held to the float64 backward-error bounds of tests/test_gpu_linear_bounds.py (its helpers,
its neighbouring-lambda sequence on one handle), and a wildfire pass in which whole cliques are skipped inside shared
waves must leave the same words as the wave-per-clique handle's.
"""
from collections import Counter

import numpy as np
import pytest

from gtsam_petercdev_amd import _abi as A
from gtsam_petercdev_amd import datasets
from tests._switches import switches
from tests.test_gpu_linear_bounds import _device_case, _judge

pytestmark = pytest.mark.gpu

OBSERVATIONS = {1: 23, 2: 46, 3: 38, 4: 42, 7: 28, 8: 18, 14: 12, 15: 9}     # track length -> landmarks
L2 = 0.1 * (1 + 1e-8)
NEIGHBOURS = [(0.1, True), (L2, True), (0.0, False), (L2, True)]            # test_neighbouring_lambdas_on_one_arena's
DAMPED = [(0.1, True), (L2, True), (1.0, False), (L2, True)]
_ARRAYS = {}


@pytest.fixture(scope="module")
def gpu():
    from gtsam_petercdev_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the HIP path has no fallback"
    return _lib


def _bal(single):
    lengths = np.concatenate([np.full(n, k if (single or k > 1) else 2) for k, n in OBSERVATIONS.items()])
    np.random.default_rng(3).shuffle(lengths)
    _, init = datasets.synth_bal(16, lengths.size, 16 * lengths.size - 1, seed=5)
    per_track = np.bincount(init.pt_idx, minlength=lengths.size)
    assert np.all(per_track >= lengths)
    within = np.arange(init.pt_idx.size) - np.repeat(np.cumsum(per_track) - per_track, per_track)
    keep = within < lengths[init.pt_idx]
    sfm = datasets.SfmData(init.cameras, init.points, init.cam_idx[keep], init.pt_idx[keep], init.uv[keep])
    return datasets.bal_arrays(sfm, priors=True)


#        arrays, ordering, amalgamation, lambdas, widest F of a leaf clique, classes that must occur
CASES = {
    "bal_1_to_15": (lambda: _bal(True), A.ORDER_SCHUR, (0.0, 128), DAMPED, 3, {16, 32, "tail"}),
    "bal_2_to_15": (lambda: _bal(False), A.ORDER_SCHUR, (0.0, 128), NEIGHBOURS, 3, {16, 32, "tail"}),
    "pose2_leaf4": (lambda: datasets.synth_manhattan_pose2(400, seed=3), A.ORDER_ND, (0.0, 128), NEIGHBOURS, 3, {16}),
    "pose2_leaf8": (lambda: datasets.synth_manhattan_pose2(400, seed=3), A.ORDER_ND, (0.5, 6), NEIGHBOURS, 6, {16, 64}),
    "pose3_leaf8": (lambda: datasets.synth_manhattan_pose3(300, seed=4), A.ORDER_ND, (0.0, 128), NEIGHBOURS, 6, {64}),
}


def _arrays(name):
    if name not in _ARRAYS:
        _ARRAYS[name] = CASES[name][0]()
    return _ARRAYS[name]


def _pair(gpu, arr, kind, amalgamation):
    """(packed handle, wave-per-clique handle) under one ordering (the switch is read when a handle is created)."""
    packed = gpu.product_backend(arr)
    with switches(GSX_BS_LEAF_PACK="0"):
        plain = gpu.product_backend(arr)
    ordering = packed.compute_ordering(kind)
    for be in (packed, plain):
        be.set_amalgamation(*amalgamation)
        be.set_ordering(ordering)
    return packed, plain


def _leaf_classes(gb, arr):
    """kernels.hip's leaf_pack_class restated over the leaf-kernel cliques (front class 0) of gsx_get_tree."""
    _, fronts = gb.get_tree()
    dims = arr.var_dims
    leaf = [(int(dims[f].sum()), int(dims[s].sum())) for (f, s), c in zip(fronts, gb.front_classes()) if (int(c) & 3) == 0]
    max_f = max(F for F, _ in leaf)

    def lanes(F, sep):
        if max_f <= 8 and sep <= 64 and F * F <= 16:
            return 16
        if max_f <= 8 and sep <= 128 and F * F <= 32:
            return 32
        return 64 if sep <= 128 else "tail"
    return max_f, Counter(lanes(F, sep) for F, sep in leaf), sorted(set(sep for _, sep in leaf))


def _same_words(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("name", list(CASES))
def test_packed_equals_wave_per_clique(gpu, name):
    _, kind, amalgamation, lambdas, widest, wanted = CASES[name]
    arr = _arrays(name)
    packed, plain = _pair(gpu, arr, kind, amalgamation)
    max_f, census, seps = _leaf_classes(packed, arr)
    print(name, "widest leaf F", max_f, "classes", dict(census), "separator rows", seps)
    assert max_f == widest and set(census) == wanted, (max_f, census)
    if name == "bal_1_to_15":
        assert seps == [9, 18, 27, 36, 63, 72, 126, 135], seps
    # no class fills whole workgroups: the last wave of each is partly (16, 32 lanes) or wholly (wave form) idle
    assert census[16] % 16 != 0 or 16 not in wanted
    assert census[32] % 8 != 0 or 32 not in wanted
    assert (census[64] + census["tail"]) % 4 != 0 or not wanted & {64, "tail"}
    for be in (packed, plain):
        be.linearize()
    for lam, diag in lambdas:
        xp, xw = packed.solve(lam, diag), plain.solve(lam, diag)
        assert np.all(np.isfinite(xw)) and np.abs(xw).max() > 0
        assert _same_words(xp, xw), (name, lam, diag, float(np.abs(xp - xw).max()))


@pytest.mark.parametrize("name", list(CASES))
def test_packed_within_the_backward_error_bounds(gpu, name):
    """check_backward's three measures (tests/_ld_linear.py) after every solve of the sequence, on one handle."""
    _, kind, amalgamation, lambdas, _, _ = CASES[name]
    gb, judge, cls = _device_case(gpu, _arrays(name), kind, amalgamation)
    _judge(gb, judge, f"packed leaves {name} classes {sorted(cls)}", lambdas=lambdas, step=False)


def test_wildfire_skips_cliques_inside_shared_waves(gpu):
    """Ring-local bundle adjustment (one moved camera re-eliminates its neighbourhood and the ancestors only): three partial
    passes — a threshold above any change (nothing spreads past the re-eliminated cliques' children), one in the range of
    the changes, and 0 (everything) — each equal between the two handles in every word and in the count."""
    arr = datasets.synth_bal_arrays(160, 3200, 12800, seed=21, long_range=0.0)
    packed, plain = _pair(gpu, arr, A.ORDER_SCHUR_ND, (0.0, 128))
    _, census, _ = _leaf_classes(packed, arr)
    assert census[16] > 100 and census[32] > 20, census
    sd = np.where(arr.var_types == A.VAR_CAMERA, 17, 3)
    off = np.concatenate([[0], np.cumsum(sd)])
    prev = []
    for be in (packed, plain):
        be.linearize()
        prev.append(be.solve(0.0, False))
    assert _same_words(*prev)
    scale = float(np.abs(prev[0]).max())
    rng = np.random.default_rng(8)
    counts = []
    for cam, thr in ((3, 10.0 * scale), (80, 1e-3 * scale), (140, 0.0)):
        v = int(arr.meta["cam_vars"][cam])
        state = arr.values[off[v]:off[v + 1]].copy()
        state[9:12] += 1e-3 * rng.standard_normal(3)          # the camera's position
        out = []
        for be in (packed, plain):
            stats = be.relinearize_partial(arr.var_keys[[v]], state)
            assert stats["n_fronts_reeliminated"] < stats["n_fronts"]
            out.append(be.backsubstitute_wildfire(thr))
        (dp, n_p), (dw, n_w) = out
        print("camera", cam, "threshold", thr, "variables solved", n_p, "of", arr.n_vars)
        assert n_p == n_w and _same_words(dp, dw), (cam, thr, n_p, n_w)
        counts.append(n_p)
    assert 0 < counts[0] < arr.n_vars and counts[2] == arr.n_vars, counts
