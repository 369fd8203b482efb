"""The back-substitution's launch plan (upload.hip: plan_backsolve; handle.h: BsLaunch) read from the library through the
host-only hook gsxtest_backsolve_plan, on handles without a device.

The level plan — what the wildfire pass and GSX_BS_TREE_OFF walk — against tests/_wildfire_cases.py::kernel_of, the
statement of the same dispatch that test_gpu_wildfire_classes.py, test_host_wildfire_cases.py and
test_gpu_backsolve_packed.py name their kernels with: every case, both amalgamation settings, with and without
GSX_BS_LEAF_PACK=0, clique by clique.  What the plan does not decide is taken from where it is decided: small / small2 is
launch_backsolve_small's choice by the launch's largest F (at most 32: small), and the wave form's tail loop (leaf_tail) is
taken by a leaf clique of more than 128 separator rows.

The default plan — the upper levels top-down, the one tree launch, the leaves — on the smallest deep tree of
tests/_linear_cases.py (no upper front at all) and on a wildfire case with blocked fronts, tree fronts and leaves."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _linear_cases as L
from tests import _wildfire_cases as W
from tests._switches import switches

BIG, SMALL, GENERIC, LEAF, TREE = range(5)       # handle.h: BsKind
AMALGAMATIONS = {"reference": W.AMALGAMATION, "relaxed": W.RELAXED}


def _big_lds():
    from gtsam_petercdev_amd import _lib
    f = _lib.load().gsxtest_backsolve_big_lds
    f.restype = C.c_longlong
    f.argtypes = [C.c_int, C.c_int, C.c_int]
    return f


def _plans(arr, ordering, amalgamation, packed=True):
    """(parent, fronts, classes, level plan records (front, kind, threads, max_F, launch), default plan records (kind,
    level, count, threads, max_n)) of a host-only handle; packed=False: made under GSX_BS_LEAF_PACK=0 (read when a handle
    is created)."""
    from gtsam_petercdev_amd import _lib
    with switches(GSX_BS_LEAF_PACK=None if packed else "0"):
        hb = _lib.ProductBackend(arr, host_only=True)
    hb.set_amalgamation(*amalgamation)
    hb.set_ordering(ordering)
    parent, fronts = hb.get_tree()
    cls = [int(c) for c in hb.front_classes()]
    hook = _lib.load().gsxtest_backsolve_plan
    hook.restype = C.c_int
    hook.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int]
    out = []
    for which in (0, 1):
        n = hook(hb._h, which, None, 0)
        assert n >= 0
        recs = np.zeros((max(n, 1), 5), np.int32)
        assert hook(hb._h, which, recs.ctypes.data_as(C.POINTER(C.c_int)), n) == n
        out.append([tuple(int(x) for x in r) for r in recs[:n]])
    hb.close()
    return [int(p) for p in parent], [(list(f), list(s)) for f, s in fronts], cls, out[0], out[1]


@functools.lru_cache(maxsize=None)
def _level_names(name, amalgamation, packed):
    """(the plan's kernel name per clique, kernel_of's, the plan's cliques in launch order with their levels)."""
    case = W.build(name)
    dims = [int(d) for d in case.arr.var_dims]
    parent, fronts, cls, level_plan, _ = _plans(case.arr, case.arr.var_keys[case.ordering], AMALGAMATIONS[amalgamation], packed)
    assert sorted(r[0] for r in level_plan) == list(range(len(fronts))), "every front in exactly one launch"
    shp = W.clique_shapes(fronts, dims)
    lvl = W.levels_of(parent)
    # the combined launch: a generic one that holds fronts of both classes
    classes_of = {}
    for f, kind, threads, max_F, launch in level_plan:
        classes_of.setdefault(launch, set()).add(cls[f] & 3)
    got = [None] * len(fronts)
    for f, kind, threads, max_F, launch in level_plan:
        if kind == BIG:
            got[f] = "big"
        elif kind == SMALL:
            got[f] = "small" if max_F <= 32 else "small2"
        elif kind == GENERIC:
            got[f] = "combined1024" if classes_of[launch] == {1, 2} else {64: "generic64", 256: "generic256", 1024: "generic1024"}[threads]
            assert got[f] != "combined1024" or threads == 1024
        else:
            assert kind == LEAF and cls[f] & 3 == 0
            got[f] = {16: "leaf16", 32: "leaf32", 64: "leaf64" if shp[f][1] <= 128 else "leaf_tail"}[threads]
    want = W.kernel_of(parent, fronts, cls, dims, _big_lds(), packed=packed)
    return got, want, [(f, lvl[f]) for f, *_ in level_plan]


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "GSX_BS_LEAF_PACK=0"])
@pytest.mark.parametrize("amalgamation", list(AMALGAMATIONS))
@pytest.mark.parametrize("name", list(W.CASES))
def test_level_plan_is_kernel_of(name, amalgamation, packed):
    got, want, order = _level_names(name, amalgamation, packed)
    assert got == want, [(f, g, w) for f, (g, w) in enumerate(zip(got, want)) if g != w]
    # top-down, and inside a level: blocked-own, small-own, the generic launches (blocked before LDS-class), leaves
    rank = {"big": 0, "small": 1, "small2": 1, "combined1024": 2, "generic1024": 2, "generic256": 3, "generic64": 3}
    keys = [(-l, rank.get(got[f], 4)) for f, l in order]
    assert keys == sorted(keys), keys
    if not packed:
        assert not {"leaf16", "leaf32"} & set(got)


def test_the_cases_reach_every_name_a_tree_can():
    """generic64 needs LDS-class cliques of at most 48 rows that backsolve_small_fits refuses, and it refuses only F > 64:
    no tree has it (tests/_wildfire_cases.py).  Every other name occurs at the reference's amalgamation already."""
    seen = set()
    for name in W.CASES:
        seen.update(_level_names(name, "reference", True)[0])
    assert seen == W.BRANCHES, seen ^ W.BRANCHES


def _default_plan_facts(arr, ordering, amalgamation):
    parent, fronts, cls, _, plan = _plans(arr, ordering, amalgamation)
    n_tree = sum(1 for c in cls if c & 4)
    n_leaf = sum(1 for c in cls if c & 3 == 0)
    upper = [r for r in plan if r[0] in (BIG, SMALL, GENERIC)]
    assert plan[:len(upper)] == upper, "the upper levels come first"
    assert [r[1] for r in upper] == sorted((r[1] for r in upper), reverse=True), "top-down"
    assert sum(r[2] for r in upper) == len(fronts) - n_tree - n_leaf
    rest = plan[len(upper):]
    assert [r[0] for r in rest] == ([TREE] if n_tree else []) + ([LEAF] if n_leaf else [])
    if n_tree:
        assert rest[0][2] == n_tree
    if n_leaf:
        assert rest[-1][1] == 0 and rest[-1][2] == n_leaf
    return upper, n_tree, n_leaf, cls


def test_default_plan_of_a_tree_without_upper_fronts():
    arr, ordering = L.DEEP_DENSE["broom65"][0]()
    upper, n_tree, n_leaf, _ = _default_plan_facts(arr, arr.var_keys[ordering], L.DEEP_AMALGAMATION)
    assert upper == [] and n_tree == 130 and n_leaf == 65


def test_default_plan_upper_levels_then_tree_then_leaves():
    """combined1024: the (193, 5) arms are blocked fronts, so they, their middle cliques and the root are upper fronts; the
    (65, 5) arms are tree fronts; the padding cliques are leaves.  The upper schedule has no combined launch: the bottom
    level's blocked fronts go to the generic kernel alone."""
    case = W.build("combined1024")
    upper, n_tree, n_leaf, cls = _default_plan_facts(case.arr, case.arr.var_keys[case.ordering], W.AMALGAMATION)
    assert n_tree > 0 and n_leaf > 0 and len(upper) >= 2
    assert sum(1 for c in cls if c & 3 == 2) == 2
    blocked = [r for r in upper if r[0] == GENERIC and r[3] == 1024]
    assert len(blocked) == 1 and blocked[0][2] == 2 and blocked[0][4] == 193 + 5 + 1
