"""The schedule switches (README; csrc/gsx_internal.h: ScheduleOptions) are read once, when a handle is created, and stay
with it: a handle made under a switch keeps the switched plan through every later gsx_set_ordering although the environment
has been restored, and a handle made afterwards has the default plan.  Host-only handles, through the observables the suite
already uses: stats(), gsx_get_gather_plan, gsx_get_hessian_groups, gsxtest_backsolve_plan.

The defaults: with no switch set, the plans of one case of each kind are what they were before the switches moved into one
struct (figures recorded from the commit before)."""
import ctypes as C
from collections import Counter

import pytest

from gtsam_petercdev_amd import _abi as A
from gtsam_petercdev_amd import _lib
from tests import _assembly_cases as AC
from tests import _gather_cases as G
from tests import _linear_cases as L
from tests import _wildfire_cases as W
from tests._switches import switches

SWITCHES = ("GSX_TREE_TIERS", "GSX_MEDIUM", "GSX_SIDE_OFF", "GSX_SIDE_MIN", "GSX_ND_LEAF", "GSX_SMALL_THREADS_SHIFT",
            "GSX_H_TILE_OFF", "GSX_FUSED_STAR", "GSX_STAR_LEAF_PACK", "GSX_BS_LEAF_PACK", "GSX_BS_TREE_OFF", "GSX_LINERR_DIRECT")
LEAF = 3   # handle.h: BsKind


def backsolve_plan(hb, which):
    """gsxtest_backsolve_plan: which = 0 the level plan (front, kind, threads, max_F, launch), 1 the default plan (kind,
    level, count, threads, max_n)."""
    hook = _lib.load().gsxtest_backsolve_plan
    hook.restype = C.c_int
    hook.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int]
    n = hook(hb._h, which, None, 0)
    assert n >= 0
    recs = (C.c_int * (5 * max(n, 1)))()
    assert hook(hb._h, which, recs, n) == n
    return [tuple(recs[5 * i:5 * i + 5]) for i in range(n)]


def _tree():
    arr = L.tree_arrays("pose2")
    return arr, A.ORDER_ND, L.TREE_AMALGAMATION


def _medium():
    arr, ordering = L.DEEP_DENSE["medium_chain"][0]()
    return arr, ordering, L.DEEP_AMALGAMATION


def _side():
    case = G.build("stacked_blocked")
    assert case.env == {"GSX_SIDE_MIN": "1"}
    return case.arr, case.arr.var_keys[case.ordering], G.AMALGAMATION


def _tile():
    case = AC.CASES["tile_group_of_4"]
    return case.arrays("int"), case.ordering, None


def _packed():
    case = W.build("pack16_wave6")
    return case.arr, case.arr.var_keys[case.ordering], W.AMALGAMATION


# switch -> (environment, case, observable of a handle with an ordering, its value is the switched one)
KINDS = {
    "GSX_TREE_TIERS=0": ({"GSX_TREE_TIERS": "0"}, _tree, lambda hb: hb.stats()["n_tree_fronts"], lambda n: n == 0),
    "GSX_MEDIUM=1": ({"GSX_MEDIUM": "1"}, _medium, lambda hb: hb.stats()["n_medium_fronts"], lambda n: n > 0),
    "GSX_SIDE_MIN=1": ({"GSX_SIDE_MIN": "1"}, _side,
                       lambda hb: sum(1 for s in hb.gather_plan()["segments"] if s["group"] == G.SIDE), lambda n: n > 0),
    "GSX_H_TILE_OFF": ({"GSX_H_TILE_OFF": "1"}, _tile,
                       lambda hb: int((hb.hessian_groups()["class"] == A.H_TILE).sum()), lambda n: n == 0),
    "GSX_BS_LEAF_PACK=0": ({"GSX_BS_LEAF_PACK": "0"}, _packed,
                           lambda hb: sorted({r[2] for r in backsolve_plan(hb, 0) if r[1] == LEAF} & {16, 32}),
                           lambda t: t == []),
}


def _handle(arr, amalgamation):
    hb = _lib.ProductBackend(arr, host_only=True)
    if amalgamation is not None:
        hb.set_amalgamation(*amalgamation)
    return hb


@pytest.mark.parametrize("kind", list(KINDS))
def test_switch_is_read_when_the_handle_is_created(kind):
    env, case, observe, switched = KINDS[kind]
    arr, ordering, amalgamation = case()
    with switches(**{k: None for k in SWITCHES}):
        with switches(**env):
            a = _handle(arr, amalgamation)
        b = _handle(arr, amalgamation)          # after the environment was put back
        if isinstance(ordering, int):
            ordering = b.compute_ordering(ordering)
        a.set_ordering(ordering)
        b.set_ordering(ordering)
        first, default = observe(a), observe(b)
        assert switched(first) and not switched(default), (kind, first, default)
        a.set_ordering(ordering)                # a second analysis, long after creation: the handle's own options again
        assert observe(a) == first, (kind, first, observe(a))
        with switches(**env):                   # ... and a switch set later does not reach a handle that exists
            b.set_ordering(ordering)
        assert observe(b) == default, (kind, default, observe(b))
    a.close()
    b.close()


def _facts(kind):
    arr, ordering, amalgamation = KINDS[kind][1]()
    hb = _handle(arr, amalgamation)
    if isinstance(ordering, int):
        ordering = hb.compute_ordering(ordering)
    hb.set_ordering(ordering)
    st = hb.stats()
    out = {
        "fronts": (st["n_tree_fronts"], st["n_medium_fronts"], st["n_big_fronts"]),
        "classes": sorted(Counter(int(c) for c in hb.front_classes()).items()),
        "gather_groups": sorted(Counter(s["group"] for s in hb.gather_plan()["segments"]).items()),
        "hessian_classes": sorted(Counter(int(c) for c in hb.hessian_groups()["class"]).items()),
        "level_plan": sorted(Counter(r[1:3] for r in backsolve_plan(hb, 0)).items()),   # (kind, threads) -> cliques
        "default_plan": backsolve_plan(hb, 1),
    }
    hb.close()
    return out


# _facts() of the commit before ScheduleOptions, no switch set
DEFAULTS = {
    "GSX_BS_LEAF_PACK=0": {"classes": [(0, 17), (5, 10)],
                           "default_plan": [(4, 0, 10, 0, 68), (3, 0, 17, 0, 0)],
                           "fronts": (10, 0, 0),
                           "gather_groups": [],
                           "hessian_classes": [(0, 82), (1, 5), (2, 1)],
                           "level_plan": [((1, 0), 10), ((3, 16), 14), ((3, 64), 3)]},
    "GSX_H_TILE_OFF": {"classes": [(0, 1)],
                       "default_plan": [(3, 0, 1, 0, 0)],
                       "fronts": (0, 0, 0),
                       "gather_groups": [],
                       "hessian_classes": [(0, 4), (1, 1)],
                       "level_plan": [((3, 64), 1)]},
    "GSX_MEDIUM=1": {"classes": [(1, 2), (2, 8)],
                     "default_plan": [(1, 9, 1, 0, 65), (1, 8, 1, 0, 105), (0, 7, 1, 0, 145), (0, 6, 1, 0, 145),
                                      (0, 5, 1, 0, 145), (0, 4, 1, 0, 145), (0, 3, 1, 0, 145), (0, 2, 1, 0, 145),
                                      (0, 1, 1, 0, 145), (0, 0, 1, 0, 145)],
                     "fronts": (0, 0, 8),
                     "gather_groups": [(1, 6), (2, 6), (3, 6), (4, 6), (5, 6), (6, 6), (7, 6)],
                     "hessian_classes": [(1, 4), (3, 8)],
                     "level_plan": [((0, 0), 8), ((1, 0), 2)]},
    "GSX_SIDE_MIN=1": {"classes": [(2, 2), (8, 135)],
                       "default_plan": [(0, 1, 1, 0, 151), (0, 0, 1, 0, 181), (3, 0, 135, 0, 0)],
                       "fronts": (0, 0, 2),
                       "gather_groups": [(0, 29), (1, 6)],
                       "hessian_classes": [(1, 155)],
                       "level_plan": [((0, 0), 2), ((3, 16), 135)]},
    "GSX_TREE_TIERS=0": {"classes": [(0, 31), (5, 30)],
                         "default_plan": [(4, 0, 30, 0, 118), (3, 0, 31, 0, 0)],
                         "fronts": (30, 0, 0),
                         "gather_groups": [],
                         "hessian_classes": [(0, 400)],
                         "level_plan": [((1, 0), 24), ((2, 256), 6), ((3, 64), 31)]},
}


@pytest.mark.parametrize("kind", list(KINDS))
def test_defaults_are_the_plans_of_an_empty_environment(kind):
    with switches(**{k: None for k in SWITCHES}):
        got = _facts(kind)
    assert got == DEFAULTS[kind], got
