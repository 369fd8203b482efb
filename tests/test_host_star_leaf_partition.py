"""The host's partition of a launch group's star leaves into the cliques that take 16 lanes of a wave, 32 lanes, or a wave
(upload.hip: partition_star_leaves; kernels.hip: star_leaf_pack_class), through the host-only hook
gsxtest_star_leaf_partition: no device.  Held to a restatement from the records: every clique in exactly one class, the
order of the list kept inside a class, the class rule; with the switch off (GSX_STAR_LEAF_PACK=0) the list stays as it is.
"""
import ctypes as C

import numpy as np
import pytest

PASSES = 4   # kernels.h: kStarPackPasses


def lanes_of(nf, dB):
    """The narrowest group with a lane per factor whose partner rows (nf dB) take at most PASSES passes of the group."""
    for g in (16, 32):
        if nf <= g and nf * dB <= g * PASSES:
            return g
    return 64


def partition(nf, dB, pack=True):
    from gtsam_petercdev_amd import _lib
    hook = _lib.load().gsxtest_star_leaf_partition
    hook.restype = None
    ip = C.POINTER(C.c_int)
    hook.argtypes = [ip, ip, C.c_int, C.c_int, ip, ip]
    nf, dB = np.ascontiguousarray(nf, np.int32), np.ascontiguousarray(dB, np.int32)
    order, counts = np.full(max(nf.size, 1), -1, np.int32), np.full(3, -1, np.int32)
    hook(nf.ctypes.data_as(ip), dB.ctypes.data_as(ip), nf.size, int(pack), order.ctypes.data_as(ip), counts.ctypes.data_as(ip))
    return [int(i) for i in order[:nf.size]], [int(c) for c in counts]


def _lists():
    rng = np.random.default_rng(11)
    edge = [1, 2, 3, 4, 7, 8, 14, 15, 16, 17, 31, 32, 33, 64, 65, 1023]
    yield "edges_dB9", edge, [9] * len(edge)
    yield "edges_dB6", edge, [6] * len(edge)
    yield "edges_dB3", edge, [3] * len(edge)
    yield "edges_dB1", edge, [1] * len(edge)
    yield "mixed_dB", list(rng.integers(1, 70, 300)), list(rng.choice([1, 2, 3, 6, 7, 9], 300))
    yield "bal_like", list(2 + rng.poisson(2.3, 2000)), [9] * 2000
    yield "only_wave", [40, 65, 100], [9, 9, 9]
    yield "only_16", [1, 2, 3, 4, 5], [9] * 5
    yield "one", [3], [9]
    yield "empty", [], []


@pytest.mark.parametrize("name", [n for n, _, _ in _lists()])
def test_partition_against_the_rule(name):
    nf, dB = next((a, b) for n, a, b in _lists() if n == name)
    order, counts = partition(nf, dB)
    assert sorted(order) == list(range(len(nf)))                      # every clique in exactly one place
    want = [[i for i in range(len(nf)) if lanes_of(int(nf[i]), int(dB[i])) == g] for g in (16, 32, 64)]
    assert counts == [len(w) for w in want]
    assert order == want[0] + want[1] + want[2]                       # the classes in turn, list order inside each


def test_rule_edges():
    # BAL: cameras of 9 — 7 factors are 63 partner rows (4 passes of 16), 8 are 72; 14 are 126 (4 passes of 32), 15 are 135
    assert [lanes_of(n, 9) for n in (1, 7, 8, 14, 15, 32, 33, 64, 65)] == [16, 16, 32, 32, 64, 64, 64, 64, 64]
    # narrow partners: the factor count decides
    assert [lanes_of(n, 1) for n in (16, 17, 32, 33)] == [16, 32, 32, 64]
    _, counts = partition([1, 7, 8, 14, 15, 32, 33, 64, 65], [9] * 9)
    assert counts == [2, 2, 5]
    _, counts = partition([16, 17, 32, 33], [1] * 4)
    assert counts == [1, 2, 1]


def test_switch_off_keeps_the_list():
    nf, dB = [3, 40, 9, 2, 65, 12], [9] * 6
    order, counts = partition(nf, dB, pack=False)
    assert order == list(range(6)) and counts == [0, 0, 6]
