#!/usr/bin/env python3
"""Generates tests/golden/colamd_perm_pose2_400_seed3.npy — the elimination order the REFERENCE's own CCOLAMD
(oracle/_ref/libccolamd_ref.so, compiled by oracle/Makefile from gtsam/3rdparty/CCOLAMD where it lies) returns for
datasets.synth_manhattan_pose2(400, seed=3) through Ordering::Colamd (oracle/oracle.py::colamd_ordering,
gtsam/inference/Ordering.cpp:43-125): the reference's default ordering, whose Bayes tree is chain-like — hundreds of
cliques deep — where nested dissection gives a balanced one.

Stored as int32 positions into the problem's ascending-key variable table (ordering = var_keys[perm]); the
reference tree is needed to build libccolamd_ref.so, so this runs in the build container only.

    python tests/golden/make_colamd_orderings.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from gtsam_petercdev_amd import datasets  # noqa: E402
from oracle import oracle  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    arr = datasets.synth_manhattan_pose2(400, seed=3)
    keys = oracle.colamd_ordering(arr)
    perm = np.searchsorted(arr.var_keys, keys).astype(np.int32)
    assert np.array_equal(arr.var_keys[perm], keys) and np.array_equal(np.sort(perm), np.arange(arr.n_vars))
    np.save(os.path.join(HERE, "colamd_perm_pose2_400_seed3.npy"), perm)
    print("pose2_400_seed3", perm.size, "variables")


if __name__ == "__main__":
    main()
