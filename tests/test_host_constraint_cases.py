"""The constraint hand-over cases (tests/_constraint_cases.py) before the device is asked: each has the clique structure it
declares, is a well-conditioned full-rank problem, and the reference's path — the oracle's restatement of EliminateQR with
Constrained::QR, on the same ordering — solves it to the 50-digit KKT solution.  No GPU."""
from __future__ import annotations

import numpy as np
import pytest

from gtsam_petercdev_amd import _lib
from tests import _constraint_cases as CC

U = 2.0 ** -53


def host_tree(case, arr):
    hb = _lib.ProductBackend(arr, host_only=True)
    try:
        hb.set_amalgamation(*case.amalgamation)
        hb.set_ordering(case.ordering())
        return hb.get_tree(), hb.stats()
    finally:
        hb.close()


@pytest.mark.parametrize("name", list(CC.ALL))
def test_case_has_the_structure_it_declares(name):
    case = CC.ALL[name]
    arr = case.arrays()
    tree, st = host_tree(case, arr)
    print(case.describe())
    CC.check_structure(case, arr, tree)
    assert st["n_constraint_rows"] == case.n_constraint_rows() == len(CC.constraint_rows(arr))
    assert all(1 <= d <= 3 for _, d in case.variables)
    if name in CC.CASES:
        assert len(case.variables) <= 10
    else:   # padded for the partial path: one dirty front must be under 15 % of the tree (csrc/incremental.hip)
        assert 100 < 15 * len(tree[0])
    # other numbers, same structure (the kept-handle test hands them over)
    arr1 = case.arrays(1)
    assert np.array_equal(arr1.f_vars, arr.f_vars) and not np.array_equal(arr1.meas, arr.meas)


@pytest.mark.parametrize("name", list(CC.ALL))
def test_case_is_exact_well_conditioned_and_solved_by_the_reference_path(oracle, name):
    case = CC.ALL[name]
    for variant in (0, 1) if name in CC.CASES else (0,):
        arr = case.arrays(variant)
        # exact inputs: quarters of magnitude <= 2, sigmas 1 and 1/2
        assert np.array_equal(arr.meas * 4, np.round(arr.meas * 4)) and np.abs(arr.meas).max() <= 2.0
        jac = CC.stated_jacobians(arr)
        ob = oracle.oracle_backend(arr)
        ob.set_ordering(case.ordering())
        ob.linearize()
        assert np.array_equal(ob.jacobians(), jac)
        hd = CC.hessian_diagonal(arr, jac)
        assert np.array_equal(ob.hessian_diagonal(), hd)
        ref = CC.reference(name, variant)
        for lam, diag in CC.DAMPINGS:
            K, _ = CC.kkt_matrix(arr, jac, lam, hd if diag else np.ones_like(hd))
            cond = np.linalg.cond(K)
            assert np.linalg.matrix_rank(K) == K.shape[0]
            x = ref[(lam, diag)]
            do = ob.solve(lam, diag)            # raises on anything but GSX_OK
            err = np.abs(do - x).max() / np.abs(x).max()
            print(f"{name} variant {variant} lam {lam} diagonal {diag}: cond2(KKT) {cond:.3e}, "
                  f"oracle vs 50 digits {err:.2e} |x|inf")
            assert cond <= 1e4
            # cond <= 1e4 and u = 1.1e-16 leave two orders of margin
            assert err <= 1e-12
            # the 50-digit step itself: the constraint rows hold to rounding of the float64 it was rounded to
            _, Cc = CC.dense_rows(arr, jac)
            assert np.all(np.abs(Cc[:, :-1] @ x - Cc[:, -1]) <= 4 * U * (np.abs(Cc[:, :-1]) @ np.abs(x) + np.abs(Cc[:, -1])))


def test_a_row_that_says_zero_equals_d_is_dropped_by_the_reference_path(oracle):
    """A constraint row whose entries ALL vanish (frontal and separator) while its rhs does not: Constrained::QR finds no
    pivot for it in any column and nothing of it reaches a conditional — the oracle returns GSX_OK and the step is that of
    the graph without the row.  (Recorded here; tests/test_gpu_constraint_handover.py asserts the device's verdict is the
    same.)"""
    case, arr, zero_row = CC.vanishing_row_case()
    jac = CC.stated_jacobians(arr)
    f, r = zero_row
    joff = arr.jacobian_offsets()
    row = jac[joff[f] + r:joff[f + 1]:arr.f_rows[f]]
    assert np.all(row[:-1] == 0.0) and row[-1] != 0.0
    ob = oracle.oracle_backend(arr)
    ob.set_ordering(case.ordering())
    ob.linearize()
    hd = CC.hessian_diagonal(arr, jac)
    for lam, diag in CC.DAMPINGS:
        do = ob.solve(lam, diag)                # GSX_OK: anything else raises
        x = np.array([float(v) for v in CC.kkt_step_mp(arr, jac, lam, hd if diag else np.ones_like(hd), skip=[zero_row])])
        assert np.abs(do - x).max() <= 1e-12 * np.abs(x).max()


def test_the_judge_is_the_float64_kkt_statement():
    """kkt_step_mp against dense_kkt_step's own arithmetic (numpy.linalg.solve of the same matrix) at float64 accuracy."""
    case = CC.CASES["three_supports"]
    arr = case.arrays()
    jac = CC.stated_jacobians(arr)
    hd = CC.hessian_diagonal(arr, jac)
    n = hd.size
    for lam, diag in CC.DAMPINGS:
        K, rhs = CC.kkt_matrix(arr, jac, lam, hd if diag else np.ones_like(hd))
        x = np.linalg.solve(K, rhs)[:n]
        assert np.allclose(x, CC.reference(case.name)[(lam, diag)], rtol=0, atol=1e-11 * np.abs(x).max())
