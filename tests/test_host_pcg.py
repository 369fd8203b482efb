"""Host side of the PCG solver (include/gsx.h: gsx_solve_pcg / gsx_set_linear_solver): the float64 restatement of the
reference's loop against its 50-digit twin on the cases the GPU tests use (tests/_pcg_restatement.py) — which is where
the GPU tests' bounds come from —, the block build against numpy's Cholesky, the defaults against the reference's header,
and the entry points' behaviour without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gtsam_petercdev_amd import _abi as A
from gtsam_petercdev_amd import _lib
from tests import _pcg_restatement as R

# Deviation of the float64 restatement from the 50-digit one over all cases and configurations, per preconditioner,
# measured on the host Jacobians: {preconditioner: (x relative in the A-norm, gamma_initial / gamma_final relative)}.  The
# unpreconditioned figures come from the 14-iteration runs on pose3example (and its Huber variant), which end on a steep
# drop of gamma.  The GPU tests give the device 8x these (tests/test_gpu_pcg.py).
DEV = {R.BLOCK_JACOBI: (6.2e-13, 4.3e-13), R.DUMMY: (6.3e-5, 1.2e-3)}


@pytest.fixture(scope="module")
def systems(oracle):
    out = {}
    for name, make in R.CASES.items():
        arr = make()
        out[name] = (arr,) + R.host_jacobian_system(arr, oracle)
    return out


@pytest.mark.parametrize("name", list(R.CASES))
def test_float64_restatement_against_50_digits(systems, name):
    arr, J, rhs = systems[name]
    worst = {pc: [0.0, 0.0] for pc in DEV}
    for pc, dg, lam in R.CONFIGS:
        D = R.damping_vector(J, dg)
        picked = R.pick_epsilon(J, rhs, arr.var_dims, lam, D, R.Params(preconditioner=pc))
        assert picked is not None, (name, pc, dg, lam, "no decisive stop: replace the case")
        prm = R.Params(500, 1, 501, picked[0], 0.0, pc)
        a = R.pcg_float64(J, rhs, arr.var_dims, lam, D, prm)
        assert R.stop_is_decisive(a) and a.k == picked[1], (name, pc, dg, lam, a.k, picked)
        m = R.pcg_mp(J, rhs, arr.var_dims, lam, D, prm)
        assert m.k == a.k, (name, pc, dg, lam, m.k, a.k)
        dx = R.a_norm(J, lam, D, a.x - m.x) / R.a_norm(J, lam, D, m.x)
        dgam = max(abs(a.gamma_initial - m.gamma_initial) / m.gamma_initial,
                   abs(a.gamma_final - m.gamma_final) / m.gamma_final)
        worst[pc] = [max(worst[pc][0], dx), max(worst[pc][1], dgam)]
    for pc, (wx, wg) in worst.items():
        print(f"{name} preconditioner {pc}: float64 vs 50 digits: x {wx:.2e} (A-norm, relative), gamma {wg:.2e}")
        assert wx <= DEV[pc][0] and wg <= DEV[pc][1], (name, pc)


@pytest.mark.parametrize("name", list(R.CASES))
def test_block_build_is_the_cholesky_factor_of_the_damped_block(systems, name):
    arr, J, rhs = systems[name]
    toff = arr.tangent_offsets()
    for dg, lam in ((0, 1e-3), (1, 10.0)):
        D = R.damping_vector(J, dg)
        blocks = R.build_blocks(J, [int(d) for d in arr.var_dims], lam, D)
        for v, L in enumerate(blocks):
            Jv = J[:, toff[v]:toff[v + 1]]
            H = Jv.T @ Jv + lam * np.diag(D[toff[v]:toff[v + 1]])
            ref = np.linalg.cholesky(H)
            # (normwise: the forward error of a Cholesky factor is bounded by d eps cond(H) |L|, d <= 9 here)
            assert np.abs(L - ref).max() <= 16 * np.finfo(float).eps * np.linalg.cond(H) * np.abs(ref).max(), (name, v)
            assert np.all(np.triu(L, 1) == 0)


def test_defaults_are_the_headers():
    """ConjugateGradientParameters() — gtsam/linear/ConjugateGradientSolver.h:45-51: minIterations(1), maxIterations(500),
    reset(501), epsilon_rel(1e-3), epsilon_abs(1e-3)."""
    p = _lib.pcg_params_default()
    assert (p.min_iterations, p.max_iterations, p.reset, p.epsilon_rel, p.epsilon_abs) == (1, 500, 501, 1e-3, 1e-3)
    assert p.preconditioner == A.PRECOND_BLOCK_JACOBI
    q = R.Params()
    assert (q.min_iterations, q.max_iterations, q.reset, q.epsilon_rel, q.epsilon_abs) == (1, 500, 501, 1e-3, 1e-3)
    import gtsam_petercdev_amd as gt
    g = gt.PCGSolverParameters()
    assert (g.minIterations, g.maxIterations, g.reset, g.epsilon_rel, g.epsilon_abs) == (1, 500, 501, 1e-3, 1e-3)


def test_exports_exist():
    lib = _lib.load()
    for name in ("gsx_pcg_params_default", "gsx_solve_pcg", "gsx_set_linear_solver"):
        assert hasattr(lib, name), name
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "gsx.h")).read()
    assert re.search(r"int32_t pcg_iterations;[^}]*\} gsx_lm_result;", hdr, re.S)      # trailing fields only
    assert re.search(r"int64_t n_pcg_solves;[^}]*\} gsx_stats;", hdr, re.S)
    assert A.LMResult._fields_[-1][0] == "pcg_iterations" and A.Stats._fields_[-1][0] == "n_pcg_solves"


def _host_backend():
    return _lib.ProductBackend(R.CASES["pose2example"](), host_only=True)


def test_argument_checks():
    be = _host_backend()
    fn = be._fn("solve_pcg")
    good = _lib.pcg_params_default()
    st_out, bad = A.PCGStats(), C.c_uint64()

    def call(prm, lam=0.0, n=be.tangent_size, out=True, h=be._h):
        buf = np.zeros(max(n, 1))
        return fn(h, C.c_double(lam), C.c_int32(0), C.c_double(1e-6), C.c_double(1e32),
                  C.byref(prm) if prm is not None else None, buf.ctypes.data_as(C.POINTER(C.c_double)) if out else None,
                  C.c_int64(n), C.byref(st_out), C.byref(bad))
    assert call(None) == A.GSX_E_INVALID
    assert call(good, h=None) == A.GSX_E_INVALID
    assert call(good, lam=-1.0) == A.GSX_E_INVALID
    assert call(good, lam=float("nan")) == A.GSX_E_INVALID
    assert call(good, n=be.tangent_size + 1) == A.GSX_E_INVALID
    for field, value in (("reset", 0), ("max_iterations", -1), ("min_iterations", -1), ("epsilon_rel", -1.0),
                         ("epsilon_abs", float("nan")), ("preconditioner", 2)):
        prm = _lib.pcg_params_default()
        setattr(prm, field, value)
        assert call(prm) == A.GSX_E_INVALID, field
        with pytest.raises(A.GsxError) as e:
            be.set_linear_solver(A.SOLVER_PCG, prm)
        assert e.value.status == A.GSX_E_INVALID, field
    with pytest.raises(A.GsxError) as e:
        be.set_linear_solver(7)
    assert e.value.status == A.GSX_E_INVALID
    be.set_linear_solver(A.SOLVER_PCG)           # host state only: needs no device
    be.set_linear_solver(A.SOLVER_MULTIFRONTAL)


@pytest.mark.skipif(_lib.device_count() > 0, reason="a GPU is visible: the numeric path is tested in test_gpu_pcg.py")
def test_no_device_is_an_error_not_a_fallback():
    be = _host_backend()
    with pytest.raises(A.GsxError) as e:
        be.solve_pcg()
    assert e.value.status == A.GSX_E_NO_DEVICE


def test_refusals_known_on_the_host():
    """PCG on a sharded handle and on hard constraints: refused by gsx_set_linear_solver before any device work."""
    be = _host_backend()
    be.set_shard(0, 2, lambda ptr, n: None)
    with pytest.raises(A.GsxError) as e:
        be.set_linear_solver(A.SOLVER_PCG)
    assert e.value.status == A.GSX_E_STATE and "sharded" in str(e.value)
    be2 = _host_backend()
    be2.set_linear_solver(A.SOLVER_PCG)
    with pytest.raises(A.GsxError) as e:
        be2.set_shard(0, 2, lambda ptr, n: None)
    assert e.value.status == A.GSX_E_STATE and "sharded" in str(e.value)
    arr = R.CASES["pose2example"]()
    con = arr.with_factor(A.F_PRIOR, [1], 3, arr.values[3:6], A.NOISE_CONSTRAINED, [0.0, 0.0, 0.0, 1000.0, 1000.0, 1000.0])
    be3 = _lib.ProductBackend(con, host_only=True)
    with pytest.raises(A.GsxError) as e:
        be3.set_linear_solver(A.SOLVER_PCG)
    assert e.value.status == A.GSX_E_STATE and "constraint" in str(e.value)
