"""The schedule switches on the device (csrc/gsx_internal.h: ScheduleOptions; tests/test_host_schedule_options.py without a
GPU): gsx_update keeps the schedule the handle was created with, and the switches that used to be latched per process —
GSX_BS_TREE_OFF, GSX_LINERR_DIRECT, GSX_H_TILE_OFF, GSX_SIDE_OFF — each on a handle of its own beside a default handle in
one process.  The two handles of a pair are never compared with each other (nobody has shown these paths bit-equal): each
is held to the bounds the suite already has for its case."""
import numpy as np
import pytest

from gtsam_petercdev_amd import _abi as A
from tests import _assembly_cases as AC
from tests import _gather_cases as G
from tests import _ld_linear as J
from tests import _ld_scalars as S
from tests import _linear_cases as lcases
from tests import _scalar_cases as scases
from tests._switches import switches
from tests.test_gpu_linear_bounds import _judge
from tests.test_gpu_update import _arrays, _grow, _new_states
from tests.test_host_schedule_options import LEAF, backsolve_plan

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from gtsam_petercdev_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the HIP path has no fallback"
    return _lib


def _pair(gpu, arr, **env):
    """(default handle, handle created under the switches); the environment is back before either gets an ordering."""
    default = gpu.product_backend(arr)
    with switches(**env):
        switched = gpu.product_backend(arr)
    return default, switched


def test_update_keeps_the_schedule_of_the_handle(gpu):
    """A handle created under GSX_TREE_TIERS=0 grows by one keyframe after the environment was restored: the analysis of
    gsx_update gives it no tree front, and it solves what a fresh handle created under the switch solves, word for word."""
    steps = list(_grow(n_poses=4, n_points=20, seed=3))
    (f1, i1), (f2, i2) = steps[1], steps[2]
    arr, arr2 = _arrays(f1, i1), _arrays(f2, i2)
    origin = list(range(len(f1))) + [-1] * (len(f2) - len(f1))
    assert -1 in origin
    amalgamation = (0.25, 64)       # (explicit on both sides: the library's own choice is made per graph)

    def handle(a, ordering=None):
        be = gpu.product_backend(a)
        be.set_amalgamation(*amalgamation)
        be.set_ordering(be.compute_ordering(A.ORDER_SCHUR_ND) if ordering is None else ordering)
        return be

    with switches(GSX_TREE_TIERS="0"):
        gb = handle(arr)
    default = handle(arr)
    assert gb.stats()["n_tree_fronts"] == 0 < default.stats()["n_tree_fronts"]
    gb.linearize()
    gb.solve(1e-3, False)
    st = gb.update(arr2, origin, _new_states(arr2, arr.var_keys))
    assert st["n_factors_added"] == origin.count(-1) > 0
    assert gb.stats()["n_tree_fronts"] == 0
    with switches(GSX_TREE_TIERS="0"):
        fresh = handle(arr2, gb.get_ordering())
    grown = handle(arr2, gb.get_ordering())      # the default schedule of the updated graph has tree fronts to lose
    assert fresh.stats()["n_tree_fronts"] == 0 < grown.stats()["n_tree_fronts"]
    assert np.array_equal(gb.front_classes(), fresh.front_classes())
    assert np.array_equal(gb.get_values(), fresh.get_values())
    gb.linearize()
    fresh.linearize()
    assert np.array_equal(gb.jacobians(), fresh.jacobians())
    for lam in (1e-3, 0.0):
        assert np.array_equal(gb.solve(lam, False), fresh.solve(lam, False)), lam
    for be in (gb, default, fresh, grown):
        be.close()


def test_backsolve_tree_off_beside_a_default_handle(gpu):
    """The launches a solve makes are those of the handle's own plan: the default plan (one tree launch) on the default
    handle, the level plan on the handle created under GSX_BS_TREE_OFF.  Counted by the timers of the launches above the
    leaf cliques (gsx_kernel_time("backsolve_launch"), profiling level 1)."""
    arr = lcases.tree_arrays("pose2")
    counts = []
    for be, tree in zip(_pair(gpu, arr, GSX_BS_TREE_OFF="1"), (True, False)):
        be.set_amalgamation(*lcases.TREE_AMALGAMATION)
        be.set_ordering(be.compute_ordering(A.ORDER_ND))
        st = be.stats()
        assert st["n_tree_fronts"] > 0 and st["n_big_fronts"] == 0     # the factorization keeps its tree kernels on both
        if tree:
            want = sum(1 for r in backsolve_plan(be, 1) if r[0] != LEAF)
        else:
            want = len({r[4] for r in backsolve_plan(be, 0) if r[1] != LEAF})
        be.linearize()
        judge = J.Judge(arr, be.jacobians())
        _judge(be, judge, f"GSX_BS_TREE_OFF beside a default handle, tree launch {tree}", step=False)
        be.set_profiling(1)
        be.solve(*lcases.LAMBDAS[0])
        be.synchronize()
        n = be.kernel_time("backsolve_launch")[1]
        assert n == want, (tree, n, want)
        counts.append(n)
        be.close()
    assert counts[0] == 1 < counts[1], counts


def test_linerr_direct_beside_a_default_handle(gpu):
    """One solved LM trial: the default handle takes e(0) from lin0_kernel and e(delta) from the model, the handle created
    under GSX_LINERR_DIRECT evaluates both over [A b] — the very numbers of gsx_linear_error at the trial's step."""
    arr = scases.chain(65)
    assert scases.slice_of(arr)[1] > 0
    k_eval = S.k_linear_error_staged(arr)
    lam, diag = 1e-3, False
    for be, direct in zip(_pair(gpu, arr, GSX_LINERR_DIRECT="1"), (False, True)):
        be.set_ordering(be.compute_ordering(A.ORDER_MINDEGREE))
        be.linearize()
        sc = S.Scalars(arr, be.jacobians())
        e0, ed, _ = be.lm_trial(False, lam, diag)
        x = be.solve(lam, diag)             # the trial's step: the same factorization and substitution again
        tag = f"GSX_LINERR_DIRECT beside a default handle, direct {direct}"
        if direct:
            sc.check_e0(e0, k_eval, tag)
            sc.check_ed(ed, x, k_eval, tag)
            assert (e0, ed) == be.linear_error(), tag
        else:
            sc.check_e0(e0, S.k_lin0(arr), tag, "e0 (lin0)")
            sc.check_model_decrease(e0, ed, x, lam, diag, S.k_model(arr, sc.m), tag)
        be.close()


def test_h_tile_off_beside_a_default_handle(gpu):
    """The panels of a tile case by assemble_h_tile_kernel on the default handle and by the generic kernels on the handle
    created under GSX_H_TILE_OFF, each judged panel by panel under the bound of the class it ran in."""
    case = AC.CASES["tile_group_of_4"]
    for data in AC.DATA:
        arr = case.arrays(data)
        for be, tile in zip(_pair(gpu, arr, GSX_H_TILE_OFF="1"), (True, False)):
            be.set_ordering(case.ordering)
            groups = be.hessian_groups()
            if tile:
                AC.check_groups(case, groups)
            assert (AC.TILE in groups["class"]) == tile, (tile, groups["class"])
            be.linearize()
            jac = be.jacobians()
            for v, k in enumerate(arr.var_keys):
                got, row_var, row_scalar = be.hessian_panel(int(k))
                p = AC.expected_panel(arr, jac, v, case.ordering)
                assert got.shape == p.exact.shape, (tile, v)
                assert np.array_equal(row_var, p.row_var) and np.array_equal(row_scalar, p.row_scalar), (tile, v)
                cls = int(groups["class"][v])
                ok, worst, kk = AC.judge(got, p, cls, data)
                assert ok, "tile %s %s: variable %d (%s): worst %.2f u against k <= %d" % (tile, data, v, AC.NAMES[cls], worst, kk)
            be.close()


def test_side_off_beside_a_default_handle(gpu):
    """stacked_blocked reaches the side group under GSX_SIDE_MIN=1; a handle created under GSX_SIDE_OFF as well has no side
    level in its plan.  Both are judged as test_gpu_extend_add.py judges the case."""
    case = G.build("stacked_blocked")
    handles = []
    with switches(**case.env):
        handles.append(gpu.product_backend(case.arr))
        with switches(GSX_SIDE_OFF="1"):
            handles.append(gpu.product_backend(case.arr))
    for be, side in zip(handles, (True, False)):
        be.set_amalgamation(*G.AMALGAMATION)
        be.set_ordering(case.arr.var_keys[case.ordering])
        plan = G.plan_of(be.gather_plan())
        assert any(s.group == G.SIDE for s in plan.segments) == side, side
        if side:
            assert case.declares <= G.branches_of(plan, be.front_classes())
        be.linearize()
        judge = J.Judge(case.arr, be.jacobians())
        lam, diag = lcases.LAMBDAS[0]
        assert np.array_equal(be.solve(lam, diag), be.solve(lam, diag)), (side, "two solves at one lambda differ")
        _judge(be, judge, f"GSX_SIDE_OFF beside a default handle, side group {side}")
        be.close()
