"""The Hessian assembly judged panel by panel in every kernel class (tests/_assembly_cases.py).

For every case: the handle itself says, through gsx_get_hessian_groups, that each variable went to the class, bundle and
launch group the case was built for (a moved threshold fails the case by name); then every variable's panel, read with
gsx_get_hessian_panel, is judged against the longdouble panel formed from the handle's own [A b] blocks — equality on the
integer data, the derived gamma_k bound on the real data; diag(H) is the panels' diagonals bit for bit, and a second
linearize + assembly gives the same bits.  Star cases run on a default handle and on one created under GSX_FUSED_STAR=0.
The worst ratio per class is printed in units of u next to the largest k it was held to.

The partial path, once per class (_assembly_cases.partial_case): two of four variables of one launch group are moved with
gsx_relinearize_partial, which reassembles the dirty variables of every group alone (the star ones through the unbundled
kernel); afterwards every panel is bit for bit that of a fresh handle's full assembly at the same values.

What gsx_get_hessian_panel can see: it completes the star group with the bundle kernel first (dev_ensure_hstar), so on a
default handle it returns that kernel's output, not what front_star_leaf_kernel formed in registers nor what the
unbundled launch over the star variables that are no leaves wrote; that those roads give the same bits is seen here only
through the partial path (unbundled against bundled) and, for the star leaves, by test_gpu_fused_star.py through the
solves.
"""
import numpy as np
import pytest

from gtsam_petercdev_amd import _abi as A

from tests import _assembly_cases as AC
from tests._switches import switches

pytestmark = pytest.mark.gpu

WORST = {}   # class -> (worst ratio in u, k of that panel's bound, case)
RAN = set()


@pytest.fixture(scope="module")
def gpu():
    from gtsam_petercdev_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the HIP path has no fallback"
    return _lib


def _two_step(gpu, arr):
    """A handle that keeps the two-step star path (the switch is read when a handle is created)."""
    with switches(GSX_FUSED_STAR="0"):
        return gpu.product_backend(arr)


def _panels(be, arr):
    return [be.hessian_panel(int(k)) for k in arr.var_keys]


def _judge_handle(be, case, arr, data, two_step):
    be.set_ordering(case.ordering)
    groups = be.hessian_groups()
    AC.check_groups(case, groups)
    if two_step:
        assert groups["fused_diag_star"] == case.fused, case.name
    else:
        assert not groups["fused_diag_star"] or case.fused, case.name
    with pytest.raises(A.GsxError) as e:    # nothing to assemble from yet
        be.hessian_panel(int(arr.var_keys[0]))
    assert e.value.status == A.GSX_E_STATE
    be.linearize()
    jac = be.jacobians()
    if data == "int":   # the blocks are the integers the case drew
        assert np.array_equal(jac, AC.host_jacobians(arr))
    panels = _panels(be, arr)
    off = arr.tangent_offsets()
    hd = be.hessian_diagonal()
    for v, (got, row_var, row_scalar) in enumerate(panels):
        p = AC.expected_panel(arr, jac, v, case.ordering)
        assert got.shape == p.exact.shape, (case.name, v)
        assert np.array_equal(row_var, p.row_var) and np.array_equal(row_scalar, p.row_scalar), (case.name, v)
        cls = int(groups["class"][v])
        ok, worst, k = AC.judge(got, p, cls, data)
        if data == "real" and worst >= WORST.get(cls, (-1.0,))[0]:
            WORST[cls] = (worst, k, case.name)
        assert ok, "%s %s: variable %d (%s): worst %.2f u against k <= %d" % (case.name, data, v, AC.NAMES[cls], worst, k)
        d = got.shape[1]
        assert np.array_equal(hd[off[v]:off[v] + d], got[:d].diagonal()), (case.name, v)
    be.linearize()
    for v, (again, _, _) in enumerate(_panels(be, arr)):
        assert np.array_equal(again, panels[v][0]), (case.name, v)
    return panels


@pytest.mark.parametrize("data", AC.DATA)
@pytest.mark.parametrize("name", list(AC.CASES))
def test_every_panel_of_the_case(gpu, name, data):
    case = AC.CASES[name]
    arr = case.arrays(data)
    be = gpu.product_backend(arr)
    panels = _judge_handle(be, case, arr, data, two_step=False)
    be.close()
    if case.is_star_case or name.startswith("both"):
        tb = _two_step(gpu, arr)
        two = _judge_handle(tb, case, arr, data, two_step=True)
        tb.close()
        for v in range(arr.n_vars):   # two handles with different launch plans, the same panels (module docstring: both
            # star groups were completed by the bundle kernel, or by the unbundled one where a variable has 65 factors)
            assert np.array_equal(two[v][0], panels[v][0]), (name, v)
    RAN.add((name, data))
    if name in AC.BOTH_SAME:   # a group alone and the same group in the fused launch
        both = AC.CASES["both_diag_and_star"]
        barr = both.arrays(data)
        for make in (gpu.product_backend, lambda a: _two_step(gpu, a)):
            bb = make(barr)
            bb.set_ordering(both.ordering)
            bb.linearize()
            for v in AC.BOTH_SAME[name]:
                assert np.array_equal(bb.hessian_panel(v)[0], panels[v][0]), (name, v)
            bb.close()


@pytest.mark.parametrize("cls", range(6), ids=AC.NAMES)
def test_partial_path_gives_the_bits_of_a_full_assembly(gpu, cls):
    pc = AC.partial_case(cls)
    arr = pc.arr

    def handle(values=None):
        be = gpu.product_backend(arr)
        be.set_amalgamation(0.0, 128)   # the reference's cliques: the padding leaves stay cliques of their own
        if values is not None:
            be.set_values(values)
        be.set_ordering(pc.ordering)
        return be

    be = handle()
    AC.check_partial_groups(pc, be.hessian_groups())
    be.linearize()
    be.solve(0.0, False)
    before = _panels(be, arr)
    off = arr.state_offsets()
    states = np.concatenate([np.linspace(0.5, -1.5, pc.dims[v]) + v for v in pc.moved])
    stats = be.relinearize_partial(arr.var_keys[pc.moved], states)
    dirty = AC.partial_dirty(pc)
    # the partial path, not the full fall-back (which reports every variable and front)
    assert stats["n_fronts_reeliminated"] < stats["n_fronts"], stats
    assert stats["n_panels_reassembled"] == len(dirty) < arr.n_vars, (stats, dirty)
    assert stats["n_factors_relinearized"] < arr.n_factors, stats
    after = _panels(be, arr)
    values = be.get_values()
    for v, x in zip(pc.moved, np.split(states, np.cumsum([pc.dims[v] for v in pc.moved])[:-1])):
        assert np.array_equal(values[off[v]:off[v + 1]], x)
    fresh = handle(values)
    fresh.linearize()
    assert np.array_equal(be.jacobians(), fresh.jacobians())
    full = _panels(fresh, arr)
    for v in range(arr.n_vars):
        assert np.array_equal(after[v][0], full[v][0]), (pc.name, v)
        assert np.array_equal(after[v][1], full[v][1])
    for v in pc.moved:   # the move is in the panels: a panel left stale would not pass
        assert not np.array_equal(after[v][0][-1], before[v][0][-1]), (pc.name, v)
    for v in set(range(arr.n_vars)) - set(dirty):
        assert np.array_equal(after[v][0], before[v][0]), (pc.name, v)
    assert np.array_equal(be.hessian_diagonal(), fresh.hessian_diagonal())
    be.close()
    fresh.close()


def test_worst_ratio_per_class():
    """After the cases: what the real data came to, next to the k it was held to.  The figures are gathered by the case
    tests of this process, so under a selection (-k) or a split over workers this test prints what it has and asserts
    only that; that every class is reached is asserted without conditions, on the host, by
    test_host_assembly_cases.py::test_every_class_and_star_form_is_reached and by each case's own class assertion."""
    if len(RAN) == 2 * len(AC.CASES):   # (the whole file ran)
        assert set(WORST) == set(range(6)), WORST
    for cls, (worst, k, name) in sorted(WORST.items()):
        print("assembly class %-5s worst |got - exact| = %6.2f u |A_B|'|A_A|   (k <= %d, %s)" % (AC.NAMES[cls], worst, k, name))
        assert worst <= k
