"""The extend-add into blocked fronts (kernels.hip: big_gather_seg_kernel, big_gather_combine_kernel; the plan of
symbolic.cpp; its filtered copy in gsx_relinearize_partial) under the float64 backward-error judge of tests/_ld_linear.py,
on the cases of tests/_gather_cases.py: every source kind (product form with F <= 4 in groups of four with tails of one,
two and three, the SAME diagonal variant, the product loop with and without a tail, stored blocks, fast sources forced
down the generic path), segments of 63 / 64 sources, two- and three-slot combines, a last segment of one source, slots
that run on over the tasks of a group and the side group's own range, unequal and full tiles, blocks wider than a tile
with more than 64 sources, mixed tasks and two tasks for one block, and launches of 3, 32 and 33 segments.  Which branches
a case took is read from the plan of the very handle that was judged (gsx_get_gather_plan); the last test asserts that
their union is _gather_cases.BRANCHES.

Per case: measures (1)-(3) and the step over _linear_cases.LAMBDAS with the derived k (no tolerance of this module's
own), and a repeated solve that must be bit-equal (the gather has no atomics).  On segment_edges and stacked_blocked the
neighbouring-lambda sequence on one arena (a stale scratch slot or a front not re-initialised is 1e7 u off).  On
segment_edges, stored_sources and stacked_blocked two partial re-eliminations each, bit-equal to the full path and judged.
test_host_gather_cases.py shows that the judge rejects one dropped source on each of these inputs.

Measured on the MI355X (worst over the module): factor 11.2 u, rhs 4.9 u, solve 2.1 u against k of 400 to 1800 (factor,
rhs) and 1000 to 4200 (solve); step 0.50 u kappa_2 (kappa_2 32 to 232).
SEEN and WORST are filled by the tests above the last one: it means something only when the whole module runs in one
process, in file order."""
import numpy as np
import pytest

from tests import _gather_cases as G
from tests import _ld_linear as J
from tests import _linear_cases as cases

pytestmark = pytest.mark.gpu

SEEN = set()
WORST = {"factor": 0.0, "rhs": 0.0, "solve": 0.0, "step": 0.0}


@pytest.fixture(scope="module")
def gpu():
    from gtsam_petercdev_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the HIP path has no fallback"
    return _lib


def _handle(gpu, case, monkeypatch):
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    gb = gpu.product_backend(case.arr)
    gb.set_amalgamation(*G.AMALGAMATION)
    gb.set_ordering(case.arr.var_keys[case.ordering])
    return gb


def _device_case(gpu, name, monkeypatch):
    """(case, backend, judge from the device's own [A b]); the declared branches asserted on the plan of this handle."""
    case = G.build(name)
    gb = _handle(gpu, case, monkeypatch)
    got = G.branches_of(G.plan_of(gb.gather_plan()), gb.front_classes())
    assert case.declares <= got, (name, sorted(case.declares - got))
    SEEN.update(got)
    gb.linearize()
    return case, gb, J.Judge(case.arr, gb.jacobians())


def _judge(gb, judge, what, lambdas, step=True):
    for lam, diag in lambdas:
        x = gb.solve(lam, diag)
        f, r, s = judge.check_backward(gb, x, lam, diag, what)
        for k, v in (("factor", f), ("rhs", r), ("solve", s)):
            WORST[k] = max(WORST[k], v)
        if step:
            WORST["step"] = max(WORST["step"], judge.check_step(x, lam, diag, what))


@pytest.mark.parametrize("name", G.NAMES)
def test_extend_add_case(gpu, name, monkeypatch):
    case, gb, judge = _device_case(gpu, name, monkeypatch)
    lam, diag = cases.LAMBDAS[0]
    x = gb.solve(lam, diag)
    assert np.array_equal(x, gb.solve(lam, diag)), (name, "two solves at one lambda differ")
    _judge(gb, judge, f"extend-add {name}", cases.LAMBDAS)
    gb.close()


@pytest.mark.parametrize("name", ["segment_edges", "stacked_blocked"])
def test_neighbouring_lambdas_on_one_arena(gpu, name, monkeypatch):
    """test_gpu_linear_bounds.py's sequence: lambda1 = 0.1, lambda2 = 0.1 (1 + 1e-8), 0, lambda2 again, each result judged
    for ITS lambda — with combine tasks whose scratch slots are reused from trial to trial."""
    case, gb, judge = _device_case(gpu, name, monkeypatch)
    l2 = 0.1 * (1 + 1e-8)
    _judge(gb, judge, f"neighbouring lambdas {name}", [(0.1, True), (l2, True), (0.0, False), (l2, True)], step=False)
    gb.close()


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("name", ["segment_edges", "stored_sources", "stacked_blocked"])
def test_partial_reelimination(gpu, name, which, monkeypatch):
    """One leaf moves (Case.movable: a leaf of a multi-segment block or the bottom of a stored arm; a leaf of a straight-add
    block, a lean leaf of a mixed task or a leaf of the upper hub): gsx_relinearize_partial re-runs the gather segments of
    the dirty blocked fronts alone, from ALL their children.  Conditionals and step bit-equal to the full path, and judged."""
    case, gb, _ = _device_case(gpu, name, monkeypatch)
    var = case.movable[which]
    gb.solve(0.0, False)
    parent, fronts = gb.get_tree()
    chain = [c for c, (f, _) in enumerate(fronts) if var in f]
    while parent[chain[-1]] >= 0:
        chain.append(int(parent[chain[-1]]))
    state, values = G.state_of(case, var, np.linspace(0.5, -1.5, case.dims[var]))
    stats = gb.relinearize_partial(case.arr.var_keys[[var]], state)
    # the partial path, not the full fallback (which reports every front and factor; taken above 15 % dirty fronts, or
    # above 5 % when they hold most of the segments, as the root does)
    assert len(chain) * 20 <= len(fronts), (chain, len(fronts))
    assert stats["n_fronts_reeliminated"] == len(chain), (stats, chain)
    assert stats["n_factors_relinearized"] < case.arr.n_factors, stats
    partial = [np.array(gb.conditional(c)) for c in range(len(fronts))]
    xp = gb.solve(0.0, False)
    full = _handle(gpu, case, monkeypatch)
    full.set_values(values)
    full.linearize()
    xf = full.solve(0.0, False)
    assert np.array_equal(gb.jacobians(), full.jacobians())
    for c in range(len(fronts)):
        assert np.array_equal(partial[c], np.array(full.conditional(c))), (name, which, "conditional of clique", c)
    assert np.array_equal(xp, xf), (name, which, float(np.max(np.abs(xp - xf))))
    full.close()
    judge = J.Judge(case.arr, gb.jacobians())
    what = f"partial {name} variable {var}"
    f, r, s = judge.check_backward(gb, xp, 0.0, False, what)
    for k, v in (("factor", f), ("rhs", r), ("solve", s)):
        WORST[k] = max(WORST[k], v)
    WORST["step"] = max(WORST["step"], judge.check_step(xp, 0.0, False, what))
    gb.close()


def test_every_branch_was_judged():
    print("branches judged:", sorted(SEEN), "worst ratios (u; step in u*kappa_2):", {k: round(v, 3) for k, v in WORST.items()})
    assert SEEN == G.BRANCHES, sorted(G.BRANCHES ^ SEEN)
