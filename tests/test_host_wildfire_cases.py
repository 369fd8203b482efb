"""The cases of tests/_wildfire_cases.py are what they claim, on the CPU: the CPU oracle (whose Bayes tree is the product's
at amalgamation 0) for the conditionals and the traversal, the host-only product backend for the tree and the front
classes.  Pinned per case: the tree shape, the kernel every clique under test is back-substituted in on the level path,
the outcome of every arm in each of the three steps, and the margin condition — every solved clique's change is at
least 100 thresholds or at most a hundredth of one, and the root's is at least 100 in steps 1 and 2 — which is a
condition of the inputs: it makes the device's float64 rounding unable to flip a decision of
test_gpu_wildfire_classes.py.  The worst margin of each step is printed."""
import ctypes as C

import numpy as np
import pytest

from tests import _wildfire_cases as W


@pytest.fixture(scope="module")
def big_lds():
    from gtsam_petercdev_amd import _lib
    f = _lib.load().gsxtest_backsolve_big_lds
    f.restype = C.c_longlong
    f.argtypes = [C.c_int, C.c_int, C.c_int]
    return f


def _host_tree(case, amalgamation):
    from gtsam_petercdev_amd import _lib
    hb = _lib.ProductBackend(case.arr, host_only=True)      # (accepts the mixed F_LINEAR / F_PRIOR graph)
    hb.set_amalgamation(*amalgamation)
    hb.set_ordering(case.arr.var_keys[case.ordering])
    parent, fronts = hb.get_tree()
    cls = [int(c) for c in hb.front_classes()]
    hb.close()
    return [int(p) for p in parent], [(list(f), list(s)) for f, s in fronts], cls


@pytest.mark.parametrize("name", list(W.CASES))
def test_case_is_what_it_claims(oracle, big_lds, name):
    case = W.build(name)
    arr = case.arr
    dims = [int(d) for d in arr.var_dims]
    assert set(W.CASES) == set(W.INTENDED) == set(W.THRESHOLDS)
    O = oracle.oracle_backend(arr)
    O.set_ordering(arr.var_keys[case.ordering])
    O.linearize()
    d_prev = O.solve(0.0, False)
    po, fo = O.get_tree()
    po, fo = [int(p) for p in po], [(list(f), list(s)) for f, s in fo]
    parent, fronts, cls = _host_tree(case, W.AMALGAMATION)
    # (the oracle numbers its cliques depth first, the product in elimination order: the same cliques and edges)
    canon = lambda par, frs: sorted((tuple(f), tuple(sorted(s)), frs[par[c]][0][0] if par[c] >= 0 else -1)
                                    for c, (f, s) in enumerate(frs))
    assert canon(parent, fronts) == canon(po, fo), "the product's tree at amalgamation 0 is the oracle's"
    # ---- the tree: bottom cliques, padding leaves, middle cliques, the root; three storeys; the partial path's 20 fronts
    nf = len(fronts)
    assert nf == 2 * len(case.arms) + len(case.pads) + 1 >= 20, nf
    root = nf - 1
    assert parent[root] == -1 and fronts[root] == (case.root, []) and W.levels_of(parent)[root] == 2
    front_of = {f[0]: c for c, (f, _) in enumerate(fronts)}
    r0 = case.root[0]
    for arm in case.arms:
        a, m = front_of[arm.a_vars[0]], front_of[arm.m_vars[0]]
        assert fronts[m] == (arm.m_vars, [r0]) and parent[m] == root
        assert fronts[a][0] == arm.a_vars and parent[a] == m and set(fronts[a][1]) < set(arm.m_vars) | {-1}
        assert W.clique_shapes(fronts, dims)[a] == (arm.fa, arm.sep) and W.clique_shapes(fronts, dims)[m] == (arm.fm, 3)
    for p in case.pads:
        assert fronts[front_of[p]] == ([p], [r0]) and dims[p] in (1, 3)
    assert sum(dims) <= 640, sum(dims)                       # (the long-double judge stays cheap)
    # s meets r0 and r1 only, its prior is the one nonlinear factor: marking s dirties the root alone
    touched = set()
    for f in range(arr.n_factors):
        vs = [int(v) for v in arr.f_vars[arr.f_key_ptr[f]:arr.f_key_ptr[f + 1]]]
        if case.s_var in vs:
            touched.update(vs)
    assert touched == set(case.root)
    # ---- the kernel of every clique under test
    kern = W.kernel_of(parent, fronts, cls, dims, big_lds)
    targets = W.target_cliques(case, fronts)
    assert sorted(set(s for _, s in targets.values())) == sorted(case.shapes)
    for c, (kind, shape) in targets.items():
        assert kern[c] == W.INTENDED[name][shape], (name, c, kind, shape, kern[c])
        assert (cls[c] & 3 == 0) == kern[c].startswith("leaf")
    assert set(kern) <= W.BRANCHES, set(kern)                # (the 64-thread generic launch: unreachable, module docstring)
    plain = W.kernel_of(parent, fronts, cls, dims, big_lds, packed=False)
    assert all(k in ("leaf64", "leaf_tail") for k, c in zip(plain, cls) if c & 3 == 0)
    # ---- the three steps on the oracle (its numbering from here on: conditional(c) is the oracle's)
    parent, fronts = po, fo
    root = [c for c, p in enumerate(parent) if p < 0][0]
    front_of = {f[0]: c for c, (f, _) in enumerate(fronts)}
    targets = W.target_cliques(case, fronts)
    values = arr.values.copy()
    a_of = {arm.kind + str(i): front_of[arm.a_vars[0]] for i, arm in enumerate(case.arms)}
    m_of = {arm.kind + str(i): front_of[arm.m_vars[0]] for i, arm in enumerate(case.arms)}
    first = None
    for step, (move, thr) in enumerate(W.steps(name)):
        values, _ = W.moved_values(case, values, move)
        O.set_values(values)
        O.linearize()
        O.solve(0.0, False)
        wf = W.wildfire_restatement(parent, fronts, O.conditional, dims, d_prev, {root}, thr)
        margin = W.worst_margin(wf, {root}, thr)
        print(f"{name} step {step + 1}: threshold {thr:g}, solved {wf.count} of {arr.n_vars} variables, worst margin "
              f"{margin:.0f}, root change / threshold {wf.change[root] / thr:.3g}")
        assert margin >= 100, (name, step, margin)
        assert wf.outcome[root] == W.KEPT
        out_a = {k: wf.outcome[c] for k, c in a_of.items()}
        out_m = {k: wf.outcome[c] for k, c in m_of.items()}
        by_shape = {}
        for c, (kind, shape) in targets.items():
            by_shape.setdefault(shape, set()).add(wf.outcome[c])
        if step == 0:
            assert wf.change[root] >= 100 * thr
            for k in a_of:
                assert (out_m[k], out_a[k]) == {"a": (W.KEPT, W.KEPT), "b": (W.KEPT, W.RESTORED),
                                                "c": (W.RESTORED, W.SKIPPED)}[k[0]], (name, k, out_m[k], out_a[k])
            for shape, seen in by_shape.items():             # all three outcomes for the shape under test, side by side
                # (combined1024's (193, 5) shape has arms a and c only)
                want = {W.KEPT, W.RESTORED, W.SKIPPED} if case.position == "bottom" else {W.KEPT, W.RESTORED}
                assert seen == want or (name == "combined1024" and shape == (193, 5) and seen == {W.KEPT, W.SKIPPED}), (shape, seen)
            assert W.SKIPPED in set(wf.outcome) and wf.count < arr.n_vars
            first = (out_m, out_a)
        elif step == 1:
            assert wf.change[root] >= 100 * thr
            for k in a_of:       # the c arms cross: M_i kept, A_i solved for the first time (and kept); b as before
                assert (out_m[k], out_a[k]) == ((W.KEPT, W.RESTORED) if k[0] == "b" else (W.KEPT, W.KEPT)), (name, k)
            assert (out_m, out_a) != first
        else:                    # everything under the root is restored, everything below skipped
            assert set(out_m.values()) == {W.RESTORED} and set(out_a.values()) == {W.SKIPPED}
            assert all(wf.outcome[front_of[p]] == W.RESTORED for p in case.pads)
            assert wf.count == sum(len(fronts[c][0]) for c in range(nf) if parent[c] == root) + len(case.root)
        d_prev = wf.delta.astype(np.float64)


@pytest.mark.parametrize("name", W.RELAXED_CASES)
def test_relaxed_tree_merges_reference_cliques(big_lds, name):
    """Under RELAXED amalgamation a front holds several reference cliques (the conditionals of that tree exist on the
    device only: the outcomes are asserted there)."""
    case = W.build(name)
    dims = [int(d) for d in case.arr.var_dims]
    parent, fronts, cls = _host_tree(case, W.RELAXED)
    ref_parent, ref_fronts, _ = _host_tree(case, W.AMALGAMATION)
    assert 7 <= len(fronts) < len(ref_fronts)
    assert sorted(v for f, _ in fronts for v in f) == list(range(case.arr.n_vars))
    kern = W.kernel_of(parent, fronts, cls, dims, big_lds)
    print(name, "relaxed:", len(fronts), "fronts of", len(ref_fronts), "kernels", sorted(set(kern)))
    assert max(W.levels_of(parent)) == (2 if name == "small2" else 1)
    assert fronts[-1][1] == [] and set(case.root) <= set(fronts[-1][0])
    # s still meets root-frontal variables only
    assert set(case.root) <= set(fronts[-1][0])
