"""The extend-add cases of tests/_gather_cases.py without a GPU: gsx_get_gather_plan on a host-only handle against the plan
restated from the tree (the first direct test of the gather plan of symbolic.cpp), the branches each case is aimed at, the
conditioning of the systems, the CPU oracle under the float64 backward-error judge on every case, and one mutation per
case — the smallest contribution to the fullest block left out of the sum — that measure (1) must reject: the judge would
notice a dropped source on these inputs whatever the device does.

Measured: kappa_2(H) between 32 and 232; the CPU oracle at most factor 11.9 u, rhs 3.5 u, solve 2.6 u against k of 400 to
1800 (factor, rhs) and 1000 to 4200 (solve), step 0.53 u kappa_2; the mutated factor's measure (1) is 4.0e7 bounds k u
on the case where it is smallest (stacked_blocked; 1.3e8 to 6.9e11 on the others), 10 is asserted."""
import numpy as np
import pytest

from gtsam_petercdev_amd import _lib
from tests import _gather_cases as G
from tests import _ld_linear as J
from tests import _linear_cases as cases

_FACTS = {}


def _facts(name, monkeypatch):
    """(case, tree, front classes, the library's plan) from a host-only handle; made once per case."""
    if name not in _FACTS:
        case = G.build(name)
        for k, v in case.env.items():
            monkeypatch.setenv(k, v)
        hb = _lib.ProductBackend(case.arr, host_only=True)
        hb.set_amalgamation(*G.AMALGAMATION)
        hb.set_ordering(case.arr.var_keys[case.ordering])
        parent, fronts = hb.get_tree()
        _FACTS[name] = (case, ([int(p) for p in parent], fronts), [int(c) for c in hb.front_classes()],
                        G.plan_of(hb.gather_plan()))
        hb.close()
    return _FACTS[name]


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.NAMES)
def test_plan_is_the_restated_plan(name, monkeypatch):
    case, tree, cls, plan = _facts(name, monkeypatch)
    rows = [sum(case.dims[v] for v in f + s) + 1 for f, s in tree[1]]
    root = [f for f, p in enumerate(tree[0]) if p < 0]
    assert len(root) == 1 and cls[root[0]] == 2 and rows[root[0]] > 140 and set(tree[1][root[0]][0]) <= set(case.hub)
    assert sum(case.dims) <= 700
    restated = G.restated_plan(tree, cls, case.dims, int(case.env.get("GSX_SIDE_MIN", 4096)))
    assert len(plan.segments) == len(restated.segments)
    for got, want in zip(plan.segments, restated.segments):
        assert got == want
    assert plan.combines == restated.combines
    G.check_plan(plan, tree, cls)


def test_wide_leaves_are_stored_and_never_split(monkeypatch):
    case, tree, cls, plan = _facts("wide_blocks", monkeypatch)
    for f, (fv, sv) in enumerate(tree[1]):
        if any(case.dims[v] > 16 for v in sv):
            assert not cls[f] & 8, (f, "a leaf on a wide variable is lean")
    wide = [s for s in plan.segments if s.dB > 16 or s.dA > 16]
    assert sorted({(s.dB, s.dA) for s in wide}) == [(1, 17), (1, 40), (1, 64), (15, 64), (17, 17), (40, 17), (40, 40), (64, 17),
                                                        (64, 64)]
    assert {len(s.sources) for s in wide} == {1, 65, 130, 131, 195} and all(s.slot == -1 for s in wide)
    assert all(len(s.sources) <= 64 for s in plan.segments if s not in wide)


def test_mixed_sources_share_a_task_or_make_two(monkeypatch):
    """One hub: the stored children run in the group of the lean ones (group 0) and join their task.  Stacked hubs: the
    upper hub's lean leaves run in the side group, its stored child (the lower hub) at the upper hub's own level."""
    case, tree, cls, plan = _facts("stored_sources", monkeypatch)
    h4, h5 = case.hub[4], case.hub[5]
    mixed = [s for s in plan.segments if (s.var_row, s.var_col) == (h5, h4)]
    assert len(mixed) == 1 and [bool(F) for _, F in mixed[0].sources] == [True, False] * 3 + [True]
    case, tree, cls, plan = _facts("stacked_blocked", monkeypatch)
    u0, u1 = case.hub[10], case.hub[11]
    two = [s for s in plan.segments if (s.var_row, s.var_col) == (u1, u0)]
    assert [(s.group, len(s.sources), s.slot >= 0) for s in two] == [(1, 1, False), (G.SIDE, 64, True), (G.SIDE, 2, True)]
    assert cls[two[0].sources[0][0]] == 2 and two[0].sources[0][1] == 0
    side = {s.slot for s in plan.segments if s.group == G.SIDE and s.slot >= 0}
    level = {s.slot for s in plan.segments if s.group != G.SIDE and s.slot >= 0}
    assert side and level and min(side) == max(level) + 1


@pytest.mark.parametrize("name,largest", [("launch_3", 3), ("launch_32", 32), ("launch_33", 33)])
def test_launch_sizes(name, largest, monkeypatch):
    _, _, _, plan = _facts(name, monkeypatch)
    assert {s.group for s in plan.segments} == {0} and len(plan.segments) == largest


def test_every_case_reaches_its_branches(monkeypatch):
    union = set()
    for name in G.NAMES:
        case, tree, cls, plan = _facts(name, monkeypatch)
        got = G.branches_of(plan, cls)
        assert case.declares <= got, (name, sorted(case.declares - got))
        union |= case.declares
    assert union == G.BRANCHES, sorted(G.BRANCHES ^ union)


# ---- the systems ------------------------------------------------------------------------------------------------------------------
_JUDGES = {}


def _oracle_case(oracle, case):
    if case.name not in _JUDGES:
        ob = oracle.oracle_backend(case.arr)
        ob.set_ordering(case.arr.var_keys[case.ordering])
        ob.linearize()
        _JUDGES[case.name] = (ob, J.Judge(case.arr, ob.jacobians()))
    return _JUDGES[case.name]


@pytest.mark.parametrize("name", G.NAMES)
def test_oracle_holds_the_bounds(oracle, name):
    """The CPU oracle under the unchanged k on every case: the bound is reachable by the reference alone.  kappa_2(H) at
    most 1e4: measure (4) means something."""
    case = G.build(name)
    ob, judge = _oracle_case(oracle, case)
    kappa = float(np.linalg.cond(judge.sys.H.astype(np.float64)))
    print(f"{name}: n {judge.sys.n} m {judge.sys.m} kappa_2(H) {kappa:.1f}")
    assert kappa <= 1e4
    for lam, diag in cases.LAMBDAS:
        x = ob.solve(lam, diag)
        judge.check_backward(ob, x, lam, diag, f"oracle {name}")
        judge.check_step(x, lam, diag, f"oracle {name}")


class _DenseFactor:
    """A dense upper-triangular factor R (R'R = the matrix, scalars in the natural = elimination order) and d, cut into
    the conditionals [R S d] of a tree: what J.gather reads."""

    def __init__(self, tree, off, R, d):
        self.parent, self.fronts = tree
        self.off, self.R, self.d = off, R, d

    def scalars(self, vs):
        return np.concatenate([np.arange(self.off[v], self.off[v + 1]) for v in vs]) if len(vs) else np.zeros(0, np.int64)

    def get_tree(self):
        return self.parent, self.fronts

    def conditional(self, c):
        fi, si = self.scalars(self.fronts[c][0]), self.scalars(self.fronts[c][1])
        cols = np.concatenate([fi, si])
        rest = np.setdiff1d(np.arange(self.R.shape[0]), cols)
        assert not np.any(self.R[np.ix_(fi, rest)]), ("clique", c, "fill outside the clique's columns")
        return np.column_stack([self.R[np.ix_(fi, cols)], self.d[fi]])


def _factor(H, g):
    L = np.linalg.cholesky(H)
    return L.T.copy(), np.linalg.solve(L, g)


MUTATION_RATIOS = {}


@pytest.mark.parametrize("name", G.NAMES)
def test_a_dropped_source_fails_measure_1(oracle, name, monkeypatch):
    """The block with the most sources, the source whose contribution -sum_i R[i, B]' R[i, A] (i over the rows of the child's
    subtree) is smallest in norm, left out of the parent's sum: the float64 factor of that matrix, presented as a
    backend, is at least 10 bounds off in measure (1) — a condition on the inputs."""
    case, tree, cls, plan = _facts(name, monkeypatch)
    _, judge = _oracle_case(oracle, case)
    S = judge.sys
    H, g = S.H.astype(np.float64), S.g.astype(np.float64)
    R, d = _factor(H, g)
    good = _DenseFactor(tree, S.off, R, d)
    x = np.linalg.solve(R, d)
    f0, r0, s0 = judge.backward(good, x, 0.0, False)
    assert f0 <= judge.kf and r0 <= judge.kf and s0 <= judge.ks, (f0, r0, s0)
    blocks = {}
    for s in plan.segments:
        if s.var_row >= 0:
            blocks.setdefault((s.front, s.var_row, s.var_col), []).extend(c for c, _ in s.sources)
    (front, vb, va), srcs = max(blocks.items(), key=lambda kv: len(kv[1]))
    B, A_ = good.scalars([vb]), good.scalars([va])
    kids = [[] for _ in tree[0]]
    for c, p in enumerate(tree[0]):
        if p >= 0:
            kids[p].append(c)

    def rows_of(c):
        out = list(good.scalars(tree[1][c][0]))
        for k in kids[c]:
            out += rows_of(k)
        return out

    contrib = []
    for c in srcs:
        rows = rows_of(c)
        contrib.append(-np.dot(R[np.ix_(rows, B)].T, R[np.ix_(rows, A_)]))
    k = int(np.argmin([np.linalg.norm(c) for c in contrib]))
    Hm = H.copy()
    Hm[np.ix_(B, A_)] -= contrib[k]
    if vb != va:
        Hm[np.ix_(A_, B)] -= contrib[k].T
    Rm, dm = _factor(Hm, g)
    f, r, s = judge.backward(_DenseFactor(tree, S.off, Rm, dm), np.linalg.solve(Rm, dm), 0.0, False)
    MUTATION_RATIOS[name] = f / judge.kf
    print(f"{name}: block ({vb}, {va}) of front {front}, {len(srcs)} sources, source {srcs[k]} of norm "
          f"{np.linalg.norm(contrib[k]):.3g} dropped: factor {f:.3g}u = {f / judge.kf:.3g} k (unmutated {f0:.2f}u, k {judge.kf})")
    assert f >= 10 * judge.kf
