"""Hand-built linear graphs whose hard-constraint rows are handed from one clique to another with DIFFERENT supports, the
structure each is meant to have (checked against get_tree on the host), and the judge: the dense KKT system of the
constrained least-squares problem solved with mpmath at 50 digits.

What the cases are about.  A clique that takes in more constraint rows than it has frontal scalars hands the excess on
(csrc/symbolic.cpp plans it, csrc/constraint.hip does it).  The excess rows of TWO frontal variables a and b of one clique,
written on (a, x) and on (b, y), leave as one row on {x} and one on {y}: they share no variable.  Both travel to x's
clique; the {y} row is zero in x's columns, finds no pivot there and must be handed on again (Constrained::QR leaves a row
without an entry in the column alone, NoiseModel.cpp:566-590).

Every coefficient is a multiple of 1/4 of magnitude at most 2, every soft sigma is 1 or 1/2: [A b] is exact in float64
and the 50-digit solution is the solution of exactly the system the device is given.  Every variable has a unit prior, so
the soft Hessian is positive definite on its own."""
from __future__ import annotations

import functools

import mpmath as mp
import numpy as np

from gtsam_petercdev_amd import _abi as A
from gtsam_petercdev_amd.graph import GaussianFactorGraph, JacobianFactor, noiseModel

DPS = 50
# (lambda, diagonal damping): LM's two damping forms and the undamped step
DAMPINGS = [(0.0, False), (0.3, False), (0.1, True)]


class _Coefficients:
    """A fixed sequence of quarters in [-2, 2] without zeros: a multiplicative congruence mod 17 walks through all of
    1..16, which are mapped to +-1/4 .. +-2.  `variant` starts the walk elsewhere (other numbers, same structure)."""

    def __init__(self, variant=0):
        self.s = 1 + (5 * variant) % 16
        self.k = 0

    def next(self):
        self.s = (self.s * 3) % 17           # 3 is a primitive root mod 17
        self.k += 1
        if self.k % 16 == 0:                 # (the walk has period 16: shift it, so that blocks do not repeat)
            self.s = self.s % 16 + 1
        v = self.s                           # 1..16
        return (v if v <= 8 else 8 - v) / 4.0

    def block(self, m, d):
        return np.array([[self.next() for _ in range(d)] for _ in range(m)])

    def vector(self, m):
        return np.array([self.next() for _ in range(m)])


class Case:
    """name; variables [(name, dim)] (the key of a variable is its index in this list); the elimination order; soft binary
    factors [(u, v, rows)]; constraint factors [(names, rows)]; `roles`: what the structure check asserts —
      fronts: {label: frontal names} that must be fronts of the tree exactly,
      path:   labels from a descendant up to an ancestor: distinct fronts on one root path, in this order,
      excess: labels of fronts that own more constraint rows than they have frontal scalars,
      between: labels of fronts on the path that own no constraint row."""

    def __init__(self, name, variables, order, soft, constraints, roles, variant=0):
        self.name, self.variables, self.order, self.soft, self.constraints, self.roles = (
            name, variables, order, soft, constraints, roles)
        self.variant = variant                # where this case's walk through the coefficients starts
        self.key = {v: i for i, (v, _) in enumerate(variables)}
        self.dim = dict(variables)
        self.amalgamation = (0.0, 16)         # the reference's Bayes tree: the cliques are natural supernodes

    def describe(self):
        r = self.roles
        lines = [f"{self.name}: order {' '.join(self.order)}"]
        for label, names in r["fronts"].items():
            lines.append(f"  front '{label}' has frontal variables {{{', '.join(names)}}}")
        if r.get("path"):
            lines.append("  on one root path, child to ancestor: " + " -> ".join(r["path"]))
        for label in r.get("excess", ()):
            lines.append(f"  front '{label}' owns more constraint rows than it has frontal scalars")
        for label in r.get("between", ()):
            lines.append(f"  front '{label}' owns no constraint row")
        return "\n".join(lines)

    def ordering(self):
        return np.array([self.key[v] for v in self.order], dtype=np.uint64)

    def graph(self, variant=0):
        """The GaussianFactorGraph: priors, soft binary factors, constraint factors — in this order."""
        c = _Coefficients(self.variant + variant)
        fg = GaussianFactorGraph()
        for v, d in self.variables:
            fg.add(JacobianFactor(self.key[v], np.eye(d), c.vector(d), noiseModel.Unit.Create(d)))
        for u, v, m in self.soft:
            fg.add(JacobianFactor(self.key[u], c.block(m, self.dim[u]), self.key[v], c.block(m, self.dim[v]), c.vector(m),
                                  noiseModel.Isotropic.Sigma(m, 0.5)))
        for i, (names, m) in enumerate(self.constraints):
            args = []
            for v in names:
                args += [self.key[v], c.block(m, self.dim[v])]
            fg.add(JacobianFactor(*args, c.vector(m), noiseModel.Constrained.All(m)))
        return fg

    def arrays(self, variant=0) -> A.ProblemArrays:
        arr = self.graph(variant).to_arrays(None)
        arr.values = np.zeros(int(arr.var_dims.sum()))
        return arr

    def n_constraint_rows(self):
        return sum(m for _, m in self.constraints)


def _two_supports(name, da, dx, rows, second="y", own=(), order=None, extra_vars=(), extra_soft=(), roles=None, variant=0):
    """One front {a, b}; `rows` constraint rows on (a, x) and `rows` on (b, `second`); x and y in different fronts, y's an
    ancestor of x's.  The soft edges make {b, x, y} the separator of a and {x, y} that of b, so a and b are one natural
    supernode (a clique joins its parent when its separator is the parent's whole clique).  x also sees r, which b does
    not, and y also sees s, which x does not: neither b and x nor x and y are one supernode; {y, r, s} is the root."""
    variables = [("a", da), ("b", da), ("x", dx), ("y", dx), ("r", 1), ("s", 1)] + list(extra_vars)
    soft = [("a", "b", 1), ("a", "y", 1), ("b", "x", 1), ("x", "y", 2), ("x", "r", 1), ("y", "s", 1), ("r", "s", 1)]
    constraints = [(("a", "x"), rows), (("b", second), rows)] + list(own)
    roles = roles or {"fronts": {"ab": ["a", "b"], "x": ["x"], "y": ["y", "r", "s"]}, "path": ["ab", "x", "y"],
                      "excess": ["ab"]}
    return Case(name, variables, order or ["a", "b", "x", "y", "r", "s"], soft + list(extra_soft), constraints, roles,
                variant=variant)


def _cases():
    out = []
    # the minimal shape: leftovers {x} and {y} from one front, dim(x) = 2 pivots on offer at x
    out.append(_two_supports("two_supports", 1, 2, 2))
    # more than dim rows on two frontal variables of one clique, wider variables
    out.append(_two_supports("two_supports_wide", 2, 3, 3))
    # an unconstrained front z between x's front and y's: the {y} row leaves x's front for y's and never meets z
    # (each clique of the chain sees one variable its child does not: x sees r, z sees s, y sees t)
    out.append(_two_supports(
        "skips_a_level", 1, 2, 2, order=["a", "b", "x", "z", "y", "r", "s", "t"], extra_vars=[("z", 2), ("t", 1)],
        extra_soft=[("x", "z", 1), ("z", "y", 2), ("z", "s", 1), ("y", "t", 1)],
        roles={"fronts": {"ab": ["a", "b"], "x": ["x"], "z": ["z"], "y": ["y", "r", "s", "t"]},
               "path": ["ab", "x", "z", "y"], "between": ["z"], "excess": ["ab"]}))
    # leftovers {x}, {y} and {x, y} from one front {a, b, c}; dim(x) = 3 offers a pivot to each of the three
    out.append(Case(
        "three_supports", [("a", 1), ("b", 1), ("c", 1), ("x", 3), ("y", 2), ("r", 1), ("s", 1)],
        ["a", "b", "c", "x", "y", "r", "s"],
        [("a", "b", 1), ("a", "c", 1), ("a", "y", 1), ("b", "c", 1), ("b", "x", 1), ("x", "y", 2), ("x", "r", 1),
         ("y", "s", 1), ("r", "s", 1)],
        [(("a", "x"), 2), (("b", "y"), 2), (("c", "x", "y"), 2)],
        {"fronts": {"ab": ["a", "b", "c"], "x": ["x"], "y": ["y", "r", "s"]}, "path": ["ab", "x", "y"], "excess": ["ab"]}))
    # x's front has a constraint row of its own on (x, y): with the arriving {x} row that is two pivots of dim(x) = 3
    out.append(_two_supports("meets_own_rows", 1, 3, 2, own=[(("x", "y"), 1)]))
    # control: both leftovers on {x} — the union of the supports is each row's support
    out.append(_two_supports("same_support", 1, 3, 2, second="x"))
    # two constrained leaves {a | x} and {b | y} hand one row each, on {x} and on {y}, to the same parent {x, y, r}
    out.append(Case(
        "two_children", [("a", 1), ("b", 1), ("x", 2), ("y", 2), ("r", 1)], ["a", "b", "x", "y", "r"],
        [("a", "x", 1), ("b", "y", 1), ("x", "y", 2), ("x", "r", 1), ("y", "r", 1)],
        [(("a", "x"), 2), (("b", "y"), 2)],
        {"fronts": {"a": ["a"], "b": ["b"], "y": ["x", "y", "r"]}, "children": [("a", "y"), ("b", "y")],
         "excess": ["a", "b"]}))
    return {c.name: c for c in out}


def _padded(name, base_order, base_vars=(), base_soft=(), roles=None, pads=20):
    """A two-supports case with `pads` scalar leaves p0, p1, ... hung on r.  gsx_relinearize_partial takes the full path
    when more than 15 % of the fronts are dirty (csrc/incremental.hip); with the leaves, re-eliminating the root alone stays
    below that and goes through the partial path, the fronts below it clean."""
    ps = [f"p{i}" for i in range(pads)]
    return _two_supports(name, 1, 2, 2, order=ps + base_order, extra_vars=list(base_vars) + [(p, 1) for p in ps],
                         extra_soft=list(base_soft) + [(p, "r", 1) for p in ps], roles=roles)


CASES = _cases()
# the same shapes inside a tree of two dozen fronts, for the partial re-elimination test only
PADDED = {c.name: c for c in [
    _padded("two_supports_padded", ["a", "b", "x", "y", "r", "s"]),
    _padded("skips_a_level_padded", ["a", "b", "x", "z", "y", "r", "s", "t"], [("z", 2), ("t", 1)],
            [("x", "z", 1), ("z", "y", 2), ("z", "s", 1), ("y", "t", 1)],
            {"fronts": {"ab": ["a", "b"], "x": ["x"], "z": ["z"], "y": ["y", "r", "s", "t"]},
             "path": ["ab", "x", "z", "y"], "between": ["z"], "excess": ["ab"]})]}
ALL = {**CASES, **PADDED}
# the cases with two fronts x and y on one root path (the hand-over from x's front to y's is what they are about)
PATH_CASES = [n for n, c in CASES.items() if c.roles.get("path")]



def vanishing_row_case():
    """two_supports with a constraint row that says 0 = d: the second row of the factor on (a, x) is zero in the frontal
    variable a AND in the separator variable x, its right-hand side is not.  Returns (case, arrays, (factor, row))."""
    c = _two_supports("vanishing_row", 1, 2, 2)
    fg = c.graph()
    fi = len(c.variables) + len(c.soft)      # the constraint factor on (a, x)
    f = fg.factors[fi]
    Ab = f.meas.reshape(-1, f.rows).T.copy()
    Ab[1, :-1] = 0.0
    assert Ab[1, -1] != 0.0
    f.meas = Ab.reshape(-1, order="F")
    arr = fg.to_arrays(None)
    arr.values = np.zeros(int(arr.var_dims.sum()))
    return c, arr, (fi, 1)


# ---- the structure check -------------------------------------------------------------------------------------------------
def constraint_rows(arr: A.ProblemArrays):
    """(factor, row) of every zero-sigma row."""
    out = []
    for f in range(arr.n_factors):
        if arr.f_noise_kind[f] not in (A.NOISE_DIAGONAL, A.NOISE_CONSTRAINED):
            continue
        par = arr.noise[arr.f_noise_ptr[f]:arr.f_noise_ptr[f + 1]]
        out += [(f, r) for r in range(arr.f_rows[f]) if par[r] == 0.0]
    return out


def check_structure(case: Case, arr: A.ProblemArrays, tree):
    """Asserts that the tree the library built for the case's ordering is the one the case declares.  tree = get_tree()."""
    parent, fronts = tree
    roles = case.roles
    name_of = {i: v for v, i in case.key.items()}
    frontal = [sorted(name_of[v] for v in fv) for fv, _ in fronts]
    front_of = {}
    for label, names in roles["fronts"].items():
        assert sorted(names) in frontal, (case.name, label, names, frontal)
        front_of[label] = frontal.index(sorted(names))
    assert len(set(front_of.values())) == len(front_of)

    def ancestors(c):
        out = []
        while parent[c] >= 0:
            c = parent[c]
            out.append(c)
        return out

    path = roles.get("path", [])
    for lo, hi in zip(path, path[1:]):   # distinct fronts, each the PARENT of the one before: one root path, nothing between
        assert parent[front_of[lo]] == front_of[hi], (case.name, lo, hi, parent, frontal)
    if path:   # x and y in distinct fronts, y's an ancestor of x's
        assert front_of["y"] in ancestors(front_of["x"]) and front_of["x"] != front_of["y"]
    for lo, hi in roles.get("children", []):
        assert parent[front_of[lo]] == front_of[hi], (case.name, lo, hi, parent, frontal)
    # the constraint rows a front owns: those whose first variable in the ordering is frontal there
    pos = {int(k): i for i, k in enumerate(case.ordering())}
    holder = {v: c for c, (fv, _) in enumerate(fronts) for v in fv}
    own = np.zeros(len(fronts), int)
    for f, _ in constraint_rows(arr):
        vs = arr.f_vars[arr.f_key_ptr[f]:arr.f_key_ptr[f + 1]]
        own[holder[min(vs, key=lambda v: pos[int(arr.var_keys[v])])]] += 1
    for label in roles.get("excess", []):
        c = front_of[label]
        scalars = sum(case.dim[name_of[v]] for v in fronts[c][0])
        assert own[c] > scalars, (case.name, label, int(own[c]), scalars)
    for label in roles.get("between", []):
        assert own[front_of[label]] == 0, (case.name, label)
    return front_of


# ---- [A b] as the case states it, and the judge ------------------------------------------------------------------------------
def stated_jacobians(arr: A.ProblemArrays) -> np.ndarray:
    """[A b] of every factor, column-major one factor after the other, as the oracle returns it: a soft row divided by its
    sigma (1 or 1/2: exact), a constraint row as it is."""
    out = []
    for f in range(arr.n_factors):
        m = arr.f_rows[f]
        Ab = arr.meas[arr.f_meas_ptr[f]:arr.f_meas_ptr[f + 1]].reshape(-1, m).T.copy()
        kind = arr.f_noise_kind[f]
        par = arr.noise[arr.f_noise_ptr[f]:arr.f_noise_ptr[f + 1]]
        if kind == A.NOISE_ISOTROPIC:
            Ab /= par[0]
        else:
            assert kind in (A.NOISE_UNIT, A.NOISE_CONSTRAINED)
        out.append(Ab.reshape(-1, order="F"))
    return np.concatenate(out)


def dense_rows(arr: A.ProblemArrays, jac: np.ndarray, skip=()):
    """(soft rows, constraint rows) of the whole graph as dense (rows, n + 1) float64 arrays, the rhs last; without the
    (factor, row) pairs in `skip`."""
    n = int(arr.var_dims.sum())
    toff, joff = arr.tangent_offsets(), arr.jacobian_offsets()
    con = set(constraint_rows(arr))
    soft_rows, con_rows = [], []
    for f in range(arr.n_factors):
        m = arr.f_rows[f]
        vs = arr.f_vars[arr.f_key_ptr[f]:arr.f_key_ptr[f + 1]]
        cols = int(arr.var_dims[vs].sum()) + 1
        M = jac[joff[f]:joff[f] + m * cols].reshape(cols, m).T
        for r in range(m):
            if (f, r) in skip:
                continue
            row = np.zeros(n + 1)
            c = 0
            for v in vs:
                d = arr.var_dims[v]
                row[toff[v]:toff[v] + d] = M[r, c:c + d]
                c += d
            row[n] = M[r, c]
            (con_rows if (f, r) in con else soft_rows).append(row)
    return np.array(soft_rows), np.array(con_rows).reshape(-1, n + 1)


def hessian_diagonal(arr, jac):
    """diag(J'J) over ALL rows, a constraint row as it is (JacobianFactor::hessianDiagonalAdd) — what diagonal damping scales."""
    Sa, Cc = dense_rows(arr, jac)
    return (Sa[:, :-1] ** 2).sum(axis=0) + (Cc[:, :-1] ** 2).sum(axis=0)


def kkt_matrix(arr, jac, lam, damp):
    """The KKT matrix [[A'A + lam diag(damp), C'], [C, 0]] and its right-hand side in float64 (for rank and condition)."""
    Sa, Cc = dense_rows(arr, jac)
    n = Sa.shape[1] - 1
    k = Cc.shape[0]
    H = Sa[:, :n].T @ Sa[:, :n] + lam * np.diag(np.asarray(damp, float))
    return np.block([[H, Cc[:, :n].T], [Cc[:, :n], np.zeros((k, k))]]), np.concatenate([Sa[:, :n].T @ Sa[:, n], Cc[:, n]])


def kkt_step_mp(arr, jac, lam, damp, skip=()):
    """min 1/2 |A x - b|^2 + 1/2 lam x' diag(damp) x over the soft rows subject to the constraint rows C x = d (the statement
    of dense_kkt_step in tests/test_gpu_constraints.py), as one dense KKT system solved by LU at 50 digits.  jac: [A b] with
    the constraint rows unwhitened; skip: (factor, row) pairs left out.  Returns x as a list of mpf."""
    with mp.workdps(DPS):
        Sa, Cc = dense_rows(arr, jac, skip)
        n = Sa.shape[1] - 1
        k = Cc.shape[0]
        Am = mp.matrix(Sa[:, :n].tolist())
        bm = mp.matrix(Sa[:, n].tolist())
        K = mp.zeros(n + k, n + k)
        H = Am.T * Am
        g = Am.T * bm
        rhs = mp.zeros(n + k, 1)
        for i in range(n):
            for j in range(n):
                K[i, j] = H[i, j]
            K[i, i] += mp.mpf(float(lam)) * mp.mpf(float(damp[i]))
            rhs[i] = g[i]
        for r in range(k):
            for j in range(n):
                K[n + r, j] = K[j, n + r] = mp.mpf(float(Cc[r, j]))
            rhs[n + r] = mp.mpf(float(Cc[r, n]))
        sol = mp.lu_solve(K, rhs)
        # the residual of the 50-digit solve itself: far below anything float64 can show
        res = K * sol - rhs
        assert max(abs(res[i]) for i in range(n + k)) < mp.mpf(10) ** (-40)
        return [sol[i] for i in range(n)]


@functools.lru_cache(maxsize=None)
def reference(name, variant=0):
    """{(lam, diagonal): float64 array of the 50-digit step} of a case, computed once."""
    case = ALL[name]
    arr = case.arrays(variant)
    jac = stated_jacobians(arr)
    hd = hessian_diagonal(arr, jac)
    out = {}
    for lam, diag in DAMPINGS:
        x = kkt_step_mp(arr, jac, lam, hd if diag else np.ones_like(hd))
        out[(lam, diag)] = np.array([float(v) for v in x])
    for v in out.values():
        v.setflags(write=False)
    return out
