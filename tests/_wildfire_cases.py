"""Hand-shaped graphs for the partial ("wildfire") back-substitution, and its restatement in numpy.longdouble
(test_host_wildfire_cases.py pins the cases on the CPU oracle, test_gpu_wildfire_classes.py judges the device on them).

A case is a three-storey Bayes tree under the natural ordering and amalgamation (0.0, 128), drawn as
_linear_cases.two_clique_arrays draws its graphs (vector variables of 1-8 dimensions, a unary JacobianFactor per variable,
two-row JacobianFactors between the variables of a clique and its separator, seeded):

    root  = {r0, r1, s}                      r0, r1, s 3-vectors, mutually adjacent
    M_i | r0                                 the middle clique of arm i: FM scalars, separator r0 (3 rows)
    A_i | first `sep` scalars of M_i         the bottom clique of arm i: FA scalars
    P_j | r0                                 padding: one-variable leaf cliques of 1 or 3 scalars

s carries the only nonlinear factor, a PriorFactor, and is coupled by JacobianFactors to r0 and r1 only: marking s in
gsx_relinearize_partial re-linearizes that prior and the two couplings, whose variables are all frontal in the root —
the root alone is re-eliminated and only its d moves.  A mixed F_LINEAR / F_PRIOR graph goes through
NonlinearFactorGraph.to_arrays(values) and is accepted by the oracle and by the product (test_host_wildfire_cases.py).
The padding makes 20 fronts or more, so that one dirty front is under both limits of gsx_relinearize_partial_impl.

Arms come in three kinds, set by the scale of their coupling factors (the whole factor, rows and right-hand side, is
multiplied: the cross term of the information matrix goes with the square):
    a  strong / strong     M_i and A_i change far above the threshold: solved and kept
    b  strong / EPS_B      M_i kept; A_i solved and restored
    c  EPS_C / strong      M_i solved and restored; A_i skipped
and the padding leaves take strong, EPS_C, EPS_B in turn.  steps(name) is the sequence of (move of s, threshold) on one
handle (MOVES; THRESHOLDS per case):
    1  a move of order 1: the kinds as above
    2  a further move with a threshold about 1e-6 of the first: the c arms' M_i now cross it (their stale values differ
       from the new ones by EPS_C^2 of a strong change) and their A_i are solved for the first time; the b arms' A_i
       (EPS_B^2: the rounding of the solve) still are restored
    3  a move of 1e-7 with the first threshold: every clique under the root is solved and restored, everything below is
       skipped — the variables marked changed in step 2 must not be seen as changed again, and the restored words are
       those of step 2, not of step 1 (the root's own change is below the threshold here on purpose: it is kept because
       it was re-eliminated)
Every solved clique's change is at least 100 thresholds or at most a hundredth of one (the host test asserts this on the
oracle; it is a condition of the inputs, so that float64 rounding on the device cannot flip a decision).

In the BOTTOM position (A_i is the clique under test) all three outcomes occur for its shape.  In the MIDDLE position
(M_i) only kept and restored do: a child of the re-eliminated root is always visited, because the root's frontal
variables count as changed whatever they did (ISAM2Clique.cpp:237-259); the skipped clique of such a case is A_i.  A
childless clique of at most 16 scalars is a leaf-kernel clique, so the leaf kernels are reached in the bottom position
only and a middle clique is LDS-class or blocked.

kernel_of() states the level plan of the back-substitution (upload.hip: plan_backsolve, which dev_backsolve_levels walks)
per clique from the tree, the front classes and the sizes; test_host_backsolve_plan.py holds it to the library's own plan
on every case here.  Branches of it that no tree reaches on the level path:
    generic backsolve_kernel with 64 threads   needs LDS-class cliques of at most 48 rows that backsolve_small_fits
                                               refuses; it refuses only F > 64 (n <= 140 holds for the class), so n > 65
    backsolve_big_kernel at F = 193            backsolve_big_lds refuses more than 192 frontal columns (kMaxChunk): F = 193
                                               is the 1024-thread generic kernel's case; the blocked kernel's is F = 192
"""
from collections import namedtuple

import numpy as np

from gtsam_petercdev_amd.graph import (JacobianFactor, NonlinearFactorGraph, PriorFactor, Values, noiseModel)
from tests._linear_cases import _split_dims

LD = np.longdouble
AMALGAMATION = (0.0, 128)
RELAXED = (0.5, 64)
EPS_B, EPS_C = 1e-7, 4e-4
# the moves of s, each added to its current value
MOVES = [np.array([1.0, -0.7, 0.5]), np.array([2.0, -2.5, 3.0]), np.array([1e-7, -1e-7, 1e-7])]

Arm = namedtuple("Arm", "fa fm sep kinds")
# name -> (arms, padding leaves, position of the clique under test, its shapes (F, separator rows))
CASES = {
    "pack16_wave6": ([Arm(3, 12, 12, "abc"), Arm(6, 12, 12, "abc"), Arm(3, 64, 64, "abc")], 8, "bottom", [(3, 12), (6, 12), (3, 64)]),
    "pack32_65": ([Arm(3, 65, 65, "abc"), Arm(5, 65, 65, "abc")], 8, "bottom", [(3, 65), (5, 65)]),
    "pack32_128": ([Arm(5, 128, 128, "abc")], 14, "bottom", [(5, 128)]),
    "wave16": ([Arm(16, 12, 12, "abc"), Arm(3, 12, 12, "abc")], 8, "bottom", [(16, 12), (3, 12)]),
    "tail129": ([Arm(3, 129, 129, "abc")], 14, "bottom", [(3, 129)]),
    "small": ([Arm(17, 5, 5, "abc"), Arm(32, 5, 5, "abc")], 8, "bottom", [(17, 5), (32, 5)]),
    "small2": ([Arm(33, 5, 5, "abc"), Arm(64, 5, 5, "abc")], 14, "bottom", [(33, 5), (64, 5)]),
    "generic256": ([Arm(65, 5, 5, "abc")], 14, "bottom", [(65, 5)]),
    "big192": ([Arm(192, 5, 5, "abc")], 14, "bottom", [(192, 5)]),
    "generic1024": ([Arm(193, 5, 5, "abc")], 14, "bottom", [(193, 5)]),
    "combined1024": ([Arm(65, 5, 5, "abc"), Arm(193, 5, 5, "ac")], 10, "bottom", [(65, 5), (193, 5)]),
    "middle_small2": ([Arm(3, 33, 12, "abc"), Arm(3, 64, 12, "abc")], 8, "middle", [(33, 3), (64, 3)]),
    "middle_big192": ([Arm(3, 192, 12, "abc")], 14, "middle", [(192, 3)]),
    "middle_generic1024": ([Arm(3, 193, 12, "abc")], 14, "middle", [(193, 3)]),
}
# the kernel each case is aimed at, for its target shapes (kernel_of's names)
INTENDED = {
    "pack16_wave6": {(3, 12): "leaf16", (6, 12): "leaf64", (3, 64): "leaf16"},
    "pack32_65": {(3, 65): "leaf32", (5, 65): "leaf32"},
    "pack32_128": {(5, 128): "leaf32"},
    "wave16": {(16, 12): "leaf64", (3, 12): "leaf64"},
    "tail129": {(3, 129): "leaf_tail"},
    "small": {(17, 5): "small", (32, 5): "small"},
    "small2": {(33, 5): "small2", (64, 5): "small2"},
    "generic256": {(65, 5): "generic256"},
    "big192": {(192, 5): "big"},
    "generic1024": {(193, 5): "generic1024"},
    "combined1024": {(65, 5): "combined1024", (193, 5): "combined1024"},
    "middle_small2": {(33, 3): "small2", (64, 3): "small2"},
    "middle_big192": {(192, 3): "big"},
    "middle_generic1024": {(193, 3): "generic1024"},
}
# (threshold of steps 1 and 3, threshold of step 2) per case, chosen on the CPU oracle: the middle (geometric mean) of the
# widest gap between the changes of the cliques the step solves — test_host_wildfire_cases.py asserts the margin of 100
THRESHOLDS = {
    "pack16_wave6": (2.8e-06, 3.9e-13),
    "pack32_65": (3e-06, 1.9e-12),
    "pack32_128": (3.5e-07, 6.2e-13),
    "wave16": (4.3e-06, 2.7e-12),
    "tail129": (1.2e-06, 5.1e-13),
    "small": (4e-06, 1e-12),
    "small2": (1.1e-06, 8.6e-13),
    "generic256": (5.8e-06, 1.2e-12),
    "big192": (2.6e-06, 5.2e-13),
    "generic1024": (4.6e-06, 1.4e-12),
    "combined1024": (1.4e-06, 8.1e-13),
    "middle_small2": (4.8e-07, 2e-13),
    "middle_big192": (4.4e-07, 1.3e-13),
    "middle_generic1024": (8.9e-07, 3e-13),
}
# under RELAXED amalgamation small2 keeps three storeys in its (64, 5) arms and merges the (33, 5) ones; pack16_wave6 becomes
# two storeys of merged fronts (an A_i of at most 16 scalars joins its M_i): visited, kept or restored as a whole
RELAXED_CASES = ["pack16_wave6", "small2"]
# every branch of the level plan's dispatch (plan_backsolve) that a tree can reach (module docstring: the others)
BRANCHES = {"leaf16", "leaf32", "leaf64", "leaf_tail", "small", "small2", "generic256", "generic1024", "combined1024", "big"}

Case = namedtuple("Case", "name arr ordering s_var arms pads root position shapes")
BuiltArm = namedtuple("BuiltArm", "kind a_vars m_vars fa fm sep")
_BUILT = {}


def build(name):
    """The case's arrays (values: zeros, s at its prior's neighbourhood), the natural ordering, the variable of s, and
    which variables make which clique.  Built once a process and shared: nobody writes to it."""
    if name in _BUILT:
        return _BUILT[name]
    arms, n_pad, position, shapes = CASES[name]
    rng = np.random.default_rng(4200 + sorted(CASES).index(name))
    dims, built = [], []
    flat = [(arm, kind) for arm in arms for kind in arm.kinds]
    a_lists, m_lists = [], []
    for arm, _ in flat:                                    # the bottom cliques first
        d = _split_dims(arm.fa, rng)
        a_lists.append(list(range(len(dims), len(dims) + len(d))))
        dims += d
    pads = list(range(len(dims), len(dims) + n_pad))
    dims += [1 if j % 2 else 3 for j in range(n_pad)]
    n_sep_vars = []
    for arm, _ in flat:                                    # the middle cliques: the bottom clique's separator is a prefix
        d_sep = _split_dims(arm.sep, rng)
        d = d_sep + _split_dims(arm.fm - arm.sep, rng)
        m_lists.append(list(range(len(dims), len(dims) + len(d))))
        n_sep_vars.append(len(d_sep))
        dims += d
    r0, r1, s = len(dims), len(dims) + 1, len(dims) + 2
    dims += [3, 3, 3]
    g = NonlinearFactorGraph()
    for k, d in enumerate(dims[:-1]):
        g.add(JacobianFactor(k, np.eye(d) * (0.7 + rng.random()), rng.normal(size=d), noiseModel.Isotropic.Sigma(d, 1.5)))
    g.add(PriorFactor(s, rng.normal(size=3), noiseModel.Diagonal.Sigmas(np.array([0.3, 0.4, 0.5]))))

    def pair(a, b, w=1.0, sd=0.3):
        g.add(JacobianFactor(a, w * rng.normal(0, sd, (2, dims[a])), b, w * rng.normal(0, sd, (2, dims[b])),
                             w * rng.normal(size=2), noiseModel.Unit.Create(2)))

    for (arm, kind), av, mv, ns in zip(flat, a_lists, m_lists, n_sep_vars):
        w_am = EPS_B if kind == "b" else 1.0
        w_mr = EPS_C if kind == "c" else 1.0
        for i, a in enumerate(av):
            for b in av[i + 1:]:
                pair(a, b)
            for b in mv[:ns]:
                pair(a, b, w_am)
        for i, a in enumerate(mv):
            for b in mv[i + 1:]:
                pair(a, b)
            pair(a, r0, w_mr)
        built.append(BuiltArm(kind, av, mv, arm.fa, arm.fm, arm.sep))
    for j, p in enumerate(pads):
        pair(p, r0, (1.0, EPS_C, EPS_B)[j % 3])
    pair(r0, r1, sd=0.6)
    pair(r0, s, sd=0.6)
    pair(r1, s, sd=0.6)
    values = Values()
    for k, d in enumerate(dims):
        values.insert(k, np.zeros(d))
    arr = g.to_arrays(values)
    _BUILT[name] = Case(name, arr, list(range(len(dims))), s, built, pads, [r0, r1, s], position, shapes)
    return _BUILT[name]


def steps(name):
    """[(move of s, threshold)] of the case: steps 1 and 2 with the case's own thresholds, step 3 with the first again."""
    t1, t2 = THRESHOLDS[name]
    return [(MOVES[0], t1), (MOVES[1], t2), (MOVES[2], t1)]


def state_offsets(arr):
    return np.concatenate([[0], np.cumsum(arr.state_dims())]).astype(np.int64)


def moved_values(case, values, move):
    """(a copy of the packed values with s moved by `move`, the new state of s)."""
    off = state_offsets(case.arr)
    out = np.array(values, dtype=np.float64)
    out[off[case.s_var]:off[case.s_var + 1]] += move
    return out, out[off[case.s_var]:off[case.s_var + 1]].copy()


# ---- the traversal ------------------------------------------------------------------------------------------------------------
SKIPPED, RESTORED, KEPT = "skipped", "restored", "kept"
Wildfire = namedtuple("Wildfire", "outcome delta count change solution")


def scalars_of(dims, vs):
    toff = np.concatenate([[0], np.cumsum(dims)]).astype(np.int64)
    return np.concatenate([np.arange(toff[v], toff[v + 1]) for v in vs]) if len(vs) else np.zeros(0, np.int64)


def back_substitute(R, rhs):
    """R x = rhs, R upper triangular, in the precision of the operands."""
    n = rhs.size
    x = np.zeros(n, rhs.dtype)
    for i in range(n - 1, -1, -1):
        x[i] = (rhs[i] - np.dot(R[i, i + 1:], x[i + 1:])) / R[i, i]
    return x


def wildfire_restatement(parent, fronts, conditional, dims, delta, replaced, threshold):
    """optimizeWildfireNonRecursive (gtsam/nonlinear/ISAM2Clique.cpp:261-287; isDirty :68-90, valuesChanged :175-183,
    restoreFromOriginals :193-201) — test_gpu_wildfire.py's restatement carried in longdouble.  Cliques are (frontal
    variables, separator variables), conditional(c) = [R S d], `replaced` the set of re-eliminated cliques, `delta` the
    previous solution.  Returns per clique one of skipped (never solved: clean, or under a clean clique) / restored /
    kept, the new delta (longdouble), the number of frontal variables solved, per solved clique the max-norm change of
    its frontal values, and per solved clique the longdouble solution before any restore."""
    children = [[] for _ in parent]
    roots = []
    for c, p in enumerate(parent):
        (children[p] if p >= 0 else roots).append(c)
    delta = np.asarray(delta, dtype=LD).copy()
    outcome = [SKIPPED] * len(parent)
    change, solution = {}, {}
    changed = set()
    count = 0
    stack = list(roots)
    while stack:
        c = stack.pop()
        fv, sv = fronts[c]
        if not ((c in replaced) or any(v in changed for v in sv)):     # ISAM2Clique::isDirty
            continue
        fi, si = scalars_of(dims, fv), scalars_of(dims, sv)
        RSd = np.asarray(conditional(c), dtype=np.float64).astype(LD)
        nf = fi.size
        orig = delta[fi].copy()
        sol = back_substitute(RSd[:, :nf], RSd[:, -1] - np.dot(RSd[:, nf:nf + si.size], delta[si]))
        count += len(fv)
        change[c] = float(np.max(np.abs(orig - sol)))
        solution[c] = sol
        if (c in replaced) or change[c] >= threshold:                   # valuesChanged
            delta[fi] = sol
            changed.update(fv)
            outcome[c] = KEPT
        else:                                                           # restoreFromOriginals
            outcome[c] = RESTORED
        stack.extend(children[c])
    return Wildfire(outcome, delta, count, change, solution)


def worst_margin(wf, replaced, threshold):
    """The margin condition: min over the solved cliques of max(change / threshold, threshold / change) — at least 100 in
    every case; the re-eliminated cliques are kept whatever they did and are left out."""
    m = float("inf")
    for c, ch in wf.change.items():
        if c not in replaced:
            m = min(m, ch / threshold if ch >= threshold else (threshold / ch if ch > 0 else float("inf")))
    return m


# ---- which kernel a clique runs in on the level path ------------------------------------------------------------------------
def levels_of(parent):
    """Height from the leaves (symbolic.cpp: children have smaller ids)."""
    lvl = [0] * len(parent)
    for c, p in enumerate(parent):
        assert p < 0 or p > c
        if p >= 0:
            lvl[p] = max(lvl[p], lvl[c] + 1)
    return lvl


def clique_shapes(fronts, dims):
    return [(int(sum(dims[v] for v in f)), int(sum(dims[v] for v in s))) for f, s in fronts]


def kernel_of(parent, fronts, classes, dims, big_lds, packed=True):
    """The level plan of the back-substitution (upload.hip: plan_backsolve; compared with the library's own by
    test_host_backsolve_plan.py): per clique the name of the kernel that back-substitutes it, from gsx_get_tree's sizes
    and gsx_get_front_classes (bits 0-1: 0 leaf kernel, 1 LDS, 2 blocked).  big_lds(max n, max F, max separator rows + 1) is bigfront.hip's backsolve_big_lds (gsxtest_backsolve_big_lds); packed = a handle made without
    GSX_BS_LEAF_PACK=0 (kernels.hip: leaf_pack_class)."""
    shp = clique_shapes(fronts, dims)
    lvl = levels_of(parent)
    cls = [int(c) & 3 for c in classes]
    N = [f + s + 1 for f, s in shp]
    out = [None] * len(parent)
    for l in range(max(lvl) + 1):
        ids = [c for c in range(len(parent)) if lvl[c] == l]
        leaf = [c for c in ids if cls[c] == 0]
        small = [c for c in ids if cls[c] == 1]
        big = [c for c in ids if cls[c] == 2]
        assert len(leaf) + len(small) + len(big) == len(ids), "a medium front: GSX_MEDIUM is not for these cases"
        assert not leaf or l == 0
        if leaf:
            max_f = max(shp[c][0] for c in leaf)
            for c in leaf:
                F, sep = shp[c]
                if packed and max_f <= 8 and sep <= 64 and F * F <= 16:
                    out[c] = "leaf16"
                elif packed and max_f <= 8 and sep <= 128 and F * F <= 32:
                    out[c] = "leaf32"
                else:
                    out[c] = "leaf64" if sep <= 128 else "leaf_tail"
        big_own = bool(big) and big_lds(max(N[c] for c in big), max(shp[c][0] for c in big), max(N[c] - shp[c][0] for c in big)) > 0
        small_own = False
        if small:
            mn, mf = max(N[c] for c in small), max(shp[c][0] for c in small)
            small_own = mf <= 64 and mn <= 140 and mn - 2 <= 144
            if small_own:
                for c in small:
                    out[c] = "small" if mf <= 32 else "small2"
        for c in big if big_own else []:
            out[c] = "big"
        big_left, small_left = bool(big) and not big_own, bool(small) and not small_own
        n_rest = len(small) + len(big)
        if big_left and small_left and n_rest <= 512 and n_rest > len(big):
            for c in small + big:
                out[c] = "combined1024"
        else:
            for c in big if big_left else []:
                out[c] = "generic1024"
            for c in small if small_left else []:
                out[c] = "generic64" if max(N[k] for k in small) <= 48 else "generic256"
    assert all(out), out
    return out


def target_cliques(case, fronts):
    """{clique id: (arm kind, shape)} of the cliques under test, found by their frontal variables."""
    by_first = {f[0]: c for c, (f, _) in enumerate(fronts)}
    out = {}
    for arm in case.arms:
        vs = arm.a_vars if case.position == "bottom" else arm.m_vars
        out[by_first[vs[0]]] = (arm.kind, (arm.fa, arm.sep) if case.position == "bottom" else (arm.fm, 3))
    return out
