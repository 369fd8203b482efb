"""The partial ("wildfire") back-substitution judged clique by clique, outcome by outcome, in every kernel of the level
schedule it runs on (solver.hip: dev_backsolve_levels; kernels.h: wildfire_skip at the top of six kernels;
kernels.hip: wildfire_post_kernel after every level).  The cases are the hand-shaped trees of tests/_wildfire_cases.py
(pinned on the CPU by test_host_wildfire_cases.py): arms whose cliques are kept, restored and skipped side by side in
one launch — for the packed leaves in one wave — with the clique under test sized over the boundaries of the dispatch.

On one handle per case: linearize and solve; then three partial passes (move s, gsx_relinearize_partial — the root alone
is re-eliminated — gsx_backsubstitute_wildfire), each starting from the previous pass's result with its stale restored
and skipped cliques; then threshold 0 (everything: word for word a fresh handle's solve at the same values) and the
second threshold again with nothing moved (nothing solved, no word changed).  After each partial pass, with the
longdouble restatement run on the device's own conditionals and the device's own previous delta:
    count      the device's count of solved variables equals the restatement's
    untouched  the frontal words of every skipped and every restored clique equal the previous delta's bit for bit
    kept       |R x_F + S x_S - d| <= k u (|R||x_F| + |S||x_S| + |d|) componentwise in longdouble, x_S from the
               device's result, for every kept clique and the re-eliminated root.  k = _ld_linear.k_solve(m, n) with
               m = the separator's rows (the longest accumulation outside the triangle) and n = F: a row of the clique
               is an inner product of at most F + m terms, a subtraction and a multiplication by the reciprocal pivot,
               (F + m + 1) u by Higham Theorem 8.5 as k_solve's own derivation uses it; k = 2 (m + 3 F + 16) bounds it
               and is the figure the suite holds every other solve to.  A kept clique solved against a stale or
               half-written separator value is off by the separator's change, 1e9 u and more
    root       the re-eliminated factorization holds factor_ratio / rhs_ratio of a Judge built from the device's [A b]
               after the partial call
The margin condition (every change 100 thresholds away from its threshold) is re-asserted on the device's conditionals.
Each case runs once more on a handle made under GSX_BS_LEAF_PACK=0: same outcomes, same counts, same words.
Which kernel every clique ran in is stated from gsx_get_tree and gsx_get_front_classes (_wildfire_cases.kernel_of, which
test_host_backsolve_plan.py holds to the library's own launch plan — upload.hip: plan_backsolve — clique by clique)
and asserted; the last test asserts that every reachable branch of the dispatch saw all three outcomes (the
unreachable ones: _wildfire_cases' docstring).  It means something only when the whole module runs in one process.

These tests judge the results of one run each: they cannot show a race between a level's kernels and its post pass.

Measured on the MI355X, worst kept-clique residual in u (k in brackets is the smallest k the class was held to):
leaf16 1.0 (44), leaf32 0.62 (180), leaf64 1.1 (44), leaf_tail 0.74 (308), small 3.02 (68), small2 2.68 (110),
generic256 2.86 (146), generic1024 3.54 (1196), combined1024 2.96 (432), big 3.17 (1190); the re-eliminated
factorization: factor at most 8.8 u, rhs at most 3.6 u against k of 800 to 1900.  Every count was exact and every
untouched clique bit-equal; the whole module takes under five seconds.
"""
import numpy as np
import pytest

from tests import _ld_linear as J
from tests import _wildfire_cases as W
from tests._switches import switches

pytestmark = pytest.mark.gpu

LD = J.LD
SEEN = {}          # kernel -> outcomes of the cliques under test that ran in it (default handles, reference cliques)
SEEN_RELAXED = {}  # the same over all cliques of the relaxed trees
WORST = {}         # kernel -> (worst kept residual in u, smallest k)


@pytest.fixture(scope="module")
def gpu():
    from gtsam_petercdev_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the HIP path has no fallback"
    return _lib


@pytest.fixture(scope="module")
def big_lds(gpu):
    import ctypes as C
    f = gpu.load().gsxtest_backsolve_big_lds
    f.restype = C.c_longlong
    f.argtypes = [C.c_int, C.c_int, C.c_int]
    return f


def _handle(gpu, case, amalgamation, packed=True):
    """A handle under the case's ordering; packed=False: made under GSX_BS_LEAF_PACK=0 (read when a handle is created)."""
    with switches(**({} if packed else {"GSX_BS_LEAF_PACK": "0"})):
        gb = gpu.product_backend(case.arr)
    gb.set_amalgamation(*amalgamation)
    gb.set_ordering(case.arr.var_keys[case.ordering])
    return gb


def _words(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _kept_ratio(RSd, x, fi, si):
    """max |R x_F + S x_S - d| / (u (|R||x_F| + |S||x_S| + |d|)) of one clique, in longdouble."""
    W_ = np.asarray(RSd, dtype=np.float64).astype(LD)
    xx = np.concatenate([x[fi], x[si]]).astype(LD)
    res = np.dot(W_[:, :-1], xx) - W_[:, -1]
    bound = np.dot(np.abs(W_[:, :-1]), np.abs(xx)) + np.abs(W_[:, -1])
    return J._ratio(res, bound)


def _sequence(gpu, case, gb, kern, what, judge):
    """The passes on one handle.  Returns [(outcome map, count, words)] of the partial passes + the two closing ones, and
    fills WORST (judge=True).  Every pass is judged against the restatement on THIS handle's conditionals."""
    arr = case.arr
    dims = [int(d) for d in arr.var_dims]
    parent, fronts = gb.get_tree()
    parent, fronts = [int(p) for p in parent], [(list(f), list(s)) for f, s in fronts]
    replaced = {c for c, (f, _) in enumerate(fronts) if case.s_var in f}
    assert len(replaced) == 1 and parent[next(iter(replaced))] < 0
    key_s = arr.var_keys[[case.s_var]]
    gb.linearize()
    d_prev = gb.solve(0.0, False)
    assert np.all(np.isfinite(d_prev))
    values = arr.values.copy()
    out = []
    for step, (move, thr) in enumerate(W.steps(case.name)):
        values, state = W.moved_values(case, values, move)
        stats = gb.relinearize_partial(key_s, state)
        assert stats["n_fronts_reeliminated"] == 1 < stats["n_fronts"] == len(fronts), stats
        wf = W.wildfire_restatement(parent, fronts, gb.conditional, dims, d_prev, replaced, thr)
        margin = W.worst_margin(wf, replaced, thr)
        assert margin >= 100, (what, step, margin)
        if judge:    # the re-eliminated root (and every resident clique with it) against the system of the new values
            jd = J.Judge(arr, gb.jacobians())
            F = J.gather(gb, jd.sys)
            fr, rr = J.factor_ratio(jd.sys, F, 0.0, False), J.rhs_ratio(jd.sys, F)
            print(f"{what} step {step + 1}: factor {fr:.2f}u rhs {rr:.2f}u (k {jd.kf})")
            assert fr <= jd.kf and rr <= jd.kf, (what, step, fr, rr, jd.kf)
        d_wf, n_wf = gb.backsubstitute_wildfire(thr)
        print(f"{what} step {step + 1}: threshold {thr:g}, solved {n_wf} of {arr.n_vars} variables, margin {margin:.0f}, "
              f"outcomes { {o: wf.outcome.count(o) for o in (W.KEPT, W.RESTORED, W.SKIPPED)} }")
        assert n_wf == wf.count, (what, step, n_wf, wf.count)
        for c, (fv, sv) in enumerate(fronts):
            fi, si = W.scalars_of(dims, fv), W.scalars_of(dims, sv)
            if wf.outcome[c] != W.KEPT:      # untouched, or put back: the previous words
                assert np.array_equal(_words(d_wf[fi]), _words(d_prev[fi])), (what, step, c, wf.outcome[c], kern[c])
                continue
            assert c in replaced or not np.array_equal(_words(d_wf[fi]), _words(d_prev[fi])), (what, step, c, "kept, not written")
            if judge:
                k = J.k_solve(int(si.size), int(fi.size))
                r = _kept_ratio(gb.conditional(c), d_wf, fi, si)
                assert r <= k, (what, step, c, kern[c], "kept clique residual", r, k)
                w = WORST.get(kern[c], (0.0, k))
                WORST[kern[c]] = (max(w[0], r), min(w[1], k))
        out.append((list(wf.outcome), n_wf, _words(d_wf).copy()))
        d_prev = d_wf
    # threshold 0: everything
    d_all, n_all = gb.backsubstitute_wildfire(0.0)
    assert n_all == arr.n_vars
    out.append((None, n_all, _words(d_all).copy()))
    # the second threshold again, nothing moved: nothing is visited
    d_same, n_same = gb.backsubstitute_wildfire(W.steps(case.name)[1][1])
    assert n_same == 0 and np.array_equal(_words(d_same), _words(d_all)), (what, n_same)
    return out, values, d_all


def _fresh_solution(gpu, case, amalgamation, values):
    fresh = _handle(gpu, case, amalgamation)
    fresh.set_values(values)
    fresh.linearize()
    x = fresh.solve(0.0, False)
    fresh.close()
    return x


def _case(gpu, big_lds, name, amalgamation):
    case = W.build(name)
    dims = [int(d) for d in case.arr.var_dims]
    gb = _handle(gpu, case, amalgamation)
    parent, fronts = gb.get_tree()
    parent, fronts = [int(p) for p in parent], [(list(f), list(s)) for f, s in fronts]
    cls = [int(c) for c in gb.front_classes()]
    kern = W.kernel_of(parent, fronts, cls, dims, big_lds)
    what = f"{name} {amalgamation}"
    out, values, d_all = _sequence(gpu, case, gb, kern, what, True)
    gb.close()
    assert np.array_equal(_words(d_all), _words(_fresh_solution(gpu, case, amalgamation, values))), (what, "threshold 0")
    # the wave-per-clique handle: the same outcomes, counts and words in every pass
    plain = _handle(gpu, case, amalgamation, packed=False)
    kern_plain = W.kernel_of(parent, fronts, cls, dims, big_lds, packed=False)
    assert all(k in ("leaf64", "leaf_tail") for k, c in zip(kern_plain, cls) if c & 3 == 0)
    out_plain, _, _ = _sequence(gpu, case, plain, kern_plain, what + " unpacked", False)
    plain.close()
    for k, ((o1, n1, w1), (o2, n2, w2)) in enumerate(zip(out, out_plain)):
        assert o1 == o2 and n1 == n2 and np.array_equal(w1, w2), (what, "pass", k + 1, "packed / wave-per-clique", n1, n2)
    return case, fronts, kern, out


@pytest.mark.parametrize("name", list(W.CASES))
def test_wildfire_per_outcome_and_kernel(gpu, big_lds, name):
    case, fronts, kern, out = _case(gpu, big_lds, name, W.AMALGAMATION)
    targets = W.target_cliques(case, fronts)
    for c, (kind, shape) in targets.items():
        assert kern[c] == W.INTENDED[name][shape], (name, c, kind, shape, kern[c])
    step1 = out[0][0]
    for shape in case.shapes:
        seen = {step1[c] for c, (_, s) in targets.items() if s == shape}
        want = {W.KEPT, W.RESTORED, W.SKIPPED} if case.position == "bottom" else {W.KEPT, W.RESTORED}
        assert seen == want or (name == "combined1024" and shape == (193, 5) and seen == {W.KEPT, W.SKIPPED}), (shape, seen)
    assert W.SKIPPED in step1
    assert [n for _, n, _ in out[:3]] != [case.arr.n_vars] * 3
    for outcome, _, _ in out[:3]:
        for c in targets:
            SEEN.setdefault(kern[c], set()).add(outcome[c])
    print(name, "kernels of the cliques under test:", sorted({kern[c] for c in targets}))


@pytest.mark.parametrize("name", W.RELAXED_CASES)
def test_wildfire_on_relaxed_fronts(gpu, big_lds, name):
    """set_amalgamation(0.5, 64): a front holds several reference cliques and is visited, kept, restored or skipped as a
    whole; the restatement runs on the product's own tree."""
    case, fronts, kern, out = _case(gpu, big_lds, name, W.RELAXED)
    assert any(len(f) > 1 and not set(case.root) & set(f) and
               not any(f == arm.a_vars or f == arm.m_vars for arm in case.arms) for f, _ in fronts), "no merged front"
    step1 = out[0][0]
    assert {W.KEPT, W.RESTORED} <= set(step1) and ((W.SKIPPED in step1) == (name == "small2")), set(step1)
    for outcome, _, _ in out[:3]:
        for c in range(len(fronts)):
            SEEN_RELAXED.setdefault(kern[c], set()).add(outcome[c])
    print(name, "relaxed:", len(fronts), "fronts, kernels", {k: sorted(v) for k, v in SEEN_RELAXED.items()})


def test_every_branch_saw_every_outcome():
    """SEEN and WORST are filled by the tests above (whole module, one process, file order)."""
    print("outcomes per kernel:", {k: sorted(v) for k, v in sorted(SEEN.items())})
    print("worst kept-clique residual per kernel, u (smallest k):", {k: (round(v[0], 2), v[1]) for k, v in sorted(WORST.items())})
    assert set(SEEN) >= W.BRANCHES, sorted(W.BRANCHES - set(SEEN))
    for k in W.BRANCHES:
        assert SEEN[k] == {W.KEPT, W.RESTORED, W.SKIPPED}, (k, SEEN[k])
    assert set(WORST) >= W.BRANCHES
    assert "small2" in SEEN_RELAXED and {"leaf16", "leaf64"} & set(SEEN_RELAXED)
