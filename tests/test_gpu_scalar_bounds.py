"""The scalars behind every accept / reject decision of LM and Dogleg under DERIVED float64 bounds (tests/_ld_scalars.py):
e(0), e(delta), the model decrease, diag(A'A), the clamped damping and the Dogleg point, each against its exact value
formed in longdouble from the device's own [A b] and the device's own step — gamma_k with k counted from the kernels
(k of 10 to 223), six to nine digits under the oracle tolerances of test_gpu_parity.py (test_step_parity,
test_lm_trial_equals_separate_calls, the Dogleg trajectory).  tests/test_host_scalar_judge.py shows that the judge fails
on six mutations of the kernels' arithmetic.

Which kernel a case reaches (kernels.hip):
  linear_error_staged_kernel   test_staged_kernel (1 to 193 factors: one wave alone, both waves, a second block whose
                               second wave has no group, dead lanes), test_staged_slice_edges (the even rounding, 96 KB)
  linear_error_kernel          test_direct_kernel (1 to 513 factors; two-row factors on even and odd offsets, general rows;
                               one factor over the 96 KB limit)
  lin0_kernel, model_error_kernel, model_final_kernel
                               test_model_path (hv_list of 255 / 256 / 257 variables; lambda 0, 1e-3, 10; both dampings)
  reduce_final_kernel / reduce_final_pair_kernel
                               every case (1 to 3 partial sums; 255 to 257 partial sums need 65 000 factors: the loop is
                               the same strided one, see test_host_scalar_judge.final_pass)
  hessian_diag_kernel, make_damping_kernel
                               test_damping_clamps (both clamps bite; an entry equal to a limit; min == max)
  gradient_kernel, ax_sqnorm_kernel, vec_dot_kernel, vec_axpby_kernel
                               test_dogleg (tangent sizes 1, 255, 256, 257; the three branches of the dog leg)
  all of them on nonlinear graphs: test_nonlinear_graphs.

No public observable tells the staged from the direct kernel (gsx_kernel_time's "linear_error" phase covers both), so the
cases rely on the rule that decides: upload.hip: upload_problem sets lin_err_slice from the largest [A b] range of 64 consecutive
factors (0 above 96 KB for the two waves), kernels.hip:1002 takes the staged kernel iff it is positive.
_scalar_cases.slice_of restates the rule and every case asserts the side it is on.  Here the direct evaluation next to the model path
is taken through gsx_linear_error, which never uses the model; a handle created under GSX_LINERR_DIRECT (read when the
handle is created, like every schedule switch) is judged beside a default one in tests/test_gpu_schedule_options.py.

Dogleg on a linear graph: a GSX_F_LINEAR factor has no nonlinear error (kernels.hip:662 returns 0), so the loop is entered
with error_tol = -1, f(0) - f(dx) = 0 makes rho 0.5 by the 1e-15 guard (optimizers.hip: gsx_dogleg_optimize), the first trial is accepted with
the radius unchanged, and the values read back ARE the dog-leg point (retract of a vector is addition from 0): one
trust-region trial inside the one iteration.

Every scalar is read twice and must be bit-equal.  Each test prints its ratios in units of u; the last prints the worst.
Measured on the MI355X (worst over the module): e0 2.4 u and ed 14.0 u of gsx_linear_error (k 27 to 200; the 14.0 is the
single 48-row factor on 128 columns, k 200), e0 of lin0_kernel 1.1 u (k 27 to 33), model decrease 3.0 u (k 39 to 223),
diag(A'A) 3.4 u (k 10 to 188), Dogleg point 1.15 u of its norm (bounds 47 to 434 u); the clamped solves: factor 2.6 u, rhs
1.6 u, solve 1.2 u (k 364 / 1024).
"""
import numpy as np
import pytest

from gtsam_petercdev_amd import _abi as A
from gtsam_petercdev_amd import datasets
from tests import _ld_linear as J
from tests import _ld_scalars as S
from tests import _linear_cases as lcases
from tests import _scalar_cases as cases

pytestmark = pytest.mark.gpu
LD = np.longdouble
WORST = {"e0": 0.0, "ed": 0.0, "lin0": 0.0, "decrease": 0.0, "diag": 0.0, "dogleg": 0.0}


def _worst(key, r):
    WORST[key] = max(WORST[key], r)


@pytest.fixture(scope="module")
def gpu():
    from gtsam_petercdev_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the HIP path has no fallback"
    return _lib


def _handle(gpu, arr, ordering=A.ORDER_MINDEGREE):
    gb = gpu.product_backend(arr)
    gb.set_ordering(gb.compute_ordering(ordering))
    gb.linearize()
    return gb, S.Scalars(arr, gb.jacobians())


def _k_eval(arr, staged):
    """The k of gsx_linear_error's kernel, after asserting which one the slice rule selects."""
    assert (cases.slice_of(arr)[1] > 0) == staged, cases.slice_of(arr)
    return S.k_linear_error_staged(arr) if staged else S.k_linear_error_direct(arr)


def _judge_eval(gb, sc, k, what, solves):
    """gsx_linear_error at the step of each solve: e(0) and e(delta) by the non-negative-sum bound, read twice."""
    for lam, diag in solves:
        x = gb.solve(lam, diag)
        e0, ed = gb.linear_error()
        assert (e0, ed) == gb.linear_error(), (what, "two evaluations differ")
        _worst("e0", sc.check_e0(e0, k, f"{what} lam={lam:g}"))
        _worst("ed", sc.check_ed(ed, x, k, f"{what} lam={lam:g}"))


SOLVES = [(0.0, False), (1e-3, False), (10.0, True)]


# ---- gsx_linear_error: the staged kernel -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cases.STAGED_N)
def test_staged_kernel(gpu, n):
    arr = cases.chain(n)
    gb, sc = _handle(gpu, arr)
    assert np.array_equal(gb.jacobians(), cases.jacobian_array(arr))     # unit noise: [A b] is what was given
    _judge_eval(gb, sc, _k_eval(arr, True), f"staged {n}", SOLVES)


@pytest.mark.parametrize("name", ["rounding", "limit"])
def test_staged_slice_edges(gpu, name):
    """The only group ends one double short of the slice's even rounding (25 of 26); 64 factors fill two slices of
    exactly 96 KB and a 65th makes the second wave's group."""
    arr = cases.staged_rounding() if name == "rounding" else cases.staged_limit()
    assert cases.slice_of(arr) == ((25, 26) if name == "rounding" else (6144, 6144))
    gb, sc = _handle(gpu, arr)
    _judge_eval(gb, sc, _k_eval(arr, True), f"staged {name}", SOLVES)


# ---- gsx_linear_error: the direct kernel -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cases.DIRECT_N + ["over"])
def test_direct_kernel(gpu, n):
    """A 64-factor range over the limit: lin_err_slice is 0.  Two-row factors on even offsets take the double2 path, those
    on odd offsets and the three- and nine-row factors the general one.  The single 48-row factor leaves a singular
    system: its steps come from damped solves only."""
    arr = cases.staged_limit(over=True) if n == "over" else cases.direct_mix(n)
    if n not in (1, "over"):
        even, odd, other = cases.two_row_offsets(arr)
        assert even > 0 and odd > 0 and other > 0
    gb, sc = _handle(gpu, arr)
    _judge_eval(gb, sc, _k_eval(arr, False), f"direct {n}", [(1.0, False), (10.0, True)] if n == 1 else SOLVES)


# ---- gsx_lm_trial: e(0) from lin0_kernel, e(delta) from the model ----------------------------------------------------------------
def _judge_trial(gb, sc, arr, what, lam, diag, limits=(1e-6, 1e32), k_eval=None):
    e0, ed, _ = gb.lm_trial(False, lam, diag, *limits)
    assert (e0, ed) == gb.lm_trial(False, lam, diag, *limits)[:2], (what, "two trials differ")
    x = gb.solve(lam, diag, *limits)         # the trial's step: the same factorization and substitution again
    tag = f"{what} lam={lam:g} diag={int(diag)}"
    _worst("lin0", sc.check_e0(e0, S.k_lin0(arr), tag, "e0 (lin0)"))
    _worst("decrease", sc.check_model_decrease(e0, ed, x, lam, diag, S.k_model(arr, sc.m), tag, *limits))
    if k_eval is not None:                   # the direct evaluation at the same step, by the plain bound
        d0, dd = gb.linear_error()
        _worst("e0", sc.check_e0(d0, k_eval, tag))
        _worst("ed", sc.check_ed(dd, x, k_eval, tag))


@pytest.mark.parametrize("name", ["vars255", "vars256", "vars257", "direct257"])
def test_model_path(gpu, name):
    arr = cases.direct_mix(257) if name == "direct257" else cases.chain_vars(int(name[4:]))
    staged = name != "direct257"
    if staged:
        assert arr.n_vars == int(name[4:])
    gb, sc = _handle(gpu, arr)
    k_eval = _k_eval(arr, staged)
    for lam in (0.0, 1e-3, 10.0):
        for diag in (False, True):
            _judge_trial(gb, sc, arr, f"model {name}", lam, diag, k_eval=k_eval)


# ---- diag(A'A) and the clamped damping ---------------------------------------------------------------------------------------------
def test_damping_clamps(gpu):
    """min_diagonal above some entries of diag(A'A) and max_diagonal below others, both limits ENTRIES of the device's
    diagonal (an entry exactly equal to a limit), then min == max.  The damped factorization and its step are judged by
    _ld_linear's backward-error measures with the limits passed through; the model decrease by the scalar judge."""
    arr = cases.clamp_graph()
    gb, sc = _handle(gpu, arr)
    judge = J.Judge(arr, gb.jacobians())
    hd = gb.hessian_diagonal()
    assert np.array_equal(hd, gb.hessian_diagonal())
    _worst("diag", sc.check_diag(hd, "clamp graph"))
    srt = np.sort(hd)
    lo, hi, mid = float(srt[len(srt) // 4]), float(srt[3 * len(srt) // 4]), float(srt[len(srt) // 2])
    assert (hd < lo).any() and (hd > hi).any() and (hd == lo).any() and (hd == hi).any() and hi > 100 * lo
    for limits in ((lo, hi), (mid, mid)):
        for lam in (0.3, 10.0):
            x = gb.solve(lam, True, *limits)
            assert np.array_equal(x, gb.solve(lam, True, *limits))
            judge.check_backward(gb, x, lam, True, f"clamps {limits}", limits=limits)
            _judge_trial(gb, sc, arr, f"clamps {limits}", lam, True, limits)
    # the clamp really changed the step: the default limits give another one
    assert not np.array_equal(gb.solve(0.3, True), gb.solve(0.3, True, lo, hi))


# ---- Dogleg ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", cases.DOGLEG_TANGENT)
def test_dogleg(gpu, nt):
    """One iteration from 0 at three radii: below |dx_u| (radius g / |g|: gradient_kernel, vec_dot), between |dx_u| and
    |dx_n| (the dog-leg point: g'g / |A g|^2, delta'delta, g'delta, vec_axpby) and above |dx_n| (the Newton point, bit for
    bit).  The Newton step comes from a twin handle's solve(0).  One scalar (nt = 1): steepest descent IS Newton's step,
    there is no middle radius."""
    arr = cases.dogleg_graph(nt)
    twin, sc = _handle(gpu, arr)
    dx_n = twin.solve(0.0, False)
    k_ax, k_dot = S.k_ax_sqnorm(arr), S.k_vec_dot(nt)
    _, _, _, (uu, nn) = S.dogleg_expected(sc, dx_n, 1.0, k_ax, k_dot)
    ru, rn = float(np.sqrt(uu)), float(np.sqrt(nn))
    radii = {"steepest": 0.5 * ru, "newton": 1.5 * rn}
    if nt > 1:
        assert ru < 0.9 * rn, (ru, rn)
        radii["dogleg"] = 0.5 * (ru + rn)
    else:
        assert abs(ru - rn) <= 1e-12 * rn
    for branch, radius in radii.items():
        got = []
        for _ in range(2):                    # a fresh handle each: the iteration commits its point
            gb = gpu.product_backend(arr)
            gb.set_ordering(gb.compute_ordering(A.ORDER_MINDEGREE))
            r = gb.dogleg_optimize(radius, max_iterations=1, error_tol=-1.0)
            assert r["iterations"] == 1 and r["final_lambda"] == radius, r
            got.append(gb.get_values())
            gb.close()
        assert np.array_equal(got[0], got[1]), (branch, "two runs differ")
        which, want, bnd, _ = S.dogleg_expected(sc, dx_n, radius, k_ax, k_dot)
        assert which == branch
        err = float(S._norm(np.asarray(got[0], LD) - want))
        size = float(S._norm(want))
        print(f"dogleg {nt} {branch}: radius {radius:.4g}, error {err / size / S.U:.2f} u, bound {float(bnd) / size / S.U:.1f} u")
        if branch == "newton":
            assert np.array_equal(got[0], dx_n)
        else:
            assert err <= float(bnd), (nt, branch, err, float(bnd))
            if branch == "steepest":      # and the step has the length of the radius
                assert abs(size - radius) <= 1e-15 * radius
        _worst("dogleg", err / size / S.U)


# ---- nonlinear graphs -------------------------------------------------------------------------------------------------------------------
def _pose2_landmarks():
    """65 Pose2 in a chain (21-double between blocks) with 22 landmarks seen from three poses each (12-double
    bearing-range blocks): odd and even offsets mixed."""
    from gtsam_petercdev_amd import graph as G
    rng = np.random.default_rng(88)
    fg, vals = G.NonlinearFactorGraph(), G.Values()
    odo = G.noiseModel.Diagonal.Sigmas([0.2, 0.2, 0.1])
    br = G.noiseModel.Diagonal.Sigmas([0.1, 0.2])
    poses = [(0.9 * k, 0.3 * np.sin(0.4 * k), 0.1 * np.cos(0.3 * k)) for k in range(65)]
    fg.add(G.PriorFactor(0, G.Pose2(*poses[0]), G.noiseModel.Diagonal.Sigmas([0.3, 0.3, 0.1])))
    for k in range(65):
        vals.insert(k, G.Pose2(*(np.array(poses[k]) + rng.normal(0, 0.03, 3))))
    for k in range(64):
        a, b = poses[k], poses[k + 1]
        c, s = np.cos(a[2]), np.sin(a[2])
        dx, dy = b[0] - a[0], b[1] - a[1]
        fg.add(G.BetweenFactor(k, k + 1, G.Pose2(c * dx + s * dy, -s * dx + c * dy, b[2] - a[2]), odo))
        if k % 3 == 0:
            L = 1000 + k // 3
            p = np.array([a[0] + 1.0, 2.0 + 0.1 * k])
            vals.insert(L, p + rng.normal(0, 0.05, 2))
            for q in (k, k + 1, k + 2):
                if q < 65:
                    x, y, th = poses[q]
                    fg.add(G.BearingRangeFactor(q, L, np.arctan2(p[1] - y, p[0] - x) - th, np.hypot(p[0] - x, p[1] - y), br))
    return fg.to_arrays(vals)


@pytest.mark.parametrize("name", ["bal7", "pose2_65", "pose3_129"])
def test_nonlinear_graphs(gpu, name):
    """The same measures on real linearizations: e(0) / e(delta) of gsx_linear_error, diag(A'A), and the model decrease
    after a real LM trial (relinearize = True)."""
    if name == "bal7":
        arr, ordering = lcases.bal_arrays(7), A.ORDER_SCHUR
    elif name == "pose2_65":
        arr, ordering = _pose2_landmarks(), A.ORDER_MINDEGREE
        assert {21, 12} <= set(np.diff(arr.jacobian_offsets()).tolist())
    else:
        arr, ordering = datasets.synth_manhattan_pose3(129, seed=4), A.ORDER_MINDEGREE
        assert 78 in set(np.diff(arr.jacobian_offsets()).tolist())
    gb = gpu.product_backend(arr)
    gb.set_ordering(gb.compute_ordering(ordering))
    e0, ed, _ = gb.lm_trial(True, 0.1, True)
    sc = S.Scalars(arr, gb.jacobians())
    x = gb.solve(0.1, True)
    _worst("lin0", sc.check_e0(e0, S.k_lin0(arr), name, "e0 (lin0)"))
    _worst("decrease", sc.check_model_decrease(e0, ed, x, 0.1, True, S.k_model(arr, sc.m), name))
    _worst("diag", sc.check_diag(gb.hessian_diagonal(), name))
    _judge_eval(gb, sc, _k_eval(arr, True), name, [(0.1, True), (1e-3, False)])


def test_worst_ratios():
    """Prints the worst ratio per measure (filled by the tests above when the module runs in one process)."""
    print("worst ratios (u):", {k: round(v, 2) for k, v in WORST.items()})
