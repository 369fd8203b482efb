"""Proves without a GPU that the scalar judge of tests/_ld_scalars.py can fail: float64 numpy emulations of the reduction
kernels' summation order (serial sums per thread, block_sum's shuffle tree and wave loop, the final pass) hold its derived
bounds on every case the device is judged on, and six one-line mutations of those emulations each miss them.  The case
shapes the GPU tests are aimed at (which kernel the slice rule selects, offsets' parity, variable counts) are asserted
here too, host-only.

Measured (emulations, worst over the cases): e0 1.1 u, ed 1.1 u against k of 26 to 51, |Ag|^2 0.3 u (k 33), diag 2.3 u
(k 11), damping 2.3 u (k 12); the mutants miss by 6e12 u or more."""
import mpmath
import numpy as np
import pytest

from tests import _ld_scalars as S
from tests import _scalar_cases as cases

LD = np.longdouble


# ---- the kernels' order of summation in float64 ------------------------------------------------------------------------------
def block_sum(v):
    """kernels.hip block_sum: per wave the shuffle-down tree (lane 0's value), then thread 0 adds the waves in order."""
    v = np.asarray(v, np.float64)
    total = np.float64(0)
    for w in range(v.size // 64):
        x = v[64 * w:64 * (w + 1)].copy()
        o = 32
        while o > 0:
            x[:64 - o] = x[:64 - o] + x[o:]       # lanes past 64 - o keep garbage lane 0 never reads
            o >>= 1
        total = total + x[0]
    return total


def final_pass(partials):
    acc = np.zeros(256)
    for i, p in enumerate(partials):
        acc[i % 256] = acc[i % 256] + p
    return block_sum(acc)


def _factor_rows(arr, jac, f, x, b_sign=-1.0, drop_second_row=False):
    """[(b^2, e^2)] per row of factor f in float64, e = A x - b accumulated column by column."""
    off = arr.jacobian_offsets()
    m = int(arr.f_rows[f])
    J = jac[off[f]:off[f + 1]].reshape(-1, m)
    toff = arr.tangent_offsets()
    xs = np.concatenate([x[toff[v]:toff[v + 1]] for v in arr.f_vars[arr.f_key_ptr[f]:arr.f_key_ptr[f + 1]]])
    out = []
    for r in range(m):
        if drop_second_row and m == 2 and r == 1:
            continue
        b = J[-1, r]
        e = np.float64(b_sign * b)
        for c in range(xs.size):
            e = e + J[c, r] * xs[c]
        out.append((b * b, e * e))
    return out


def linear_error_direct(arr, jac, x, **mut):
    n = arr.n_factors
    nb = min(max(-(-n // 256), 1), S.CAP // 2)
    p0, pd = [], []
    for blk in range(nb):
        a0, ad = np.zeros(256), np.zeros(256)
        for t in range(256):
            for f in range(blk * 256 + t, n, nb * 256):
                for q0, qd in _factor_rows(arr, jac, f, x, **mut):
                    a0[t], ad[t] = a0[t] + q0, ad[t] + qd
        p0.append(block_sum(0.5 * a0))
        pd.append(block_sum(0.5 * ad))
    return final_pass(p0), final_pass(pd)


def linear_error_staged(arr, jac, x, drop_last_group=False, dead_lanes_live=False, **mut):
    n = arr.n_factors
    groups = -(-n // 64)
    nb = min(max((groups + 1) // 2, 1), S.CAP // 2)
    p0, pd = [], []
    for blk in range(nb):
        a0, ad = np.zeros(128), np.zeros(128)
        for wave in range(2):
            for g in range(blk * 2 + wave, groups - int(drop_last_group), nb * 2):
                for lane in range(64):
                    f = g * 64 + lane
                    if f >= n:
                        if not dead_lanes_live:
                            continue
                        f = n - 1                 # the alias the kernel gives its dead lanes
                    for q0, qd in _factor_rows(arr, jac, f, x, **mut):
                        a0[64 * wave + lane], ad[64 * wave + lane] = a0[64 * wave + lane] + q0, ad[64 * wave + lane] + qd
        p0.append(block_sum(0.5 * a0))
        pd.append(block_sum(0.5 * ad))
    return final_pass(p0), final_pass(pd)


def ax_sqnorm(arr, jac, v, skip_factor=None):
    n = arr.n_factors
    nb = min(max(-(-n // 256), 1), S.CAP)
    parts = []
    for blk in range(nb):
        acc = np.zeros(256)
        for t in range(256):
            for f in range(blk * 256 + t, n, nb * 256):
                if f == skip_factor:
                    continue
                for _, qd in _factor_rows(arr, jac, f, v, b_sign=0.0):     # the kernel has no b: e starts at 0
                    acc[t] = acc[t] + qd
        parts.append(block_sum(acc))
    return final_pass(parts)


def hessian_diag(arr, jac):
    """diag(A'A) accumulated factor by factor in float64 (any order holds the bound)."""
    off, toff = arr.jacobian_offsets(), arr.tangent_offsets()
    d = np.zeros(int(toff[-1]))
    for f in range(arr.n_factors):
        m = int(arr.f_rows[f])
        J = jac[off[f]:off[f + 1]].reshape(-1, m)
        idx = np.concatenate([np.arange(toff[v], toff[v + 1]) for v in arr.f_vars[arr.f_key_ptr[f]:arr.f_key_ptr[f + 1]]])
        for c, i in enumerate(idx):
            for r in range(m):
                d[i] = d[i] + J[c, r] * J[c, r]
    return d


def _case(arr):
    jac = cases.jacobian_array(arr)
    sc = S.Scalars(arr, jac)
    x = np.random.default_rng(arr.n_factors).normal(size=sc.n)
    return jac, sc, x


# ---- the judge's own arithmetic ------------------------------------------------------------------------------------------------
def test_longdouble_scalars_against_mpmath():
    arr = cases.chain(9)
    jac, sc, x = _case(arr)
    mpmath.mp.dps = 50
    off, toff = arr.jacobian_offsets(), arr.tangent_offsets()
    e0 = ed = ag = mpmath.mpf(0)
    g = [mpmath.mpf(0)] * sc.n
    rows = []
    for f in range(arr.n_factors):
        m = int(arr.f_rows[f])
        J = jac[off[f]:off[f + 1]].reshape(-1, m)
        idx = np.concatenate([np.arange(toff[v], toff[v + 1]) for v in arr.f_vars[arr.f_key_ptr[f]:arr.f_key_ptr[f + 1]]])
        for r in range(m):
            b = mpmath.mpf(float(J[-1, r]))
            a = [mpmath.mpf(float(J[c, r])) for c in range(idx.size)]
            rows.append((idx, a))
            e0 += b * b / 2
            ed += (sum(ac * mpmath.mpf(float(x[i])) for ac, i in zip(a, idx)) - b) ** 2 / 2
            for ac, i in zip(a, idx):
                g[i] += ac * b
    for idx, a in rows:
        ag += sum(ac * g[i] for ac, i in zip(a, idx)) ** 2

    def rel(got, want):
        got = mpmath.mpf(float(got)) + mpmath.mpf(float(got - LD(float(got))))
        return float(abs(got - want) / abs(want))
    assert rel(sc.e0, e0) <= 1e-17 and rel(sc.ed(x), ed) <= 1e-17 and rel(sc.ax2(sc.g), ag) <= 1e-17
    assert max(rel(a, b) for a, b in zip(sc.g, g)) <= 1e-16
    assert S.block_depth(256) == 10 and S.block_depth(128) == 8 and S.k_final(257) == 12


# ---- the shapes the device cases are aimed at --------------------------------------------------------------------------------
def test_case_shapes():
    for n in cases.STAGED_N:
        arr = cases.chain(n)
        assert arr.n_factors == n and cases.slice_of(arr)[1] > 0
    assert cases.slice_of(cases.staged_rounding()) == (25, 26)
    assert cases.slice_of(cases.staged_limit()) == (6144, 6144) and cases.staged_limit().n_factors == 65
    assert cases.slice_of(cases.staged_limit(over=True)) == (6176, 0)
    for n in cases.DIRECT_N:
        arr = cases.direct_mix(n)
        assert arr.n_factors == n and cases.slice_of(arr)[1] == 0, n
        if n > 1:
            even, odd, other = cases.two_row_offsets(arr)
            assert even > 0 and odd > 0 and other > 0, (n, even, odd, other)
    for nv in (255, 256, 257):
        assert cases.chain_vars(nv).n_vars == nv
    for nt in cases.DOGLEG_TANGENT:
        assert int(cases.dogleg_graph(nt).var_dims.sum()) == nt


# ---- correct emulations pass ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cases.STAGED_N)
def test_staged_emulation_passes(n):
    arr = cases.chain(n)
    jac, sc, x = _case(arr)
    e0, ed = linear_error_staged(arr, jac, x)
    k = S.k_linear_error_staged(arr)
    sc.check_e0(e0, k, f"staged emulation {n}")
    sc.check_ed(ed, x, k, f"staged emulation {n}")


@pytest.mark.parametrize("n", [255, 257])
def test_direct_emulation_passes(n):
    arr = cases.direct_mix(n)
    jac, sc, x = _case(arr)
    e0, ed = linear_error_direct(arr, jac, x)
    k = S.k_linear_error_direct(arr)
    sc.check_e0(e0, k, f"direct emulation {n}")
    sc.check_ed(ed, x, k, f"direct emulation {n}")


def test_dogleg_and_damping_emulations_pass():
    arr = cases.clamp_graph()
    jac, sc, _ = _case(arr)
    g64 = sc.g.astype(np.float64)
    sc.check_ax2(ax_sqnorm(arr, jac, g64), g64, S.k_ax_sqnorm(arr), "ax_sqnorm emulation")
    d = hessian_diag(arr, jac)
    sc.check_diag(d, "diag emulation")
    lo, hi = np.sort(d)[[len(d) // 4, 3 * len(d) // 4]]
    assert (d < lo).any() and (d > hi).any()
    damp = 0.3 * np.minimum(np.maximum(d, lo), hi)
    sc.check_damping(damp, 0.3, True, lo, hi, "damping emulation")


# ---- the mutants fail ------------------------------------------------------------------------------------------------------------
def _fails(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


def test_mutant_last_group_dropped():
    arr = cases.chain(193)
    jac, sc, x = _case(arr)
    e0, ed = linear_error_staged(arr, jac, x, drop_last_group=True)
    k = S.k_linear_error_staged(arr)
    _fails(sc.check_e0, e0, k, "mutant: last group dropped")
    _fails(sc.check_ed, ed, x, k, "mutant: last group dropped")


def test_mutant_dead_lane_alias_counted():
    arr = cases.chain(65)
    jac, sc, x = _case(arr)
    e0, ed = linear_error_staged(arr, jac, x, dead_lanes_live=True)
    k = S.k_linear_error_staged(arr)
    _fails(sc.check_e0, e0, k, "mutant: dead lanes alias the last factor")
    _fails(sc.check_ed, ed, x, k, "mutant: dead lanes alias the last factor")


def test_mutant_second_row_dropped():
    arr = cases.direct_mix(255)
    jac, sc, x = _case(arr)
    e0, ed = linear_error_direct(arr, jac, x, drop_second_row=True)
    k = S.k_linear_error_direct(arr)
    _fails(sc.check_e0, e0, k, "mutant: second row of a two-row factor dropped")
    _fails(sc.check_ed, ed, x, k, "mutant: second row of a two-row factor dropped")


def test_mutant_wrong_sign_of_b():
    arr = cases.chain(64)
    jac, sc, x = _case(arr)
    e0, ed = linear_error_staged(arr, jac, x, b_sign=1.0)
    k = S.k_linear_error_staged(arr)
    sc.check_e0(e0, k, "mutant: b with the wrong sign (e0 does not see it)")
    _fails(sc.check_ed, ed, x, k, "mutant: b with the wrong sign")


def test_mutant_clamp_on_lambda_d():
    arr = cases.clamp_graph()
    jac, sc, _ = _case(arr)
    d = hessian_diag(arr, jac)
    lo, hi = np.sort(d)[[len(d) // 4, 3 * len(d) // 4]]
    damp = np.minimum(np.maximum(0.3 * d, lo), hi)
    _fails(sc.check_damping, damp, 0.3, True, lo, hi, "mutant: clamp applied to lambda d")


def test_mutant_ax_sqnorm_without_a_factor():
    arr = cases.chain(129)
    jac, sc, _ = _case(arr)
    g64 = sc.g.astype(np.float64)
    _fails(sc.check_ax2, ax_sqnorm(arr, jac, g64, skip_factor=77), g64, S.k_ax_sqnorm(arr), "mutant: |Ag|^2 without a factor")
