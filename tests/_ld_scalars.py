"""The extended-precision judge of the SCALARS behind every accept / reject decision of LM and Dogleg (host only, no GPU,
no oracle): the linearized errors e(0) and e(delta), the model decrease, diag(A'A), the damping vector, and Dogleg's
g = A'b, g'g, |A g|^2 and dog-leg point.  Inputs are a backend's own float64 [A b] (gsx_get_jacobians) and its own step:
only the reductions are judged — linearization and the solve are judged elsewhere (_ld_linear.py).

Exact values are formed in numpy.longdouble (64-bit significand) from the float64 data:

    e0* = 1/2 sum b^2      ed* = 1/2 sum |A delta - b|^2      g* = A'b      |A g*|^2      d* = diag(A'A)

Bounds are DERIVED from the kernels' code, not measured.  gamma_k = k u / (1 - k u), u = 2^-53.  A sum of non-negative
terms computed in ANY order with k roundings behind each term is within gamma_k of its exact value (Higham, Accuracy and
Stability of Numerical Algorithms, 2nd ed., section 4.2): e0, ed, |A g|^2, diag(A'A) and g'g are such sums, judged by
|got - exact| <= gamma_k exact.  The signed sums (g, g'delta) are judged by gamma_k sum |terms|.
(ed and |A g|^2 are non-negative sums of SQUARES of signed inner products: strictly, the rounding behind a row's
e = A delta - b is relative to |b| + |A||delta|, not to |e|.  The bound gamma_k exact is the tighter of the two and is
kept; the test graphs have residuals of the size of b.)

k is the number of roundings on the longest path from a datum to the scalar (kernels.hip line numbers):

  term     the flops of one row's term: its columns, + 3 (the subtraction of b, the square, the factor 1/2):
           linear_error_kernel :918-930 / :899-915, linear_error_staged_kernel :974-986, ax_sqnorm_kernel :1792-1802
  serial   the additions into one thread's accumulator: (rows of the tallest factor) x ceil(items / (grid x block)),
           grid from the launcher (:1008-1014, :1070, :1078, :1809, :1822)
  block    block_sum :55-66: wave_sum's six shuffle steps (:34-38) and one addition per wave of the block
  final    reduce_final_kernel :805-811 / reduce_final_pair_kernel :815-820 / model_final_kernel :1059-1068:
           ceil(partials / 256) serial additions and block_sum of 256 threads

The model-based e(delta) of gsx_lm_trial: e(delta) = e(0) - 1/2 g'delta - 1/2 lambda delta'D delta holds for the exact
solution of (H + lambda D) delta = g; for the computed one, with r = (H + lambda D) delta - g, the true value is larger
by 1/2 delta'r.  The judge forms r in longdouble and allows, ON THE MODEL DECREASE e(0) - e(delta) (what LM divides by),

    |1/2 delta'r| + gamma_k (|g|'|delta| + lambda delta'D delta),

k of model_error_kernel :1046-1054 (k_model below).
"""
import numpy as np

from tests._ld_linear import LD, U

CAP = 4096                                   # handle.h: gsx_context::kPartials


def _cdiv(a, b):
    return -(-int(a) // int(b))


def block_depth(threads):
    """block_sum (kernels.hip:55-66): six shuffle additions, then thread 0 adds one value per wave."""
    return 6 + threads // 64


def k_final(partials, pair=False):
    """reduce_final_kernel / reduce_final_pair_kernel / model_final_kernel: 256 threads stride over the partial sums."""
    return _cdiv(partials, 256) + block_depth(256)


def _shape(arr):
    """(A-columns of the widest factor, rows of the tallest)."""
    nk = np.diff(arr.f_key_ptr)
    cols = np.add.reduceat(arr.var_dims[arr.f_vars], arr.f_key_ptr[:-1])
    return int(np.max(np.where(nk > 0, cols, 0))), int(arr.f_rows.max())


def k_linear_error_direct(arr):
    """linear_error_kernel (:888-938): grid = ceil(n / 256) <= kPartials / 2 (:1012-1013), 256 threads, a factor a thread
    per trip, its rows added one after the other (:928-929; :912-915 for the double2 path)."""
    cols, rows = _shape(arr)
    n = arr.n_factors
    nb = min(max(_cdiv(n, 256), 1), CAP // 2)
    return (cols + 3) + rows * _cdiv(n, nb * 256) + block_depth(256) + k_final(nb)


def k_linear_error_staged(arr):
    """linear_error_staged_kernel (:945-997): 128 threads = two waves, a group of 64 factors a wave per trip, grid =
    ceil(groups / 2) <= kPartials / 2 (:1008-1009); a lane adds the rows of its factor of every group of its wave."""
    cols, rows = _shape(arr)
    groups = _cdiv(arr.n_factors, 64)
    nb = min(max(_cdiv(groups, 2), 1), CAP // 2)
    return (cols + 3) + rows * _cdiv(groups, 2 * nb) + block_depth(128) + k_final(nb)


def k_lin0(arr):
    """lin0_kernel (:1027-1040): a factor's term is 1/2 sum_r b_r^2 — rows additions, the square, the factor 1/2 — added
    once per factor; grid = ceil(n / 256) <= kPartials (:1070-1071)."""
    _, rows = _shape(arr)
    n = arr.n_factors
    nb = min(max(_cdiv(n, 256), 1), CAP)
    return (rows + 2) + _cdiv(n, nb * 256) + block_depth(256) + k_final(nb)


def k_ax_sqnorm(arr):
    """ax_sqnorm_kernel (:1787-1806): as the direct kernel without b; grid = ceil(n / 256) <= kPartials (:1809-1810)."""
    cols, rows = _shape(arr)
    n = arr.n_factors
    nb = min(max(_cdiv(n, 256), 1), CAP)
    return (cols + 2) + rows * _cdiv(n, nb * 256) + block_depth(256) + k_final(nb)


def k_vec_dot(n):
    """vec_dot_kernel (:1814-1819): one product a term; grid = ceil(n / 1024) <= kPartials (:1822-1823)."""
    nb = min(max(_cdiv(n, 1024), 1), CAP)
    return 1 + _cdiv(n, nb * 256) + block_depth(256) + k_final(nb)


def k_model(arr, m):
    """model_error_kernel (:1041-1057): a scalar's term x (g + lambda D x) is four flops, a variable's scalars are added
    one after the other (:1050-1053), a variable a thread per trip, grid = ceil(variables / 256) <= kPartials (:1078-1079);
    model_final_kernel halves the sum and subtracts it from e(0) (:1066: two roundings).  g is read from the rhs rows of
    the H panels: an inner product of at most m terms in any order, gamma_m (m = _ld_linear's longest accumulation)."""
    nv = arr.n_vars
    nb = min(max(_cdiv(nv, 256), 1), CAP)
    return 4 + int(arr.var_dims.max()) * _cdiv(nv, nb * 256) + block_depth(256) + k_final(nb) + 2 + m


def k_diag(m):
    """An entry of diag(A'A): a sum of at most m squares in any order, a rounding for each square."""
    return m + 1


def _ratio(err, scale):
    """|err| / (u scale); infinite where the scale is 0 and the error is not, or the error is not finite."""
    err, scale = np.abs(np.asarray(err, LD)), np.asarray(scale, LD)
    if not np.all(np.isfinite(err)) or np.any((scale == 0) & (err != 0)):
        return float("inf")
    pos = scale > 0
    return float(np.max(err[pos] / scale[pos]) / LD(U)) if pos.any() else 0.0


def bound(k):
    """gamma_k in units of u: what a ratio is compared with."""
    return k / (1.0 - k * U)


class Scalars:
    """The exact scalars of one linearization, from the float64 [A b] of jacobians(), factor block by factor block."""

    def __init__(self, arrays, jac):
        self.arrays = arrays
        self.off = np.asarray(arrays.tangent_offsets(), dtype=np.int64)
        self.n = n = int(self.off[-1])
        joff = arrays.jacobian_offsets()
        self.blocks = []                      # (scalar indices, A_f, b_f) per factor, longdouble
        self.g = np.zeros(n, LD)
        self.absg = np.zeros(n, LD)           # |A'||b|
        self.diagH = np.zeros(n, LD)
        rows = np.zeros(n, np.int64)
        e0 = LD(0)
        for f in range(arrays.n_factors):
            vs = arrays.f_vars[arrays.f_key_ptr[f]:arrays.f_key_ptr[f + 1]]
            m = int(arrays.f_rows[f])
            idx = np.concatenate([np.arange(self.off[v], self.off[v + 1]) for v in vs])
            Ab = np.asarray(jac[joff[f]:joff[f + 1]], dtype=np.float64).reshape(idx.size + 1, m).T.astype(LD)
            A, b = Ab[:, :-1], Ab[:, -1]
            self.blocks.append((idx, A, b))
            self.g[idx] += np.dot(A.T, b)
            self.absg[idx] += np.dot(np.abs(A).T, np.abs(b))
            self.diagH[idx] += np.sum(A * A, axis=0)
            rows[idx] += m
            e0 += np.dot(b, b)
        self.e0 = e0 / 2
        self.m = int(rows.max()) + 1          # as _ld_linear: + the damping row
        self.gg = np.dot(self.g, self.g)

    # ---- exact values ----
    def ed(self, x):
        x = np.asarray(x, LD)
        s = LD(0)
        for idx, A, b in self.blocks:
            e = np.dot(A, x[idx]) - b
            s += np.dot(e, e)
        return s / 2

    def ax2(self, v):
        v = np.asarray(v, LD)
        s = LD(0)
        for idx, A, _ in self.blocks:
            e = np.dot(A, v[idx])
            s += np.dot(e, e)
        return s

    def times(self, x, damp=None):
        """(A'A + diag(damp)) x."""
        x = np.asarray(x, LD)
        y = np.zeros(self.n, LD) if damp is None else np.asarray(damp, LD) * x
        for idx, A, _ in self.blocks:
            y[idx] += np.dot(A.T, np.dot(A, x[idx]))
        return y

    def damping(self, lam, diag, min_diagonal=1e-6, max_diagonal=1e32):
        """lambda D: D = I or clamp(diag A'A) — make_damping_kernel's fmin(fmax(d, min), max) (:1670)."""
        if not lam > 0:
            return np.zeros(self.n, LD)
        d = np.minimum(np.maximum(self.diagH, LD(min_diagonal)), LD(max_diagonal)) if diag else np.ones(self.n, LD)
        return LD(lam) * d

    # ---- checks: each returns its ratio in units of u and asserts it under gamma_k ----
    def _check(self, what, name, ratio, k):
        print(f"{what}: {name} {ratio:.2f} u (k {k})")
        assert ratio <= bound(k), (what, name, ratio, k)
        return ratio

    def check_e0(self, got, k, what, name="e0"):
        return self._check(what, name, _ratio(LD(got) - self.e0, self.e0), k)

    def check_ed(self, got, x, k, what, name="ed"):
        ed = self.ed(x)
        return self._check(what, name, _ratio(LD(got) - ed, ed), k)

    def check_diag(self, got, what):
        return self._check(what, "diag", _ratio(np.asarray(got, LD) - self.diagH, self.diagH), k_diag(self.m))

    def check_damping(self, got, lam, diag, min_diagonal, max_diagonal, what):
        """A damping vector lambda D (host emulations; the device's is judged through its solve): one more rounding for
        the product with lambda."""
        want = self.damping(lam, diag, min_diagonal, max_diagonal)
        return self._check(what, "damping", _ratio(np.asarray(got, LD) - want, want), k_diag(self.m) + 1)

    def check_ax2(self, got, v, k, what):
        want = self.ax2(v)
        return self._check(what, "|Ag|^2", _ratio(LD(got) - want, want), k)

    def check_model_decrease(self, e0_got, ed_got, x, lam, diag, k, what, min_diagonal=1e-6, max_diagonal=1e32):
        """e(0) - e(delta) of the model path against the true decrease, with the 1/2 delta'r allowance."""
        x = np.asarray(x, LD)
        damp = self.damping(lam, diag, min_diagonal, max_diagonal)
        r = self.times(x, damp) - self.g
        slack = np.abs(np.dot(x, r)) / 2
        want = self.e0 - self.ed(x)
        scale = np.dot(np.abs(self.g), np.abs(x)) + np.dot(x, damp * x)
        err = np.abs((LD(e0_got) - LD(ed_got)) - want)
        ratio = _ratio(max(err - slack, LD(0)), scale)
        print(f"{what}: decrease {float(want):.6e}, 1/2 delta'r {float(slack):.2e}, error {float(err):.2e}")
        return self._check(what, "decrease", ratio, k)


# ---- Dogleg ------------------------------------------------------------------------------------------------------------------
def _norm(v):
    v = np.asarray(v, LD)
    return np.sqrt(np.dot(v, v))


def dogleg_expected(S, dx_n, radius, k_ax, k_dot):
    """(branch, expected point, bound on ||point - expected||_2) of DoglegOptimizerImpl::ComputeDoglegPoint as
    gsx_dogleg_optimize evaluates it (optimizers.hip: dogleg_coefficients and the steepest-descent point of the iterate body), from the exact g = A'b, step = g'g / |A g|^2 and
    the backend's Newton step dx_n.

    First-order propagation of the derived relative errors, doubled for the second-order terms:
      eta   = gamma_m || |A'||b| ||_2                 the error of the device's g (an inner product of at most m terms)
      r_gg  = gamma_k_dot + 2 eta / |g|               g'g
      r_ag  = gamma_k_ax + 2 eta |A'A g| / |A g|^2    |A g|^2: |A (g + dg)|^2 - |A g|^2 = 2 dg'(A'A g) to first order
      step  = gg / ag2: r_gg + r_ag + u;  uu = step^2 gg: 2 r_step + r_gg + 2 u;  nn: gamma_k_dot;
      un = step g'dx_n: absolute (gamma_k_dot sum|g dx_n| + eta |dx_n|) step + |un| (r_step + u).
    'steepest' (radius^2 < uu): the point is radius g / |g| whatever the step: coefficient sqrt(radius^2 / uu) step, seven
      roundings and half of r_gg's reduction part; direction error eta / |g|.
    'newton' (radius^2 >= nn): 0 g + 1 dx_n — exact, the bound is 0.
    'dogleg': tau solves uu (1 - tau)^2 + 2 un tau (1 - tau) + nn tau^2 = radius^2; d tau by implicit differentiation plus
      the float64 quadratic formula's own roundings (twelve, the cancellation in -b + sqrt(..) amplified by
      (|b| + sq) / |sq - |b||)."""
    u = LD(U)
    g = S.g
    dx_n = np.asarray(dx_n, LD)
    gg, ag2 = S.gg, S.ax2(g)
    step = gg / ag2
    uu, nn, un = step * step * gg, np.dot(dx_n, dx_n), step * np.dot(g, dx_n)
    gn = np.sqrt(gg)
    eta = bound(S.m) * u * _norm(S.absg)
    r_gg = bound(k_dot) * u + 2 * eta / gn
    r_ag = bound(k_ax) * u + 2 * eta * _norm(S.times(g)) / ag2
    r_step = r_gg + r_ag + u
    rsq = LD(radius) * LD(radius)
    if rsq < uu:
        point = LD(radius) * g / gn
        b = LD(radius) * (2 * eta / gn + (bound(k_dot) / 2 + 8) * u)
        return "steepest", point, 2 * b, (uu, nn)
    if rsq >= nn:
        return "newton", dx_n.copy(), LD(0), (uu, nn)
    a, b, c = uu - 2 * un + nn, 2 * (un - uu), uu - rsq
    sq = np.sqrt(b * b - 4 * a * c)
    t1, t2 = (-b + sq) / (2 * a), (-b - sq) / (2 * a)
    tau = t1 if 0 <= t1 <= 1 else t2
    assert 0 <= tau <= 1, tau
    d_uu = uu * (2 * r_step + r_gg + 2 * u)
    d_nn = nn * bound(k_dot) * u
    d_un = step * (bound(k_dot) * u * np.dot(np.abs(g), np.abs(dx_n)) + eta * np.sqrt(nn)) + np.abs(un) * (r_step + u)
    dF = np.abs(-2 * uu * (1 - tau) + 2 * un * (1 - 2 * tau) + 2 * nn * tau)
    d_tau = ((1 - tau) ** 2 * d_uu + 2 * tau * (1 - tau) * d_un + tau ** 2 * d_nn) / dF
    amp = (np.abs(b) + sq) / np.abs(sq - np.abs(b))
    d_tau += np.abs(tau) * (12 * amp) * u
    point = (1 - tau) * step * g + tau * dx_n
    err = d_tau * (step * gn + np.sqrt(nn)) + (1 - tau) * step * (gn * (r_step + 2 * u) + eta) + 3 * u * _norm(point)
    return "dogleg", point, 2 * err, (uu, nn)
