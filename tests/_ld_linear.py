"""The extended-precision judge of elimination, solve and marginals (host only, no GPU, no oracle).

A backend (the CPU oracle or the device: anything with get_tree / conditional / solve / arrays) eliminates the whitened
rows [A b] of a linearization into a Bayes tree of conditionals [R S d].  Stacked, the conditionals are the rows of the
Cholesky factor of the damped system

    Hd = A'A + lambda D,     D = I  or  clamp(diag A'A),     g = A'b,

so whatever kernels produced them, the following hold for a backward-stable float64 implementation, with every product
formed here in numpy.longdouble (64-bit significand) from the float64 data:

  (1) factor   |R'R - Hd|   <= gamma (|R'||R| + |A'||A| + lambda |D|)     componentwise; R upper triangular
  (2) rhs      |R'd - g|    <= gamma (|R'||d| + |A'||b|)                   componentwise
  (3) solve    |Hd x - g|   <= gamma ((|R'||R| + |A'||A| + lambda |D|)|x| + |A'||b|)   for x = solve(lambda, diag)
  (4) forward  ||x - x*||_2 <= gamma kappa_2(Hd) ||x*||_2,   max|S - S*| <= gamma kappa_2(H) max|S*|

x* and S* = H^-1 are float64 results refined with longdouble residuals until the correction is below 1e-18 relative —
or, where kappa_2 eps_longdouble is above that (kappa_2 of more than a few tens), until it stalls below 1e-3 u kappa_2
(_converged): the reference is then good to a thousandth of the unit (4) is measured in, no better.  The pin against
mpmath (test_host_linear_judge.py) covers n <= 40 at small kappa_2 only.
The bounds are backward-error bounds: they do not depend on the conditioning of the problem (4 carries kappa_2
explicitly) nor on the rounding of a second implementation.  gamma = k u, u = 2^-53; k_factor / k_solve below derive k.

VectorJudge (below) takes measures (2) and (3) with the same bounds and k without ever forming an n x n array, for systems
of several thousand scalars.

Everything is kept in VARIABLE coordinates (scalar i of variable v at tangent_offsets[v] + i, the layout of solve()'s
result); gather() also returns the elimination order of the scalars, in which R is upper triangular.
"""
import numpy as np

LD = np.longdouble
# The judge is only a judge with a significand longer than float64's: x87 extended (eps 2^-63) or better.  A platform
# whose long double is double must not pass quietly.
assert np.finfo(LD).eps <= 2.0 ** -63, (
    "tests/_ld_linear.py needs numpy.longdouble with eps <= 2^-63 (x87 extended or binary128); this platform's is %r"
    % (np.finfo(LD).eps,))

U = 2.0 ** -53


def k_factor(m, n):
    """k of measures (1) and (2), from m = the longest accumulation of whitened rows into one entry of A'A (the largest
    number of rows that touch one scalar, a diagonal entry collects them all) and n = the number of scalars.

    Forming Hd in float64: an entry of A'A is an inner product of at most m terms, |fl(x'y) - x'y| <= gamma_m |x|'|y| for
    ANY order of summation (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., (3.5)); the damping term adds
    one addition, the product lambda d one rounding, d itself (a diagonal entry, clamped) gamma_m relative, and the
    reference's sqrt(lambda) sqrt(d) rows, squared again by the elimination, three more: (m + 5) u (|A'||A| + lambda |D|).
    Cholesky of that matrix: |R'R - Hd^| <= gamma_(n+1) |R'||R| (Higham Theorem 10.3; the proof counts the at most n - 1
    products, one subtraction chain and one division behind an entry, in any order).  The kernels multiply by a computed
    reciprocal where the theorem divides (one more rounding per entry) and take the pivot as d * rsqrt(d) from a refined
    seed (error of the refined 1/sqrt(d) at most 2 u, one more for the product): (n + 5) u |R'||R|.
    The right-hand side is column n + 1 of the same factorization, so (2) has the same two terms with b for A and d for R.
    The sum (m + 5) + (n + 5) bounds either coefficient; twice that figure covers the second-order terms and the
    difference between the exact and the computed |R|:   k = 2 (m + n + 10)."""
    return 2 * (m + n + 10)


def k_solve(m, n):
    """k of measures (3) and (4).  With x the computed solution of R x = d:  (R + E) x = d, |E| <= gamma_n |R| for any
    order of summation (Higham Theorem 8.5), one more u per entry for the multiplication by the reciprocal pivot:
    |R x - d| <= (n + 1) u |R||x|.  Then
        Hd x - g = (Hd - R'R) x + R'(R x - d) + (R'd - g),
    and with (1), (2) and |d| <= |R||x| + |R x - d|:
        |Hd x - g| <= [(m + 5)(|A'||A| + lambda|D|) + ((n + 5) + (n + 1) + (n + 5)) |R'||R|] u |x| + (m + 5) u |A'||b|,
    every coefficient at most m + 3 n + 16; twice that:   k = 2 (m + 3 n + 16).
    A marginal block is a block of R^-1 R^-T: the same factor and two triangular solves per column, so its forward error
    is kappa_2 times the same backward error (Higham Theorem 7.2 applied to (3) read as a perturbed system): the same k."""
    return 2 * (m + 3 * n + 16)


class LinearSystem:
    """Hd, |A'||A|, g, |A'||b| of one linearization in longdouble, formed factor block by factor block from the float64
    [A b] that jacobians() returned (a dense A'A in longdouble costs minutes; the blocks take well under a second)."""

    def __init__(self, arrays, jac):
        self.arrays = arrays
        self.off = np.asarray(arrays.tangent_offsets(), dtype=np.int64)
        self.n = n = int(self.off[-1])
        joff = arrays.jacobian_offsets()
        self.blocks = []                      # (scalar indices, A_f, b_f) per factor
        self.H = np.zeros((n, n), LD)
        self.absH = np.zeros((n, n), LD)
        self.g = np.zeros(n, LD)
        self.absg = np.zeros(n, LD)
        rows = np.zeros(n, np.int64)
        for f in range(arrays.n_factors):
            vs = arrays.f_vars[arrays.f_key_ptr[f]:arrays.f_key_ptr[f + 1]]
            m = int(arrays.f_rows[f])
            if m == 0 or len(vs) == 0:
                continue
            idx = np.concatenate([np.arange(self.off[v], self.off[v + 1]) for v in vs])
            assert len(set(idx.tolist())) == idx.size, "a factor names a variable twice"
            Ab = np.asarray(jac[joff[f]:joff[f + 1]], dtype=np.float64).reshape(idx.size + 1, m).T.astype(LD)
            A, b = Ab[:, :-1], Ab[:, -1]
            self.blocks.append((idx, A, b))
            ix = np.ix_(idx, idx)
            self.H[ix] += np.dot(A.T, A)
            self.absH[ix] += np.dot(np.abs(A).T, np.abs(A))
            self.g[idx] += np.dot(A.T, b)
            self.absg[idx] += np.dot(np.abs(A).T, np.abs(b))
            rows[idx] += m
        self.m = int(rows.max()) + 1          # + 1: the damping row of that scalar

    def damping(self, lam, diag, min_diagonal=1e-6, max_diagonal=1e32):
        """lambda D as a vector: D = I or the clamped diagonal of A'A (gsx_solve's rule)."""
        if not lam > 0:
            return np.zeros(self.n, LD)
        d = np.clip(np.diag(self.H), LD(min_diagonal), LD(max_diagonal)) if diag else np.ones(self.n, LD)
        return LD(lam) * d

    def damped(self, lam, diag, limits=(1e-6, 1e32)):
        Hd = self.H.copy()
        Hd[np.diag_indices(self.n)] += self.damping(lam, diag, *limits)
        return Hd

    def times(self, x, lam=0.0, diag=False, limits=(1e-6, 1e32)):
        """Hd x from the factor blocks."""
        x = np.asarray(x, LD)
        y = self.damping(lam, diag, *limits) * x
        for idx, A, _ in self.blocks:
            y[idx] += np.dot(A.T, np.dot(A, x[idx]))
        return y


class Factor:
    """What gather() returns: R (n x n) and d in variable coordinates, the scalars in elimination order, and R'R, |R'||R|
    summed clique by clique (rows of different cliques share no product: sum over cliques of [R S]'[R S] on the clique's
    columns, which costs the flops of the factorization, not n^3)."""

    def __init__(self, R, d, order, cliques):
        self.R, self.d, self.order = R, d, order
        n = R.shape[0]
        self.RtR = np.zeros((n, n), LD)
        self.aRtaR = np.zeros((n, n), LD)
        for cols, W in cliques:
            ix = np.ix_(cols, cols)
            self.RtR[ix] += np.dot(W.T, W)
            self.aRtaR[ix] += np.dot(np.abs(W).T, np.abs(W))


def gather(backend, system):
    """The conditionals [R S d] of every clique of the backend's Bayes tree scattered into one n x n matrix and one vector
    (variable coordinates), with the scalars in elimination order (children before parents, frontals in the clique's
    order): R[order][:, order] is upper triangular."""
    parent, fronts = backend.get_tree()
    off, n = system.off, system.n
    R = np.zeros((n, n), LD)
    d = np.zeros(n, LD)
    seen = np.zeros(n, bool)
    depth = []
    for c in range(len(fronts)):
        k, p = 0, parent[c]
        while p >= 0:
            k, p = k + 1, parent[p]
        depth.append(k)
    order, cliques = [], []
    for c in sorted(range(len(fronts)), key=lambda c: -depth[c]):
        fv, sv = fronts[c]
        fi = np.concatenate([np.arange(off[v], off[v + 1]) for v in fv])
        si = np.concatenate([np.arange(off[v], off[v + 1]) for v in sv]) if len(sv) else np.zeros(0, np.int64)
        # a separator variable is a frontal variable of an ancestor
        anc, p = set(), parent[c]
        while p >= 0:
            anc.update(fronts[p][0])
            p = parent[p]
        assert set(sv) <= anc, ("clique", c, "separator outside its ancestors")
        RSd = np.asarray(backend.conditional(c), dtype=np.float64)
        assert RSd.shape == (fi.size, fi.size + si.size + 1), (c, RSd.shape, fi.size, si.size)
        assert not seen[fi].any(), "a variable is frontal in two cliques"
        seen[fi] = True
        cols = np.concatenate([fi, si])
        R[np.ix_(fi, cols)] = RSd[:, :-1]
        d[fi] = RSd[:, -1]
        order.extend(fi.tolist())
        cliques.append((cols, RSd[:, :-1].astype(LD)))
    assert seen.all(), "a variable is frontal in no clique"
    return Factor(R, d, np.asarray(order, np.int64), cliques)


def _ratio(lhs, rhs):
    """max |lhs| / (u rhs); infinite where rhs is exactly 0 and lhs is not."""
    lhs, rhs = np.abs(np.asarray(lhs, LD)), np.asarray(rhs, LD)
    if np.any((rhs == 0) & (lhs != 0)) or not np.all(np.isfinite(lhs)):
        return float("inf")
    pos = rhs > 0
    return float(np.max(lhs[pos] / rhs[pos]) / LD(U)) if pos.any() else 0.0


def factor_ratio(system, F, lam, diag, limits=(1e-6, 1e32)):
    """Measure (1) in units of u; infinite when a structural zero is not zero: an entry of R below the diagonal (in
    elimination order), or a difference where the bound is exactly 0."""
    if np.any(np.tril(F.R[np.ix_(F.order, F.order)], -1) != 0):
        return float("inf")
    bound = F.aRtaR + system.absH
    bound[np.diag_indices(system.n)] += system.damping(lam, diag, *limits)
    return _ratio(F.RtR - system.damped(lam, diag, limits), bound)


def rhs_ratio(system, F):
    """Measure (2) in units of u."""
    return _ratio(np.dot(F.R.T, F.d) - system.g, np.dot(np.abs(F.R).T, np.abs(F.d)) + system.absg)


def solve_ratio(system, F, x, lam, diag, limits=(1e-6, 1e32)):
    """Measure (3) in units of u."""
    ax = np.abs(np.asarray(x, LD))
    bound = np.dot(F.aRtaR, ax) + np.dot(system.absH, ax) + system.damping(lam, diag, *limits) * ax + system.absg
    return _ratio(system.times(x, lam, diag, limits) - system.g, bound)


def _converged(rel, prev, kappa, what):
    """The refinement stops when the correction is below 1e-18 relative.  A residual formed with a 64-bit significand cannot
    push it there once kappa_2 eps_longdouble exceeds 1e-18 (kappa_2 of a few tens): then it stops when the correction no
    longer halves, and must by then be below 1e-3 u kappa_2 — a thousandth of the unit measure (4) is expressed in."""
    if rel <= 1e-18:
        return True
    if prev is not None and rel >= 0.5 * prev:
        assert rel <= 1e-3 * U * kappa, (what, "refinement stalled at", rel, "kappa", kappa)
        return True
    return False


def _block_rows(M, off):
    """Per variable block row of M: (rows, columns of its non-zero blocks) — M X then costs the non-zeros of a sparse H
    (bundle adjustment: 5 x fewer longdouble products), and no more than the dense product when H is dense."""
    nz = np.add.reduceat(np.add.reduceat((M != 0).astype(np.int64), off[:-1], 0), off[:-1], 1) > 0
    out = []
    for i in range(len(off) - 1):
        cols = np.concatenate([np.arange(off[j], off[j + 1]) for j in np.nonzero(nz[i])[0]])
        out.append((np.arange(off[i], off[i + 1]), cols))
    return out


def refined_inverse(M, off=None):
    """(M^-1 in longdouble, kappa_2(M)): the float64 inverse X0, then X <- X + X0 (I - M X) with the residual in longdouble
    until the correction is below 1e-18 max|X| (see _converged).  off: the variables' offsets (block sparsity of M)."""
    M64 = np.asarray(M, np.float64)
    rows = _block_rows(M, off) if off is not None else [(np.arange(M.shape[0]), np.arange(M.shape[0]))]
    X0 = np.linalg.inv(M64)
    kappa = float(np.linalg.cond(M64))
    X = X0.astype(LD)
    eye = np.eye(M.shape[0], dtype=LD)
    prev = None
    for _ in range(12):
        res = eye.copy()
        for r, c in rows:
            res[r] -= np.dot(M[np.ix_(r, c)], X[c])
        corr = np.dot(X0, res.astype(np.float64)).astype(LD)   # the correction itself needs no more than float64
        X += corr
        rel = float(np.max(np.abs(corr)) / np.max(np.abs(X)))
        if _converged(rel, prev, kappa, "inverse"):
            return X, kappa
        prev = rel
    raise AssertionError("the refinement of the inverse did not converge")


def refined_solve(system, lam, diag):
    """(x*, kappa_2(Hd)): the float64 solution of Hd x = g refined with longdouble residuals until the correction is below
    1e-18 ||x|| (see _converged)."""
    Hd = system.damped(lam, diag)
    H64 = Hd.astype(np.float64)
    kappa = float(np.linalg.cond(H64))
    X0 = np.linalg.inv(H64)
    x = np.dot(X0, system.g.astype(np.float64)).astype(LD)
    prev = None
    for _ in range(12):
        res = system.g - np.dot(Hd, x)
        corr = np.dot(X0, res.astype(np.float64)).astype(LD)
        x += corr
        rel = float(np.linalg.norm(corr.astype(np.float64)) / np.linalg.norm(x.astype(np.float64)))
        if _converged(rel, prev, kappa, "step"):
            return x, kappa
        prev = rel
    raise AssertionError("the refinement of the step did not converge")


def step_ratio(x, xstar, kappa):
    """Measure (4) for the step, in units of u kappa_2."""
    e = np.asarray(x, LD) - xstar
    return float(np.sqrt(np.dot(e, e)) / np.sqrt(np.dot(xstar, xstar)) / LD(U) / LD(kappa))


def covariance_ratio(block, star_block, star_max, kappa):
    """Measure (4) for a covariance block, in units of u kappa_2, against max|S*| over the whole inverse."""
    return float(np.max(np.abs(np.asarray(block, LD) - star_block)) / star_max / LD(U) / LD(kappa))


class Judge:
    """One linearization under judgement: the system, its k, and the refined x* / S* computed once and kept."""

    def __init__(self, arrays, jac):
        self.sys = LinearSystem(arrays, jac)
        self.kf = k_factor(self.sys.m, self.sys.n)
        self.ks = k_solve(self.sys.m, self.sys.n)
        self._star = {}
        self._sigma = None

    def backward(self, backend, x, lam, diag, limits=(1e-6, 1e32)):
        """(factor, rhs, solve) ratios in u for the backend's conditionals, taken as the factorization at (lam, diag);
        limits = (min_diagonal, max_diagonal) of the diagonal damping's clamp."""
        F = gather(backend, self.sys)
        return (factor_ratio(self.sys, F, lam, diag, limits), rhs_ratio(self.sys, F),
                solve_ratio(self.sys, F, x, lam, diag, limits))

    def check_backward(self, backend, x, lam, diag, what, limits=(1e-6, 1e32)):
        f, r, s = self.backward(backend, x, lam, diag, limits)
        print(f"{what} lam={lam:g} diag={int(diag)} n={self.sys.n} m={self.sys.m}: factor {f:.2f}u (k {self.kf}), "
              f"rhs {r:.2f}u (k {self.kf}), solve {s:.2f}u (k {self.ks})")
        assert f <= self.kf, (what, "factor", lam, diag, f, self.kf)
        assert r <= self.kf, (what, "rhs", lam, diag, r, self.kf)
        assert s <= self.ks, (what, "solve", lam, diag, s, self.ks)
        return f, r, s

    def check_step(self, x, lam, diag, what):
        key = (float(lam), bool(diag))
        if key not in self._star:
            self._star[key] = refined_solve(self.sys, lam, diag)
        xs, kappa = self._star[key]
        r = step_ratio(x, xs, kappa)
        print(f"{what} lam={lam:g} diag={int(diag)}: step {r:.3f} u*kappa (kappa {kappa:.1f}, k {self.ks})")
        assert r <= self.ks, (what, "step", lam, diag, r, self.ks)
        return r

    def sigma(self):
        if self._sigma is None:
            S, kappa = refined_inverse(self.sys.H, self.sys.off)
            self._sigma = (S, kappa, np.max(np.abs(S)))
        return self._sigma

    def var_index(self, key):
        return int(np.searchsorted(self.sys.arrays.var_keys, np.uint64(key)))

    def check_covariance(self, keys, block, what):
        """A marginal (one key) or joint (several keys, blocks in that order) covariance against S*."""
        S, kappa, smax = self.sigma()
        off = self.sys.off
        idx = np.concatenate([np.arange(off[v], off[v + 1]) for v in (self.var_index(k) for k in keys)])
        block = np.asarray(block)
        assert block.shape == (idx.size, idx.size), (what, keys, block.shape)
        r = covariance_ratio(block, S[np.ix_(idx, idx)], smax, kappa)
        assert r <= self.ks, (what, "covariance", keys, r, self.ks)
        return r


# ---- the same measures (2) and (3) without an n x n array: for systems too large for the dense judge -------------------------
def gather_cliques(backend, off, n):
    """[(frontal scalars, column scalars, [R S] in longdouble, d in longdouble)] per clique, variable coordinates.  Rows
    of different cliques share no product, so R'v and |R|'|R||x| are sums over this list (the order does not matter)."""
    parent, fronts = backend.get_tree()
    seen = np.zeros(n, bool)
    out = []
    for c, (fv, sv) in enumerate(fronts):
        fi = np.concatenate([np.arange(off[v], off[v + 1]) for v in fv])
        si = np.concatenate([np.arange(off[v], off[v + 1]) for v in sv]) if len(sv) else np.zeros(0, np.int64)
        RSd = np.asarray(backend.conditional(c), dtype=np.float64)
        assert RSd.shape == (fi.size, fi.size + si.size + 1), (c, RSd.shape, fi.size, si.size)
        assert not seen[fi].any(), "a variable is frontal in two cliques"
        seen[fi] = True
        assert np.all(np.tril(RSd[:, :fi.size], -1) == 0), ("clique", c, "R is not upper triangular")
        out.append((fi, np.concatenate([fi, si]), RSd[:, :-1].astype(LD), RSd[:, -1].astype(LD)))
    assert seen.all(), "a variable is frontal in no clique"
    return out


class VectorJudge:
    """Measures (2) and (3) with the bounds and the k of Judge, every product a vector: R'd and |R'||d| summed clique by
    clique, Hd x, |A'||A||x|, g, |A'||b| and the diagonal of A'A (the damping) summed factor by factor, in longdouble."""

    def __init__(self, arrays, jac):
        self.arrays = arrays
        self.off = np.asarray(arrays.tangent_offsets(), dtype=np.int64)
        self.n = n = int(self.off[-1])
        joff = arrays.jacobian_offsets()
        self.blocks = []
        self.g = np.zeros(n, LD)
        self.absg = np.zeros(n, LD)
        self.diagH = np.zeros(n, LD)
        rows = np.zeros(n, np.int64)
        for f in range(arrays.n_factors):
            vs = arrays.f_vars[arrays.f_key_ptr[f]:arrays.f_key_ptr[f + 1]]
            m = int(arrays.f_rows[f])
            if m == 0 or len(vs) == 0:
                continue
            idx = np.concatenate([np.arange(self.off[v], self.off[v + 1]) for v in vs])
            assert len(set(idx.tolist())) == idx.size, "a factor names a variable twice"
            Ab = np.asarray(jac[joff[f]:joff[f + 1]], dtype=np.float64).reshape(idx.size + 1, m).T.astype(LD)
            A, b = Ab[:, :-1], Ab[:, -1]
            self.blocks.append((idx, A, b))
            self.g[idx] += np.dot(A.T, b)
            self.absg[idx] += np.dot(np.abs(A).T, np.abs(b))
            self.diagH[idx] += np.sum(A * A, axis=0)
            rows[idx] += m
        self.m = int(rows.max()) + 1          # + 1: the damping row of that scalar (as LinearSystem.m)
        self.kf = k_factor(self.m, self.n)
        self.ks = k_solve(self.m, self.n)

    def damping(self, lam, diag, min_diagonal=1e-6, max_diagonal=1e32):
        if not lam > 0:
            return np.zeros(self.n, LD)
        d = np.clip(self.diagH, LD(min_diagonal), LD(max_diagonal)) if diag else np.ones(self.n, LD)
        return LD(lam) * d

    def backward(self, backend, x, lam, diag):
        """(rhs, solve) ratios in u."""
        n = self.n
        cliques = gather_cliques(backend, self.off, n)
        x = np.asarray(x, LD)
        ax = np.abs(x)
        Rtd, aRtad, aRtaRx = np.zeros(n, LD), np.zeros(n, LD), np.zeros(n, LD)
        for fi, cols, W, d in cliques:
            aW = np.abs(W)
            Rtd[cols] += np.dot(W.T, d)
            aRtad[cols] += np.dot(aW.T, np.abs(d))
            aRtaRx[cols] += np.dot(aW.T, np.dot(aW, ax[cols]))
        damp = self.damping(lam, diag)
        Hx, aHax = damp * x, damp * ax
        for idx, A, _ in self.blocks:
            aA = np.abs(A)
            Hx[idx] += np.dot(A.T, np.dot(A, x[idx]))
            aHax[idx] += np.dot(aA.T, np.dot(aA, ax[idx]))
        return _ratio(Rtd - self.g, aRtad + self.absg), _ratio(Hx - self.g, aRtaRx + aHax + self.absg)

    def check_backward(self, backend, x, lam, diag, what):
        r, s = self.backward(backend, x, lam, diag)
        print(f"{what} lam={lam:g} diag={int(diag)} n={self.n} m={self.m}: rhs {r:.2f}u (k {self.kf}), "
              f"solve {s:.2f}u (k {self.ks})")
        assert r <= self.kf, (what, "rhs", lam, diag, r, self.kf)
        assert s <= self.ks, (what, "solve", lam, diag, s, self.ks)
        return r, s
