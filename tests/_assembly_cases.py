"""Hessian assembly, panel by panel: the cases that reach every kernel class of upload.hip's "H assembly groups", and the
extended-precision judge of a panel (host only, no GPU, no oracle).

The panel of variable A under an elimination ordering (banner above assemble_h_kernel, kernels.hip): rows = A's own
scalars, then the scalars of its later-eliminated neighbours in elimination order, then the right-hand side; with
[A_1 .. A_n b] the whitened block of a factor that holds A,

    panel[rows of B, :] = sum over the factors holding A and B of  A_B' A_A        panel[last row, :] = sum  b' A_A.

expected_panel() forms exactly that in numpy.longdouble from the float64 [A b] blocks of gsx_get_jacobians, never
looking at a term list.  restated_panel() is the other road: the term lists of symbolic.cpp and the chunking of the heavy
kernel restated in float64, used only by the host test to show that the judge notices a wrong term (MUTATIONS).

Two data sets per case (DATA):

  int    unit noise, entries of [A b] small integers, |a| <= 8: every product and every sum is an integer far below 2^53,
         exact in float64 in any order and on the matrix cores: the device panel must EQUAL the expected one.
  real   normal entries, the factors' scales spread over six decades, diagonal sigmas: judged componentwise by

             |got - exact| <= gamma_k (|A_B|' |A_A|),     gamma_k = k u,  u = 2^-53.

k is DERIVED from the kernels' code, nothing is measured to set it.  An entry is a sum of products a_r b_r, one per factor
row behind it; a product that passes through j roundings on its way to the stored entry carries (1 + delta)^j, and j is at
most the number of roundings of the whole accumulation (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.,
(3.5): any order of summation).  So k = (rows accumulated behind the entry, as the kernel pads them) + (additions of
partial sums: one per term into the panel, one per copy or wave); a fused multiply-add only removes roundings.  With
R = the rows of the factors behind the entry and T = the terms (block products) behind it (kernels.hip):

  light   assemble_h_kernel, one wave: acc = a0 b0 + a1 b1, += a_r b_r (:1532-1543), panel += acc per term (:1546), the
          store adds the one LDS copy to 0 (:1553-1555)                                                   k = R + T + 1
  heavy   the same kernel, four waves with a contiguous chunk of terms each; the store adds the four copies in wave
          order (:1554)                                                                                   k = R + T + 4
  huge    assemble_h_global_kernel: acc += per row (:1652), panel += acc per term (:1653)                 k = R + T
  tile    assemble_h_tile_kernel: per factor two v_mfma_f64_16x16x4 over rows 0-3 and 4-7, absent rows as zeros
          (:1599-1600, :1612-1613): 8 row slots a factor whatever its rows; panel += g per term (:1623)    k = 8 T + T
  diag    assemble_h_diag_body: a v_mfma_f64_16x16x4 per four row slots, a factor of m rows takes 4 ceil(m / 4) slots
          (two 2-row factors may share one: fewer) (:1703-1733); the four waves' tiles are added in wave order
          (:1743)                                                                                         k = R4 + 4
  star    assemble_h_star_kernel and assemble_h_star_bundle_body through star_entry / star_accum (:1756-1769): a
          partner-block entry is one factor's inner product; an own-block or rhs entry adds every factor's rows to a
          running sum                                                                                     k = R + T
          (front_star_leaf_kernel forms the same entries with the same two helpers: same bits.)

worst_ratio() returns max |got - exact| / (u |A_B|'|A_A|) so that the tests can print it next to k.
"""
import numpy as np

from gtsam_petercdev_amd import _abi as A
from gtsam_petercdev_amd.graph import GaussianFactorGraph, JacobianFactor, noiseModel

from tests._ld_linear import LD, U

DATA = ("int", "real")
TILE, LIGHT, HEAVY, HUGE, STAR, DIAG = A.H_TILE, A.H_LIGHT, A.H_HEAVY, A.H_HUGE, A.H_STAR, A.H_DIAG
NAMES = A.HESSIAN_CLASS_NAMES
COPIES = {LIGHT: 1, HEAVY: 4, HUGE: 0, TILE: 0, DIAG: 4, STAR: 0}


class Case:
    """dims: the variables' dimensions, eliminated in index order.  factors: (variables, rows) in graph order; `ids` names
    each factor's data stream, so that two cases sharing factors share their numbers.  expect: {variable: class} of the
    variables the case was built for; bundles: {star variable: bundle size} (0 = the group runs unbundled);
    group_size: {variable: number of variables in its launch group}; same_group: variables that must share a group;
    fused: whether a handle without star leaves (GSX_FUSED_STAR=0) launches diag and star fused."""

    def __init__(self, name, dims, factors, expect, bundles=None, group_size=None, same_group=None, fused=False, ids=None,
                 seed=0):
        self.name, self.dims, self.factors, self.expect = name, list(dims), [(tuple(v), int(m)) for v, m in factors], expect
        self.bundles, self.group_size, self.same_group, self.fused = bundles or {}, group_size or {}, same_group, fused
        self.ids = list(range(len(self.factors))) if ids is None else list(ids)
        self.seed = seed
        self.ordering = list(range(len(self.dims)))
        assert len(self.factors) <= 400 and len(self.dims) <= 80, name
        assert {v for vs, _ in self.factors for v in vs} == set(range(len(dims))), name

    @property
    def is_star_case(self):
        return any(c == STAR for c in self.expect.values()) or self.name.startswith("star")

    def arrays(self, data):
        """The graph as JacobianFactor slots on vector variables (keys = indices), values zero."""
        fg = GaussianFactorGraph()
        for (vs, m), fid in zip(self.factors, self.ids):
            rng = np.random.default_rng([1234 + self.seed, fid, DATA.index(data)])
            cols = sum(self.dims[v] for v in vs) + 1
            if data == "int":
                Ab, model = rng.integers(-8, 9, (m, cols)).astype(float), None
            else:
                scale = 10.0 ** (-3.0 + 6.0 * ((fid * 5) % 13) / 12.0)       # six decades across the factors
                Ab = scale * rng.normal(size=(m, cols))
                model = noiseModel.Diagonal.Sigmas(0.5 + 1.5 * rng.random(m), smart=False)
            args, c = [], 0
            for v in vs:
                args += [v, Ab[:, c:c + self.dims[v]]]
                c += self.dims[v]
            args.append(Ab[:, c])
            if model is not None:
                args.append(model)
            fg.add(JacobianFactor(*args))
        arr = fg.to_arrays(None)
        assert list(arr.var_keys) == self.ordering and list(arr.var_dims) == self.dims, self.name
        arr.values = np.zeros(int(arr.var_dims.sum()))
        return arr


def host_jacobians(arr):
    """What gsx_get_jacobians returns for these graphs (linear factors at zero values): the rows of [A b] over their
    sigmas.  For the host test, which has no device to ask."""
    off = arr.jacobian_offsets()
    out = np.zeros(int(off[-1]))
    for f in range(arr.n_factors):
        m = int(arr.f_rows[f])
        Ab = np.array(arr.meas[arr.f_meas_ptr[f]:arr.f_meas_ptr[f + 1]]).reshape(-1, m).T
        kind = int(arr.f_noise_kind[f])
        p = arr.noise[arr.f_noise_ptr[f]:arr.f_noise_ptr[f + 1]]
        assert kind in (A.NOISE_UNIT, A.NOISE_DIAGONAL)
        if kind == A.NOISE_DIAGONAL:
            Ab = Ab / p[:, None]
        out[off[f]:off[f + 1]] = Ab.T.reshape(-1)
    return out


# ---- the judge ----------------------------------------------------------------------------------------------------------
class Panel:
    """exact[rows, dim] and mag = |A_B|'|A_A| in longdouble; R, T, R4 per entry (module docstring); row_var, row_scalar."""


def _blocks(arr, jac, f):
    """[A b] of factor f as a float64 m x cols array and the column of every variable in it."""
    off = arr.jacobian_offsets()
    m = int(arr.f_rows[f])
    vs = [int(v) for v in arr.f_vars[arr.f_key_ptr[f]:arr.f_key_ptr[f + 1]]]
    Ab = np.asarray(jac[off[f]:off[f + 1]], float).reshape(-1, m).T
    col, c = {}, 0
    for v in vs:
        col[v] = c
        c += int(arr.var_dims[v])
    return Ab, vs, col


def expected_panel(arr, jac, var, ordering=None):
    """The panel of variable `var` (an index) from the [A b] blocks `jac`, straight from the definition.  ordering: the
    elimination order as variable indices (default: index order)."""
    pos = np.arange(arr.n_vars) if ordering is None else np.argsort(np.asarray(ordering))
    d = int(arr.var_dims[var])
    mine = [f for f in range(arr.n_factors) if var in arr.f_vars[arr.f_key_ptr[f]:arr.f_key_ptr[f + 1]]]
    later = sorted({int(u) for f in mine for u in arr.f_vars[arr.f_key_ptr[f]:arr.f_key_ptr[f + 1]] if pos[u] > pos[var]},
                   key=lambda u: pos[u])
    row0, r = {var: 0}, d
    for u in later:
        row0[u] = r
        r += int(arr.var_dims[u])
    rows = r + 1
    p = Panel()
    p.exact, p.mag = np.zeros((rows, d), LD), np.zeros((rows, d), LD)
    p.R, p.T, p.R4 = (np.zeros((rows, d), np.int64) for _ in range(3))
    for f in mine:
        Ab, vs, col = _blocks(arr, jac, f)
        m = Ab.shape[0]
        AA = Ab[:, col[var]:col[var] + d].astype(LD)
        for u, r0, du in [(u, row0[u], int(arr.var_dims[u])) for u in vs if u in row0] + [(-1, rows - 1, 1)]:
            c0 = col[u] if u >= 0 else Ab.shape[1] - 1
            AB = Ab[:, c0:c0 + du].astype(LD)
            p.exact[r0:r0 + du] += AB.T @ AA
            p.mag[r0:r0 + du] += np.abs(AB).T @ np.abs(AA)
            p.R[r0:r0 + du] += m
            p.T[r0:r0 + du] += 1
            p.R4[r0:r0 + du] += 4 * (-(-m // 4))
    p.row_var = np.array([u for u in [var] + later for _ in range(int(arr.var_dims[u]))] + [-1])
    p.row_scalar = np.array([k for u in [var] + later for k in range(int(arr.var_dims[u]))] + [0])
    return p


def k_of(cls, p):
    """The derived k of every entry of a panel assembled by class `cls` (module docstring)."""
    if cls == TILE:
        return 8 * p.T + p.T
    if cls == DIAG:
        return p.R4 + 4
    return p.R + p.T + COPIES[cls]


def worst_ratio(got, p):
    """max over the entries of |got - exact| / (u |A_B|'|A_A|), and the ratio of that entry to its k = 1 unit; an entry
    with nothing behind it must be exactly zero."""
    err = np.abs(np.asarray(got, float).astype(LD) - p.exact)
    assert np.all(err[p.mag == 0] == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(p.mag > 0, err / (LD(U) * p.mag), 0)


def judge(got, p, cls, data):
    """(ok, worst ratio / k over the entries, largest k).  int: equality; real: the gamma_k bound."""
    got = np.asarray(got, float)
    if got.shape != p.exact.shape:
        return False, np.inf, 0
    k = k_of(cls, p)
    ratio = worst_ratio(got, p)
    if data == "int":
        return bool(np.array_equal(got.astype(LD), p.exact)), float(np.max(ratio)), int(k.max())
    return bool(np.all(ratio <= k)), float(np.max(ratio)), int(k.max())


# ---- the restatement through the term lists (host test only) -------------------------------------------------------------
MUTATIONS = ("drop_last_of_64", "partner_at_neighbour_rows", "rhs_from_previous_factor", "skip_wave_chunk")


def restated_panel(arr, jac, var, ordering=None, waves=4, mutation=None):
    """The panel in float64 the way the heavy kernel goes about it: the term list of symbolic.cpp (per factor: own block,
    every later variable of the factor in the factor's order, rhs), split in `waves` contiguous chunks rounded up to even,
    a copy per wave, the copies added in wave order.  mutation: one of MUTATIONS."""
    pos = np.arange(arr.n_vars) if ordering is None else np.argsort(np.asarray(ordering))
    d = int(arr.var_dims[var])
    ref = expected_panel(arr, jac, var, ordering)
    rows = ref.exact.shape[0]
    row0 = {int(u): int(np.flatnonzero((ref.row_var == u) & (ref.row_scalar == 0))[0]) for u in set(ref.row_var.tolist()) - {-1}}
    terms = []   # (factor, colB, dB, dst)
    for f in range(arr.n_factors):
        vs = [int(v) for v in arr.f_vars[arr.f_key_ptr[f]:arr.f_key_ptr[f + 1]]]
        if var not in vs:
            continue
        _, _, col = _blocks(arr, jac, f)
        terms.append((f, col[var], d, 0))
        for u in vs:
            if pos[u] > pos[var]:
                terms.append((f, col[u], int(arr.var_dims[u]), row0[u]))
        terms.append((f, sum(int(arr.var_dims[v]) for v in vs), 1, rows - 1))
    if mutation == "drop_last_of_64":
        assert len(terms) >= 64
        del terms[63]
    if mutation == "partner_at_neighbour_rows":
        k = next(i for i, t in enumerate(terms) if 0 < t[3] < rows - 1)
        f, cb, db, dst = terms[k]
        others = sorted({t[3] for t in terms if 0 < t[3] < rows - 1 and t[3] != dst and t[3] + db <= rows - 1})
        terms[k] = (f, cb, db, others[0])
    if mutation == "rhs_from_previous_factor":
        ks = [i for i, t in enumerate(terms) if t[3] == rows - 1]
        f_prev = terms[ks[0]][0]
        f, cb, db, dst = terms[ks[1]]
        _, vs_prev, _ = _blocks(arr, jac, f_prev)
        if int(arr.f_rows[f_prev]) == int(arr.f_rows[f]):
            terms[ks[1]] = (f, cb, db, dst, f_prev, sum(int(arr.var_dims[v]) for v in vs_prev))
    tn = len(terms)
    chunk = ((tn + waves - 1) // waves + 1) & ~1
    copies = np.zeros((waves, rows, d))
    for w in range(waves):
        if mutation == "skip_wave_chunk" and w == 1:
            continue
        for t in terms[w * chunk:min(tn, (w + 1) * chunk)]:
            f, cb, db, dst = t[:4]
            Ab, _, col = _blocks(arr, jac, f)
            B = Ab[:, cb:cb + db]
            if len(t) > 4:   # the rhs column of another factor against this factor's own block
                B = _blocks(arr, jac, t[4])[0][:, t[5]:t[5] + 1]
            copies[w, dst:dst + db] += B.T @ Ab[:, col[var]:col[var] + d]
    out = np.zeros((rows, d))
    for w in range(waves):
        out = out + copies[w]
    return out


# ---- the cases -----------------------------------------------------------------------------------------------------------
def _cyc(v, partners, n, m=2, flip=False):
    """n binary factors of m rows between v and the partners in turn."""
    return [((partners[i % len(partners)], v) if flip else (v, partners[i % len(partners)]), m) for i in range(n)]


def _terms_case(name, cls, nb, nu, m=2, d0=8, pd=(2, 3, 1), expect_rest=None):
    """Variable 0 of dimension d0 with nb binary factors (3 terms each) to later partners in turn and nu unary factors
    (2 terms each), all of m rows: 3 nb + 2 nu terms."""
    dims = [d0] + list(pd)
    fac = _cyc(0, list(range(1, len(dims))), nb, m) + [((0,), m)] * nu
    fac += [((v,), 2) for v in range(1, len(dims)) if nb < len(pd) and v > nb]   # (every variable is in the graph)
    return Case(name, dims, fac, {0: cls})


def _star_graph(n, d=3, partners=(4, 4), m=2, extra=()):
    """n star variables of dimension d, each with one factor of m rows to every partner (the last variables)."""
    dims = [d] * n + list(partners)
    fac = [((v, n + q), m) for v in range(n) for q in range(len(partners))]
    return dims, fac + list(extra)


def _bundles(sizes):
    return {v: s for v, s in enumerate(x for s in sizes for x in [s] * max(s, 1))}


def _build():
    C = []
    # ---- tile: 2..64 terms, factors of at most 8 rows and 16 columns with the rhs ----
    C.append(Case("tile_terms_2", [3], [((0,), 2)], {0: TILE}))
    C.append(_terms_case("tile_terms_64", TILE, 20, 2, d0=3))
    C.append(_terms_case("tile_terms_65_is_light", LIGHT, 21, 1, d0=8))
    C.append(Case("tile_rows_8", [3, 2], [((0,), 8), ((0, 1), 8), ((1,), 2)], {0: TILE}))
    C.append(Case("tile_rows_9_is_light", [3, 2], [((0,), 8), ((0, 1), 9), ((1,), 2)], {0: LIGHT}))
    C.append(Case("tile_cols_16", [7, 8], [((0,), 2), ((0, 1), 3), ((1,), 2)], {0: TILE, 1: TILE}))
    C.append(Case("tile_cols_17_is_light", [8, 8], [((0,), 2), ((0, 1), 3), ((1,), 2)], {0: LIGHT}))
    C.append(Case("tile_ternary_first_and_middle", [3, 4, 5], [((0, 1, 2), 4), ((0,), 2), ((1,), 3), ((2,), 2), ((1, 0, 2), 5)],
                  {0: TILE, 1: TILE, 2: TILE}))
    for n in (1, 4, 5):   # n tile variables under a hub that a 9-row factor keeps out of the tile class
        C.append(Case("tile_group_of_%d" % n, [3] * n + [2],
                      [((v,), 2) for v in range(n)] + [((v, n), 2) for v in range(n)] + [((n,), 9)],
                      {**{v: TILE for v in range(n)}, n: LIGHT}, group_size={0: n}))
    # panels of p = 8 x 16 = 128 and 2p = 8 x 32 doubles in one group: the LDS stride is that of the larger
    C.append(Case("tile_group_p_and_2p", [8, 8, 7, 7, 7, 2],
                  [((0,), 2), ((0, 2), 2), ((1,), 3), ((1, 2), 2), ((1, 3), 2), ((1, 4), 2), ((1, 5), 2)] +
                  [((v,), 9) for v in (2, 3, 4, 5)], {0: TILE, 1: TILE}, same_group=(0, 1), group_size={0: 2}))
    # ---- light ----
    C.append(_terms_case("light_terms_6", LIGHT, 2, 0, m=9))
    C.append(_terms_case("light_terms_7", LIGHT, 1, 2, m=9))
    C.append(_terms_case("light_terms_8", LIGHT, 2, 1, m=9))
    C.append(_terms_case("light_terms_63", LIGHT, 21, 0, m=9))
    C.append(_terms_case("light_terms_64", LIGHT, 20, 2, m=9))
    C.append(_terms_case("light_terms_65", LIGHT, 21, 1, m=9))
    # 120 terms on a panel of 65 x 32 = 2080 doubles: one wave, two blocks of records
    C.append(Case("light_120_terms_wide_panel", [32, 16, 16], _cyc(0, [1, 2], 40) + [((1,), 2), ((2,), 2)], {0: LIGHT}))
    C.append(Case("light_rows_1_3_5_9", [8, 2, 3],
                  [((0, 1), 1), ((0,), 3), ((0, 2), 5), ((0, 1), 9), ((0,), 1), ((0, 2), 2), ((1,), 2), ((2,), 2)], {0: LIGHT}))
    # ---- heavy: 96 terms or more on at most 1536 doubles ----
    C.append(_terms_case("heavy_terms_96", HEAVY, 32, 0))
    C.append(_terms_case("heavy_terms_97", HEAVY, 31, 2))
    C.append(_terms_case("heavy_terms_98", HEAVY, 32, 1))
    C.append(_terms_case("heavy_terms_99", HEAVY, 33, 0))
    C.append(_terms_case("heavy_terms_261", HEAVY, 87, 0))     # a wave's chunk of 66 records: two fetches
    C.append(Case("heavy_panel_1536", [32, 15], _cyc(0, [1], 33) + [((1,), 2)], {0: HEAVY}))           # 48 x 32
    C.append(Case("heavy_panel_1537_is_light", [29, 23], _cyc(0, [1], 33) + [((1,), 2)], {0: LIGHT}))  # 53 x 29
    # ---- huge: above 6144 doubles ----
    C.append(Case("huge_193x64", [64, 64, 64], [((0, 1), 2), ((0, 2), 3), ((0,), 2), ((1,), 2), ((2,), 2)],
                  {0: HUGE, 1: LIGHT, 2: LIGHT}))
    C.append(Case("huge_two_in_a_group", [64, 64, 64], [((0, 1), 2), ((0, 2), 3), ((1, 2), 2), ((0,), 2), ((1,), 5), ((2,), 2)],
                  {0: HUGE, 1: HUGE, 2: LIGHT}, same_group=(0, 1), group_size={0: 2}))
    # ---- diag: the last-eliminated variable, at most 15 dimensions, 32 factors or more ----
    def diag_case(name, d, nf, cls, rows=(2,)):
        fac = [((0, 1), 2), ((0,), 2)] + [((1,), rows[i % len(rows)]) for i in range(nf - 1)]
        return Case(name, [2, d], fac, {1: cls})
    for d in (1, 8, 15):
        C.append(diag_case("diag_dim_%d_32_factors" % d, d, 32, DIAG))
    C.append(diag_case("diag_dim_16_is_light", 16, 32, LIGHT))
    C.append(diag_case("diag_31_factors_is_tile", 8, 31, TILE))
    C.append(diag_case("diag_33_factors", 8, 33, DIAG))
    C.append(diag_case("diag_100_factors", 8, 100, DIAG))
    C.append(diag_case("diag_rows_1_2_5", 8, 40, DIAG, rows=(1, 2, 5, 2, 2, 9)))
    # ---- star: dimension <= 7, binary factors of one shape, a partner each ----
    for n, sizes in ((1, [1]), (5, [5]), (6, [5, 1]), (11, [5, 5, 1])):
        dims, fac = _star_graph(n)
        C.append(Case("star_%d_variables" % n, dims, fac, {v: STAR for v in range(n)}, bundles=_bundles(sizes)))
    dims, fac = _star_graph(3, d=7)
    C.append(Case("star_dim_7_alone_in_bundle", dims, fac, {v: STAR for v in range(3)}, bundles=_bundles([1, 1, 1])))
    dims, fac = _star_graph(3, d=8)
    C.append(Case("star_dim_8_refused", dims, fac, {v: TILE for v in range(3)}))
    dims, fac = _star_graph(4, m=3)
    C.append(Case("star_rows_3", dims, fac, {v: STAR for v in range(4)}, bundles=_bundles([4])))
    # two shapes A A B B A: the bundles are 2, 2, 1
    dd = [3, 3, 2, 2, 3]
    C.append(Case("star_two_shapes_interleaved", dd + [4, 4], [((v, 5 + q), 2) for v in range(5) for q in range(2)],
                  {v: STAR for v in range(5)}, bundles=_bundles([2, 2, 1])))
    # factor totals of a bundle: 32 + 32 = 64 share one, 32 + 33 = 65 do not
    for tot, sizes in ((64, [2]), (65, [1, 1])):
        n1 = tot - 32
        C.append(Case("star_bundle_%d_factors" % tot, [3, 3] + [1] * 33,
                      [((0, 2 + q), 2) for q in range(32)] + [((1, 2 + q), 2) for q in range(n1)] +
                      ([((34,), 2)] if n1 < 33 else []), {0: STAR, 1: STAR}, bundles=_bundles(sizes)))
    C.append(Case("star_65_factors_unbundled", [3, 3] + [1] * 65,
                  [((0, 2 + q), 2) for q in range(65)] + [((1, 2 + q), 2) for q in range(2)],
                  {0: STAR, 1: STAR}, bundles={0: 0, 1: 0}))
    dims, fac = _star_graph(3)
    C.append(Case("star_refused_two_factors_to_one_partner", dims, fac + [((0, 3), 2)], {0: TILE, 1: STAR, 2: STAR},
                  bundles={1: 2, 2: 2}))
    C.append(Case("star_refused_prior", dims, fac + [((1,), 2)], {0: STAR, 1: TILE, 2: STAR}, bundles={0: 2, 2: 2}))
    C.append(Case("star_refused_unequal_partners", [3, 3, 3, 4, 5], [((v, 3 + q), 2) for v in range(3) for q in range(2)],
                  {v: TILE for v in range(3)}))
    # ---- diag and star together: 11 star variables under two partners with 32 factors each; the same factors (and
    #      numbers) with the partners' unary factors cut to 10 (no diag group) and with a prior on every star variable ----
    dims, fac = _star_graph(11, partners=(6, 6))
    unary = [((11 + q,), 2) for q in range(2) for _ in range(21)]
    few = [i for i, (vs, _) in enumerate(unary) if i % 21 < 10]
    priors = [((v,), 2) for v in range(11)]
    nf, nu = len(fac), len(unary)
    C.append(Case("both_diag_and_star", dims, fac + unary, {**{v: STAR for v in range(11)}, 11: DIAG, 12: DIAG},
                  bundles=_bundles([5, 5, 1]), fused=True))
    C.append(Case("both_star_alone", dims, fac + [unary[i] for i in few], {**{v: STAR for v in range(11)}, 11: TILE, 12: TILE},
                  bundles=_bundles([5, 5, 1]), ids=list(range(nf)) + [nf + i for i in few]))
    C.append(Case("both_diag_alone", dims, fac + unary + priors, {**{v: TILE for v in range(11)}, 11: DIAG, 12: DIAG},
                  ids=list(range(nf + nu)) + [1000 + v for v in range(11)]))
    names = [c.name for c in C]
    assert len(set(names)) == len(names)
    return {c.name: c for c in C}


CASES = _build()
# the variables whose panels must be the same numbers in "both_diag_and_star" and in the case where their group is alone
BOTH_SAME = {"both_star_alone": range(11), "both_diag_alone": (11, 12)}


def check_groups(case, groups):
    """Assert that every variable the case names reached its class, bundle and group (gsx_get_hessian_groups)."""
    cls = groups["class"]
    for v, want in case.expect.items():
        assert cls[v] == want, "%s: variable %d is %s, the case was built for %s" % (
            case.name, v, NAMES[cls[v]] if cls[v] >= 0 else cls[v], NAMES[want])
    for v, size in case.bundles.items():
        assert groups["bundle_size"][v] == size, "%s: variable %d sits in a bundle of %d, built for %d" % (
            case.name, v, groups["bundle_size"][v], size)
        assert (groups["bundle"][v] >= 0) == (size > 0), (case.name, v)
        if size > 0:   # ... shared with exactly that many variables
            assert int(np.sum((groups["bundle"] == groups["bundle"][v]) & (cls == STAR))) == size, (case.name, v)
    for v, n in case.group_size.items():
        assert int(np.sum(groups["group"] == groups["group"][v])) == n, (case.name, v, n)
    if case.same_group:
        assert len({int(groups["group"][v]) for v in case.same_group}) == 1, case.name
    for g in set(groups["group"].tolist()):
        members = np.flatnonzero(groups["group"] == g)
        assert sorted(groups["position"][members].tolist()) == list(range(len(members))), (case.name, g)
        assert len(set(cls[members].tolist())) == 1, (case.name, g)


# ---- the partial path (gsx_relinearize_partial: partial_assemble launches each group's kernel on the dirty variables
#      alone; star variables always through the unbundled kernel) --------------------------------------------------------------
# Four variables g0..g3 of the class, each with a NATIVE factor whose right-hand side moves with the variable (a
# PriorFactor; the star variables, which may have none, two BetweenFactors to partners of their own), the class-shaping
# JacobianFactors to later partners, and N_PADS scalar leaves under a hub so that the dirty cliques stay under both
# fall-back limits of gsx_relinearize_partial.  g1 and g2 are moved: a strict sub-range of their group that does not
# start it.
N_PADS = 40
PartialCase = __import__("collections").namedtuple("PartialCase", "name cls arr ordering group moved dims")


def partial_case(cls):
    from gtsam_petercdev_amd.graph import BetweenFactor, NonlinearFactorGraph, PriorFactor, Values
    rng = np.random.default_rng(900 + cls)
    d, partners = {TILE: (3, [2, 3]), LIGHT: (8, [12]), HEAVY: (8, [2, 3, 1]), HUGE: (8, [64] * 12), DIAG: (8, []),
                   STAR: (3, [3] * 8)}[cls]
    # (huge: the twelve 64-dimensional partners make a dozen dirty blocked cliques that hold every gather segment of the
    #  tree, so the 5 % limit applies: 320 leaves)
    n_pads = 320 if cls == HUGE else N_PADS
    dims = [d] * 4 + [1 if j % 2 else 3 for j in range(n_pads)] + list(partners) + [3]
    p0, hub = 4 + n_pads, len(dims) - 1
    g = NonlinearFactorGraph()

    def unary(k, m=None):
        g.add(JacobianFactor(k, np.eye(dims[k])[:m or dims[k]] * (0.7 + rng.random()) + 0.05 * rng.normal(size=(m or dims[k], dims[k])),
                             rng.normal(size=m or dims[k]), noiseModel.Isotropic.Sigma(m or dims[k], 1.5)))

    def pair(a, b, m=2):
        g.add(JacobianFactor(a, rng.normal(0, 0.3, (m, dims[a])), b, rng.normal(0, 0.3, (m, dims[b])), rng.normal(size=m),
                             noiseModel.Diagonal.Sigmas(0.5 + rng.random(m), smart=False)))

    for v in range(4):
        if cls == STAR:
            for q in range(2):
                g.add(BetweenFactor(v, p0 + 2 * v + q, rng.normal(size=3), noiseModel.Diagonal.Sigmas(0.5 + rng.random(3))))
            continue
        g.add(PriorFactor(v, rng.normal(size=d), noiseModel.Diagonal.Sigmas(0.5 + rng.random(d))))
        if cls == TILE:
            pair(v, p0), pair(v, p0 + 1)
        elif cls == LIGHT:
            pair(v, p0, 9)
        elif cls == HEAVY:
            for i in range(32):
                pair(v, p0 + i % 3)
        elif cls == HUGE:
            for q in range(12):
                pair(v, p0 + q)
        elif cls == DIAG:
            for i in range(32):
                unary(v, 2)
    for k in range(4, len(dims)):
        unary(k)
    for k in range(4, hub):
        pair(k, hub)
    values = Values()
    for k, dk in enumerate(dims):
        values.insert(k, np.zeros(dk))
    arr = g.to_arrays(values)
    assert list(arr.var_keys) == list(range(len(dims)))
    return PartialCase("partial_" + NAMES[cls], cls, arr, list(range(len(dims))), [0, 1, 2, 3], [1, 2], dims)


def partial_dirty(pc):
    """The variables whose panels gsx_relinearize_partial reassembles: every variable of a factor of a moved one."""
    arr, out = pc.arr, set()
    for f in range(arr.n_factors):
        vs = [int(v) for v in arr.f_vars[arr.f_key_ptr[f]:arr.f_key_ptr[f + 1]]]
        if set(vs) & set(pc.moved):
            out |= set(vs)
    return sorted(out)


def check_partial_groups(pc, groups):
    """g0..g3 are of the case's class and share a launch group; the dirty members of that group are a strict subset of it
    that leaves out its first variable."""
    cls, grp, pos = groups["class"], groups["group"], groups["position"]
    for v in pc.group:
        assert cls[v] == pc.cls, "%s: variable %d is %s" % (pc.name, v, NAMES[cls[v]])
    assert len({int(grp[v]) for v in pc.group}) == 1, pc.name
    members = np.flatnonzero(grp == grp[pc.group[0]])
    dirty = [v for v in partial_dirty(pc) if grp[v] == grp[pc.group[0]]]
    assert set(pc.moved) <= set(dirty) and len(dirty) < len(members), (pc.name, dirty, members)
    assert min(pos[v] for v in dirty) > 0, (pc.name, dirty)
    if pc.cls == STAR:
        assert all(groups["bundle_size"][v] == 4 for v in pc.group), pc.name   # the full path bundles what the partial does not
