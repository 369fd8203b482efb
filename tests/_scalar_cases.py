"""Seeded LINEAR graphs for the scalar-reduction tests (test_host_scalar_judge.py, test_gpu_scalar_bounds.py): the smallest
shapes that reach each edge of the linearized-error, damping and Dogleg reductions.  Every factor has the unit noise
model, so its whitened [A b] is the block it was given (upload.hip: whiten_linear_factor copies it) and the host tests
know the device's Jacobian array without a device: jacobian_array()."""
import numpy as np

from gtsam_petercdev_amd.graph import GaussianFactorGraph, JacobianFactor

# upload.hip, upload_problem: the staged kernel's LDS slice is the largest [A b] range of 64 consecutive factors,
# rounded up to even, and 0 (the direct kernel) when two slices exceed 96 KB
SLICE_LIMIT = 96 * 1024 // (2 * 8)          # 6144 doubles


def _graph(dims, factors, seed):
    """factors: [(rows, [variables])].  A unary factor of as many rows as its variable has scalars gets a dominant
    diagonal, so that a graph whose every variable has one is well determined."""
    rng = np.random.default_rng(seed)
    fg = GaussianFactorGraph()
    seen = set()
    for m, vs in factors:
        args = []
        for v in vs:
            blk = rng.normal(0, 0.4, (m, dims[v]))
            if len(vs) == 1 and m == dims[v]:
                blk += np.eye(m) * (1.0 + rng.random())
            args += [v, blk]
            seen.add(v)
        fg.add(JacobianFactor(*args, rng.normal(size=m)))
    assert seen == set(range(len(dims))), "a variable without a factor"
    arr = fg.to_arrays(None)
    arr.values = np.zeros(int(arr.var_dims.sum()))
    return arr


def jacobian_array(arr):
    """gsx_get_jacobians of a unit-noise linear graph: the given blocks, one after the other."""
    return np.asarray(arr.meas[:int(arr.f_meas_ptr[-1])], dtype=np.float64).copy()


def slice_of(arr):
    """(largest range of 64 consecutive factors, lin_err_slice) by upload_problem's rule; the offsets of a problem are
    cumulative, hence ascending."""
    off = arr.jacobian_offsets()
    worst = max(int(off[min(arr.n_factors, i0 + 64)] - off[i0]) for i0 in range(0, arr.n_factors, 64))
    even = (worst + 1) & ~1
    return worst, (even if 0 < even <= SLICE_LIMIT else 0)


STAGED_N = [1, 63, 64, 65, 127, 128, 129, 192, 193]


def chain(n_factors):
    """u0 b01 u1 b12 ... : unary factors (rows = the variable's 1 to 4 scalars) interleaved with two- and three-row
    factors between neighbours; an even count ends on a three-row unary factor on variable 0.  (n + 1) // 2 variables.
    One factor: three rows on a 2-dimensional variable — a square system has e(delta) = 0 at its solution, and a bound
    relative to e(delta) judges nothing there."""
    if n_factors == 1:
        return _graph([2], [(3, [0])], 5101)
    nv = (n_factors + 1) // 2
    dims = [(2, 3, 1, 4)[k % 4] for k in range(nv)]
    factors = []
    for k in range(nv):
        factors.append((dims[k], [k]))
        if k + 1 < nv:
            factors.append((2 + k % 2, [k, k + 1]))
    if len(factors) < n_factors:
        factors.append((3, [0]))
    assert len(factors) == n_factors
    return _graph(dims, factors, 5100 + n_factors)


def chain_vars(n_vars):
    """The chain with n_vars variables (2 n_vars - 1 factors)."""
    return chain(2 * n_vars - 1)


def staged_rounding():
    """Blocks of 9 + 10 + 6 = 25 doubles: the slice is 26, the only group ends one double short of it."""
    return _graph([2, 2], [(3, [0]), (2, [0, 1]), (2, [1])], 5301)


def staged_limit(over=False):
    """64 three-row factors on a 15- and a 16-dimensional variable, 96 doubles each: 6144 doubles, two slices of exactly
    96 KB; a 65th small factor makes a second group.  over: one factor has four rows, 6176 doubles — the direct kernel."""
    dims = [15, 16] * 4
    factors = [(3, [2 * (k % 4), 2 * ((k // 4) % 4) + 1]) for k in range(64)]
    if over:
        factors[17] = (4, factors[17][1])
    factors.append((1, [0]))
    return _graph(dims, factors, 5302 + int(over))


DIRECT_N = [1, 255, 256, 257, 513]


def direct_mix(n_factors):
    """Nine-row factors on two 9-dimensional variables (171 doubles; 40 of every 64 factors: 6840 doubles, over the
    limit) interleaved with two-row factors on a 2- and a 9-dimensional variable (24 doubles) and three-row unary factors
    on a 2-dimensional variable (a 3 x 3 block).  171 and 9 are odd, so two-row factors land on even and on odd offsets.
    n_factors = 1: one 48-row factor on two 64-dimensional variables (6192 doubles), the only way for a single factor
    past the limit; its system is singular, the step comes from a damped solve."""
    if n_factors == 1:
        return _graph([64, 64], [(48, [0, 1])], 5401)
    nv9, nv2 = n_factors // 8 + 2, n_factors // 8 + 1
    dims = [9] * nv9 + [2] * nv2
    factors, cb, c2, c3 = [], 0, 0, 0
    for i in range(n_factors):
        kind = "b2b3b2bb"[i % 8]
        if kind == "b":
            factors.append((9, [cb % nv9, (cb + 1) % nv9]))
            cb += 1
        elif kind == "2":
            factors.append((2, [(7 * c2) % nv9, nv9 + c2 % nv2]))
            c2 += 1
        else:
            factors.append((3, [nv9 + c3 % nv2]))
            c3 += 1
    return _graph(dims, factors, 5400 + n_factors)


def two_row_offsets(arr):
    """(number of two-row factors on an even offset, on an odd offset, other factors)."""
    off = arr.jacobian_offsets()[:-1]
    two = arr.f_rows == 2
    return int(np.sum(two & (off % 2 == 0))), int(np.sum(two & (off % 2 == 1))), int(np.sum(~two))


DOGLEG_TANGENT = [1, 255, 256, 257]


def dogleg_graph(n_tangent):
    """A chain of 3-dimensional variables (the last takes what is left) with n_tangent scalars in all: a unary factor
    each, a two-row factor between neighbours."""
    dims = [3] * (n_tangent // 3) + ([n_tangent % 3] if n_tangent % 3 else [])
    factors = []
    for k, d in enumerate(dims):
        factors.append((d, [k]))
        if k + 1 < len(dims):
            factors.append((2, [k, k + 1]))
    assert sum(dims) == n_tangent
    return _graph(dims, factors, 5500 + n_tangent)


def clamp_graph():
    """The 129-factor chain with the columns of every third variable scaled by 30 and of every third-plus-one by 1/30:
    diag(A'A) spans six decades, so limits taken from its own entries clamp from both sides."""
    arr = chain(129)
    off = arr.jacobian_offsets()
    meas = arr.meas.copy()
    for f in range(arr.n_factors):
        m = int(arr.f_rows[f])
        blk = meas[off[f]:off[f + 1]].reshape(-1, m)        # (columns + 1) x m: column-major [A b]
        col = 0
        for v in arr.f_vars[arr.f_key_ptr[f]:arr.f_key_ptr[f + 1]]:
            d = int(arr.var_dims[v])
            blk[col:col + d] *= (30.0, 1.0 / 30.0, 1.0)[v % 3]
            col += d
    arr.meas = meas
    return arr
