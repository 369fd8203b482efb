"""The rows of L21 of the blocked fronts (csrc/bigfront.hip, section B: 32 rows per workgroup, or 64 with L11 staged
once for both row halves when the launch holds more 32-row blocks than the device has CUs) under the float64 backward-error bounds of test_gpu_linear_bounds.py: same graphs (dense Gaussian cliques of
chosen frontal and separator width, cases.two_clique_arrays / cases._edge_graph), same judges and gamma (tests/_ld_linear.py),
through the C ABI.  A wrong or missing row of L21 breaks R'R = H + lambda D in the columns of that front (measure 1), the
right-hand side row breaks R'd = g (measure 2), and either breaks the step (measure 3).

Every graph carries a full-rank unary factor on every variable (0.7-1.7 times the identity at sigma 1.5), so H is
positive definite at lambda = 0 and at every lambda used: no case can be indeterminate, none is skipped.

What reaches the kernel.  A front is eliminated by the blocked kernels when it has more than 140 rows (symbolic.cpp:
kSmallMaxN); below that the whole front lives in LDS and big_rows never sees it.  Of the row-block edges listed for
F = 32 and F = 96 the library therefore runs the short ones (F + rows <= 140) in its LDS class: they are judged all the
same, and `blocked` below says which class each case must be in, so a case that silently changed class fails.  Chunks of
one to three column steps over FEW rows do reach the kernel in the second round of a two-round front (F = 193: 128 + 65
columns, F = 224: 128 + 96), whose rows below are the separator and the right-hand side alone.  A single front is a
small launch and runs the 32-row form; the 64-row form is reached by the launch groups at the end (150 and 64 fronts
of one level): the first strides over row blocks at six column steps, the others repeat the row-block edges in that
form at every number of column steps, one to six.

Both LDS sizing functions of bigfront.hip (the rows launcher's and backsolve_big_lds) are checked on the host.
"""
import ctypes as C

import pytest

from tests import _ld_linear as J
from tests import _linear_cases as cases

ROW_EDGES = [1, 31, 32, 33, 63, 64, 65, 97, 129]          # rows below the chunk, right-hand side row included
ROW_WIDTHS = [32, 96, 192]                                # one, three and six column steps of 32
TWO_ROUND_WIDTHS = [193, 224, 360, 384]
TWO_ROUND_ROWS = [1, 33, 65]
L2 = 0.1 * (1 + 1e-8)
NEIGHBOURS = [(0.1, True), (L2, True), (0.0, False), (L2, True)]
K_SMALL_MAX_N = 140                                       # gsx_internal.h: kSmallMaxN
K_MAX_CHUNK = 192                                         # bigfront.hip: kMaxChunk
LDS_PER_CU = 160 * 1024
TILE_BYTES = 32 * 34 * 8                                  # an LDS tile of big_rows_kernel: 32 rows of stride 34


@pytest.fixture(scope="module")
def gpu():
    from gtsam_petercdev_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the HIP path has no fallback"
    return _lib


def _front_case(gpu, F, rows):
    """(backend, judge, class of the front with F frontal columns and `rows` rows below them).  rows = 1: the root clique
    (B, c) of the two-clique tree, whose only row below is the right-hand side; otherwise the child (A | B)."""
    if rows == 1:
        arr, order, _, _ = cases.two_clique_arrays(5, F - 3)
    else:
        arr, order, _, _ = cases.two_clique_arrays(F, rows - 1)
    gb = gpu.product_backend(arr)
    gb.set_amalgamation(0.0, 128)
    gb.set_ordering(order)
    _, fronts = gb.get_tree()
    cls = gb.front_classes()
    dims = arr.var_dims
    shape = [(int(sum(dims[v] for v in f)), int(sum(dims[v] for v in s)) + 1) for f, s in fronts]
    assert (F, rows) in shape, shape
    gb.linearize()
    return gb, J.Judge(arr, gb.jacobians()), int(cls[shape.index((F, rows))]) & 3


def _judge(gb, judge, what, lambdas):
    for lam, diag in lambdas:
        judge.check_backward(gb, gb.solve(lam, diag), lam, diag, what)


@pytest.mark.gpu
@pytest.mark.parametrize("F", ROW_WIDTHS)
@pytest.mark.parametrize("rows", ROW_EDGES)
def test_row_block_edges(gpu, F, rows):
    """A half-empty second half (1, 31, 32 rows; 65, 97 in the second block), an exactly full block (64), one row spilling
    into a new block (33 into the second half, 65 and 129 into a new block)."""
    gb, judge, cls = _front_case(gpu, F, rows)
    blocked = F + rows > K_SMALL_MAX_N
    assert (cls == 2) == blocked, (F, rows, cls)
    _judge(gb, judge, f"row edges F={F} rows={rows} class {cls}", cases.LAMBDAS)


@pytest.mark.gpu
@pytest.mark.parametrize("F", TWO_ROUND_WIDTHS)
@pytest.mark.parametrize("rows", TWO_ROUND_ROWS)
def test_two_rounds(gpu, F, rows):
    """Two chunks: the second round's rows start where the first chunk ended, and the first round's rows include the
    second chunk's columns.  F = 360 with only the right-hand side row is the root shape of the benchmark.  One handle at
    two neighbouring lambdas and back: a tile left over from the previous trial is 1e7 u off."""
    gb, judge, cls = _front_case(gpu, F, rows)
    assert cls == 2, (F, rows, cls)
    _judge(gb, judge, f"two rounds F={F} rows={rows}", NEIGHBOURS)


def _backsolve_big_lds():
    from gtsam_petercdev_amd import _lib
    f = _lib.load().gsxtest_backsolve_big_lds
    f.restype = C.c_longlong
    f.argtypes = [C.c_int, C.c_int, C.c_int]
    return f


def _split(total):
    """Variables of at most 64 dimensions that add up to `total`."""
    return [64] * (total // 64) + ([total % 64] if total % 64 else [])


def mixed_group_arrays():
    """150 childless cliques of one level over one clique B of 455 scalars (six variables of 64 dimensions, one of 63 and
    one of 8 that no leaf touches, so that no leaf's separator is the whole of B and none is merged into the root):
    leaf k is one variable of 17-64 dimensions, every tenth three of 64 (192 columns: six column steps for the whole
    group), joined to the first 2-7 variables of B.  Fronts of 17-192 frontal columns over 129-448 rows (3-7 row blocks of
    64), all taller than the LDS class."""
    bdims = [64] * 6 + [63, 8]
    ldims = [17, 33, 64, 40, 24]
    dims, edges, shapes = [], [], []
    leaves = []
    for k in range(150):
        mine = list(range(len(dims), len(dims) + (3 if k % 10 == 9 else 1)))
        dims += [64, 64, 64] if k % 10 == 9 else [ldims[k % len(ldims)]]
        edges += [(a, b) for a in mine for b in mine if a < b]
        leaves.append((mine, 2 + k % 6))
    b0 = len(dims)
    dims += bdims
    for mine, m in leaves:
        edges += [(a, b0 + j) for a in mine for j in range(m)]
        shapes.append((sum(dims[a] for a in mine), sum(bdims[:m]) + 1))
    edges += [(b0 + i, b0 + j) for i in range(len(bdims)) for j in range(i + 1, len(bdims))]
    arr, order = cases._edge_graph(dims, edges, 9500)
    return arr, order, shapes


@pytest.mark.gpu
def test_mixed_group(gpu):
    """One launch group of fronts of different width and height, in the 64-row form at six column steps
    (big_rows_kernel<6, 2>, the instance of the benchmark's first blocked level): the narrow fronts run their missing
    column steps on tiles of zeros, the short ones leave workgroups with nothing to do, and with 150 fronts of up to 7 row
    blocks the grid is capped (1024 / 150 = 6 workgroups a front): the tallest fronts' first workgroup strides on to a
    second row block, whose L11 stream restarts from the column block kept in registers.  Fronts of 192 columns are among
    the tallest (k = 59, 119: 448 rows), so the strided pass runs all six steps on real tiles."""
    arr, order, shapes = mixed_group_arrays()
    widest = max(r for _, r in shapes)
    assert (widest + 63) // 64 == 7 and 7 * len(shapes) > 1024 >= 6 * len(shapes)
    assert max(f for f, _ in shapes) == 192 and (192, 448) in shapes
    _group_case(gpu, arr, order, shapes, "mixed group")


WIDE_EDGES = [31, 32, 33, 63, 64, 65, 97, 129]            # ROW_EDGES without the lone right-hand side row
# frontal width -> whole row blocks of 64 put under every front, so that the shortest one is past the LDS class
WIDE_WIDTHS = {32: 2, 64: 1, 96: 1, 128: 0, 160: 0, 192: 0}


def wide_edges_arrays(F):
    """64 childless cliques of F frontal columns over 64 j + (31, 32, 33, 63, 64, 65, 97, 129) rows, eight of each, with
    j = WIDE_WIDTHS[F] whole row blocks underneath so that every front has more than 140 rows: separators made of
    variables of the root clique B (30, 31, 32, 62, 63, 64, 64, the j blocks of 64 and an untouched 8 dimensions).  At
    least 320 blocks of 32 rows in one launch: more than the 256 CUs of the device, so the launch takes 64 rows per
    workgroup, and these are the row-block edges of THAT form at ceil(F / 32) column steps."""
    j = WIDE_WIDTHS[F]
    bdims = [30, 31, 32, 62, 63, 64, 64] + [64] * j + [8]
    under = list(range(7, 7 + j))
    seps = [s + under for s in ([0], [1], [2], [3], [4], [5], [2, 5], [5, 6])]   # 30 ... 128 scalars (+ 64 j): rows = + 1
    mine_dims = _split(F)
    dims, edges, shapes, leaves = [], [], [], []
    for k in range(64):
        leaves.append((list(range(len(dims), len(dims) + len(mine_dims))), seps[k % 8]))
        dims += mine_dims
    b0 = len(dims)
    dims += bdims
    for mine, sep in leaves:
        edges += [(a, b) for a in mine for b in mine if a < b]
        edges += [(a, b0 + i) for a in mine for i in sep]
        shapes.append((F, sum(bdims[i] for i in sep) + 1))
    edges += [(b0 + i, b0 + k) for i in range(len(bdims)) for k in range(i + 1, len(bdims))]
    arr, order = cases._edge_graph(dims, edges, 9600 + F)
    return arr, order, shapes


def _group_case(gpu, arr, order, shapes, what):
    gb = gpu.product_backend(arr)
    gb.set_amalgamation(0.0, 128)
    gb.set_ordering(order)
    _, fronts = gb.get_tree()
    cls = gb.front_classes()
    dims = arr.var_dims
    got = sorted((int(sum(dims[v] for v in f)), int(sum(dims[v] for v in s)) + 1) for (f, s), c in zip(fronts, cls)
                 if len(s) and (int(c) & 3) == 2)
    assert got == sorted(shapes), (got[:5], sorted(shapes)[:5])
    gb.linearize()
    judge = J.VectorJudge(arr, gb.jacobians())
    for lam, diag in [(0.1, True), (L2, True), (0.0, False)]:
        judge.check_backward(gb, gb.solve(lam, diag), lam, diag, what)


@pytest.mark.gpu
@pytest.mark.parametrize("F", list(WIDE_WIDTHS))
def test_row_block_edges_of_a_wide_launch(gpu, F):
    """The row-block edges in the 64-row form, at one to six column steps (big_rows_kernel<1..6, 2>): in the last row
    block a second half that is empty (31, 32 rows), holds one row (33) or is one short (63), a full block (64), one row
    into a new block (65, 129) and a half-empty block (97)."""
    arr, order, shapes = wide_edges_arrays(F)
    under = 64 * WIDE_WIDTHS[F]
    assert sorted(set(r for _, r in shapes)) == [under + r for r in WIDE_EDGES]
    assert all(F + r > K_SMALL_MAX_N for _, r in shapes)
    assert len(shapes) * ((under + 129 + 31) // 32) >= 320     # 32-row blocks of the launch's grid
    _group_case(gpu, arr, order, shapes, f"wide launch edges F={F}")


def test_rows_launch_sizing():
    """Host only: the LDS the rows launcher asks for at every chunk width, launch size and device size, against the
    160 KB of a CU, and what its guard refuses: exactly the widths no round makes (0, and anything past kMaxChunk, for
    which there is no kernel).  Launches of more 32-row blocks than the device has CUs take 64 rows per workgroup."""
    from gtsam_petercdev_amd import _lib
    f = _lib.load().gsxtest_big_rows_lds
    f.restype = C.c_longlong
    f.argtypes = [C.c_int, C.c_longlong, C.c_int, C.POINTER(C.c_int)]
    for cus in (64, 256, 304):
        for tiles in (1, 2, cus - 1, cus, cus + 1, 1024, 100000):
            for fw in range(-1, 2 * K_MAX_CHUNK + 1):
                rows = C.c_int(-7)
                b = f(fw, tiles, cus, C.byref(rows))
                assert b == f(fw, tiles, cus, None)
                if fw < 1 or fw > K_MAX_CHUNK:
                    assert b == 0 and rows.value == 0, (fw, tiles, b, rows.value)
                    continue
                nk = (fw + 31) // 32
                assert rows.value == (64 if tiles > cus else 32), (fw, tiles, cus, rows.value)
                # column blocks of L11 double-buffered (2 nk tiles), one T / X pair per 32 rows
                assert b == (2 * nk + 2 * rows.value // 32) * TILE_BYTES, (fw, tiles, b, rows.value)
                assert 0 < b <= LDS_PER_CU, (fw, tiles, b)
    assert f(K_MAX_CHUNK, 0, 256, None) == 0 and f(K_MAX_CHUNK, 257, 0, None) == 0
    assert f(K_MAX_CHUNK, 257, 256, None) == 16 * TILE_BYTES   # six column steps, two row halves: 136 KB


def test_backsolve_big_sizing():
    """Host only: backsolve_big_lds over F = 1 .. 385 and heights from the lone right-hand side row to past the 320 rows
    (separator and right-hand side) its level test admits: the bytes are the kernel's own layout (xs[n], y, one block's
    solution, the packed inverses and the strictly lower tiles of L11), never past the launcher's 160 KB - 256, and 0
    exactly for what does not fit, is wider than one chunk, or is taller than that below the frontal columns."""
    f = _backsolve_big_lds()
    limit = LDS_PER_CU - 256
    for F in range(1, 2 * K_MAX_CHUNK + 2):
        nk = (F + 31) // 32
        for below in (1, 2, 161, 320, 321, 400):               # n - F: separator rows and the right-hand side row
            n = F + below
            want = 8 * (((n + 1) & ~1) + nk * 32 + 32 + nk * 528 + nk * (nk - 1) // 2 * 1024)
            if F > K_MAX_CHUNK or below > 320 or want > limit:
                want = 0
            assert f(n, F, below) == want, (F, below, f(n, F, below), want)
            assert want <= limit
    assert f(K_MAX_CHUNK + 320, K_MAX_CHUNK, 320) > 0           # the widest front over the tallest separator fits
    assert f(30000, 100, 0) == 0                                # a front taller than LDS holds
