"""Loader of the product library (csrc/libgsx.so).  There is NO fallback: if the HIP
library is missing or cannot be loaded every entry point raises."""
from __future__ import annotations

import ctypes as C

import numpy as np
import os

from . import _abi as A

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libgsx.so")
_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the hot path.")
        _lib = C.CDLL(LIB_PATH)
    return _lib


def device_count() -> int:
    f = load().gsx_device_count
    f.restype = C.c_int32
    return int(f())


def version() -> str:
    f = load().gsx_version
    f.restype = C.c_char_p
    return f().decode()


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_int64)


class ShardInfo(C.Structure):
    _fields_ = [("rank", C.c_int32), ("world", C.c_int32), ("n_cap_fronts", C.c_int32), ("n_own_fronts", C.c_int32),
                ("cap_level0", C.c_int32), ("n_own_factors", C.c_int32), ("cap_doubles", C.c_int64),
                ("cap_flops", C.c_double), ("own_flops", C.c_double), ("total_flops", C.c_double)]


class PartialStats(C.Structure):
    _fields_ = [("n_factors_relinearized", C.c_int32), ("n_panels_reassembled", C.c_int32),
                ("n_fronts_reeliminated", C.c_int32), ("n_fronts", C.c_int32)]


class UpdateStats(C.Structure):
    _fields_ = [("n_vars_added", C.c_int32), ("n_vars_removed", C.c_int32), ("n_factors_added", C.c_int32),
                ("n_factors_removed", C.c_int32), ("n_vars_affected", C.c_int32), ("n_fronts", C.c_int32),
                ("host_symbolic_s", C.c_double), ("device_s", C.c_double)]


class ProductBackend(A.Backend):
    def __init__(self, arrays: A.ProblemArrays, device: int = 0, host_only: bool = False):
        """host_only=True skips the upload of the initial values: only the host-side entry points
        (orderings, symbolic analysis, get_tree, stats) are usable — for tests without a GPU."""
        super().__init__(load(), "gsx_", arrays, device, set_initial=not host_only)

    def set_amalgamation(self, relax: float, max_frontal_dim: int = 128):
        """Relaxed clique amalgamation for the next set_ordering (include/gsx.h); 0 = the reference's Bayes tree."""
        self._check(self._fn("set_amalgamation")(self._h, C.c_double(relax), C.c_int32(max_frontal_dim)),
                    "set_amalgamation")

    # -- one problem over several GPUs (include/gsx.h: gsx_set_shard) ------------------------------------------
    def set_shard(self, rank: int, world: int, allreduce):
        """Make this handle rank `rank` of `world` handles solving ONE problem; call before set_ordering.
        `allreduce(ptr, count) -> None` sums `count` doubles of device memory at address `ptr` over the ranks in place
        (see distributed.torch_allreduce).  Every later call on the handle is collective."""
        def cb(_user, ptr, count):
            try:
                allreduce(int(ptr), int(count))
                return 0
            except Exception as e:  # a raise cannot cross the C frame
                import sys
                print(f"gsx allreduce callback failed: {e!r}", file=sys.stderr)
                return 1
        self._shard_cb = ALLREDUCE_FN(cb)   # keep the trampoline alive as long as the handle
        self._check(self._fn("set_shard")(self._h, C.c_int32(rank), C.c_int32(world), self._shard_cb, None),
                    "set_shard")

    def front_classes(self) -> np.ndarray:
        """gsx_get_front_classes: per front, bits 0-1 = 0 leaf kernel / 1 LDS / 2 blocked / 3 medium, bit 2 = tree front,
        bit 3 = lean leaf."""
        n = C.c_int32()
        self._check(self._fn("get_tree")(self._h, C.byref(n), None, None, None, None, None, None), "get_tree")
        out = np.zeros(max(n.value, 1), np.int32)
        self._check(self._fn("get_front_classes")(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))), "get_front_classes")
        return out[:n.value]

    def gather_plan(self) -> dict:
        """gsx_get_gather_plan: the extend-add plan into the blocked fronts.  "segments": one dict per segment in launch
        order (A.GATHER_SEGMENT_FIELDS; group -1 = the side group, var_row -1 = the right-hand side), "sources":
        [(child front, F of a lean leaf or 0 for a stored block)], "combines": one dict per multi-segment task
        (A.GATHER_COMBINE_FIELDS)."""
        ns, nsrc, nm = C.c_int32(), C.c_int64(), C.c_int32()
        fn = self._fn("get_gather_plan")
        self._check(fn(self._h, C.byref(ns), C.byref(nsrc), C.byref(nm), None, None, None), "get_gather_plan")
        seg = np.zeros((max(ns.value, 1), len(A.GATHER_SEGMENT_FIELDS)), np.int64)
        src = np.zeros((max(nsrc.value, 1), 2), np.int32)
        comb = np.zeros((max(nm.value, 1), len(A.GATHER_COMBINE_FIELDS)), np.int32)
        self._check(fn(self._h, None, None, None, seg.ctypes.data_as(C.POINTER(C.c_int64)),
                       src.ctypes.data_as(C.POINTER(C.c_int32)), comb.ctypes.data_as(C.POINTER(C.c_int32))),
                    "get_gather_plan")
        return {"segments": [dict(zip(A.GATHER_SEGMENT_FIELDS, (int(v) for v in row))) for row in seg[:ns.value]],
                "sources": [(int(c), int(f)) for c, f in src[:nsrc.value]],
                "combines": [dict(zip(A.GATHER_COMBINE_FIELDS, (int(v) for v in row))) for row in comb[:nm.value]]}

    def hessian_groups(self) -> dict:
        """gsx_get_hessian_groups: per variable (index as in get_tree) "class" (A.H_TILE ... A.H_DIAG, -1 = another rank's),
        "group", "position", "bundle", "bundle_size" (star variables; -1 / 0 when unbundled), and "fused_diag_star" for
        the handle.  Host side: also answers on a host_only handle."""
        n = max(self.arrays.n_vars, 1)
        cols = {k: np.full(n, -1, np.int32) for k in ("class", "group", "position", "bundle", "bundle_size")}
        fused = C.c_int32()
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self._fn("get_hessian_groups")(self._h, ip(cols["class"]), ip(cols["group"]), ip(cols["position"]),
                                                   ip(cols["bundle"]), ip(cols["bundle_size"]), C.byref(fused)),
                    "get_hessian_groups")
        out = {k: a[:self.arrays.n_vars] for k, a in cols.items()}
        out["fused_diag_star"] = bool(fused.value)
        return out

    def hessian_panel(self, key):
        """gsx_get_hessian_panel: (panel[rows, dim], row_var[rows], row_scalar[rows]) of variable `key` as assembled on the
        device; the last row is the right-hand side (row_var -1)."""
        rows, dim = C.c_int32(), C.c_int32()
        fn = self._fn("get_hessian_panel")
        self._check(fn(self._h, C.c_uint64(int(key)), C.byref(rows), C.byref(dim), None, None, None), "get_hessian_panel")
        out = np.zeros(rows.value * dim.value)
        rv, rs = np.zeros(rows.value, np.int32), np.zeros(rows.value, np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        self._check(fn(self._h, C.c_uint64(int(key)), C.byref(rows), C.byref(dim), out.ctypes.data_as(C.POINTER(C.c_double)),
                       ip(rv), ip(rs)), "get_hessian_panel")
        return out.reshape(dim.value, rows.value).T, rv, rs

    def shard_probe_buffer(self):
        """(device address, doubles) of a buffer the library hipMalloc'd itself and that holds nothing between calls — what
        distributed.checked_allreduce probes the in-place collective on (gsx_scratch_buffer)."""
        ptr = C.POINTER(C.c_double)()
        n = C.c_int64()
        self._check(self._fn("scratch_buffer")(self._h, C.byref(ptr), C.byref(n)), "scratch_buffer")
        return C.cast(ptr, C.c_void_p).value, n.value

    def shard_info(self):
        """(info dict, front_owner[n_fronts] with -1 = cap, factor_owned[n_factors]) of the current ordering."""
        info = ShardInfo()
        n = C.c_int32()
        self._check(self._fn("get_tree")(self._h, C.byref(n), None, None, None, None, None, None), "get_tree")
        owner = np.zeros(max(n.value, 1), np.int32)
        owned = np.zeros(max(self.arrays.n_factors, 1), np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self._fn("get_shard")(self._h, C.byref(info), ip(owner), ip(owned)), "get_shard")
        d = {k: getattr(info, k) for k, _ in ShardInfo._fields_}
        return d, owner[:n.value], owned[:self.arrays.n_factors]

    def relinearize_partial(self, keys, states=None) -> dict:
        """gsx_relinearize_partial (include/gsx.h): move the variables `keys` to `states` (their packed states one after the
        other; None = the handle's values are already current), re-linearize their factors and re-eliminate only the
        cliques that hold them and their ancestors.  Returns the counts of what was redone."""
        ks = np.ascontiguousarray(keys, dtype=np.uint64)
        st = PartialStats()
        if states is None:
            sp, ns = None, 0
        else:
            sv = np.ascontiguousarray(states, dtype=np.float64)
            sp, ns = sv.ctypes.data_as(C.POINTER(C.c_double)), sv.size
        self._check(self._fn("relinearize_partial")(self._h, ks.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_int32(ks.size),
                                                    sp, C.c_int64(ns), C.byref(st)), "relinearize_partial")
        return {k: getattr(st, k) for k, _ in PartialStats._fields_}

    def backsubstitute_wildfire(self, threshold: float, want_delta: bool = True):
        """gsx_backsubstitute_wildfire (include/gsx.h): ISAM2's partial back-substitution on the resident undamped
        factorization.  Returns (delta or None, number of frontal variables back-substituted)."""
        out = np.zeros(self.tangent_size) if want_delta else None
        cnt = C.c_int64()
        bad = C.c_uint64()
        ptr = out.ctypes.data_as(C.POINTER(C.c_double)) if want_delta else None
        st = self._fn("backsubstitute_wildfire")(self._h, C.c_double(threshold), ptr,
                                                 C.c_int64(self.tangent_size if want_delta else 0),
                                                 C.byref(cnt), C.byref(bad))
        self._check(st, "backsubstitute_wildfire", key=bad.value)
        return out, cnt.value

    def get_ordering(self) -> np.ndarray:
        """gsx_get_ordering: the keys in the handle's current elimination order."""
        out = np.zeros(self.arrays.n_vars, dtype=np.uint64)
        self._check(self._fn("get_ordering")(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64))), "get_ordering")
        return out

    def update(self, arrays: A.ProblemArrays, factor_origin, new_values) -> dict:
        """gsx_update (include/gsx.h) — ISAM2::update's structural part on the live handle: `arrays` is the WHOLE graph
        after the update, factor_origin[i] the index of its factor i in the current graph (-1: new; current factors not
        named are removed), new_values the packed states of the new variables in ascending-key order.  Kept variables
        keep their linearization point and kept factors their [A b]; only the new factors are linearized."""
        fo = np.ascontiguousarray(factor_origin, dtype=np.int32)
        nv = np.ascontiguousarray(new_values, dtype=np.float64)
        if fo.size != arrays.n_factors:
            raise ValueError("factor_origin must have one entry per factor of the updated graph")
        desc = arrays.desc()
        st = UpdateStats()
        try:
            self._check(self._fn("update")(self._h, C.byref(desc), fo.ctypes.data_as(C.POINTER(C.c_int32)),
                                           nv.ctypes.data_as(C.POINTER(C.c_double)) if nv.size else None,
                                           C.c_int64(nv.size), C.byref(st)), "update")
        except A.GsxError:
            # a failure before the switch leaves the handle as it was; one in the middle of it leaves the NEW problem
            # with every state flag dropped (set_values + set_ordering rebuild it): follow whichever the handle holds
            if int(self._fn("state_size", C.c_int64)(self._h)) == int(arrays.values.size) != int(self.arrays.values.size):
                self.arrays, self._desc = arrays, desc
                self.state_size = int(arrays.values.size)
                self.tangent_size = int(self._fn("tangent_size", C.c_int64)(self._h))
                self.jacobian_size = int(self._fn("jacobian_size", C.c_int64)(self._h))
            raise
        self.arrays, self._desc = arrays, desc
        self.state_size = int(self._fn("state_size", C.c_int64)(self._h))
        self.tangent_size = int(self._fn("tangent_size", C.c_int64)(self._h))
        self.jacobian_size = int(self._fn("jacobian_size", C.c_int64)(self._h))
        return {k: getattr(st, k) for k, _ in UpdateStats._fields_}

    def set_block_jacobians(self, first_factor: int, blocks):
        """gsx_set_block_jacobians: refresh the [A b] blocks of the GSX_F_LINEAR factors first_factor.. in place (blocks =
        the factors' m x (sum d + 1) column-major blocks one after the other, unwhitened: the slot's noise model is folded
        in by the library) — the S5 fallback for factor types the backend does not know."""
        bl = [np.asfortranarray(b, dtype=np.float64).ravel(order="F") for b in blocks]
        flat = np.concatenate(bl) if bl else np.zeros(0)
        self._check(self._fn("set_block_jacobians")(self._h, C.c_int32(first_factor), C.c_int32(len(bl)),
                                                    flat.ctypes.data_as(C.POINTER(C.c_double)), C.c_int64(flat.size)),
                    "set_block_jacobians")

    def solve_gfg_h(self, blocks=None):
        """gsx_solve_gfg_h: the linear seam on a kept handle (GSX_F_LINEAR factors only): new numbers, same structure."""
        out = np.zeros(int(self.arrays.var_dims.sum()))
        bad = C.c_uint64()
        if blocks is None:
            bp, nb = None, 0
        else:
            flat = np.concatenate([np.asfortranarray(b, dtype=np.float64).ravel(order="F") for b in blocks])
            bp, nb = flat.ctypes.data_as(C.POINTER(C.c_double)), flat.size
        st = self._fn("solve_gfg_h")(self._h, bp, C.c_int64(nb), out.ctypes.data_as(C.POINTER(C.c_double)),
                                     C.c_int64(out.size), C.byref(bad))
        if st == A.GSX_E_INDETERMINATE:
            raise A.IndeterminantLinearSystemException(bad.value, "solve_gfg_h")
        self._check(st, "solve_gfg_h")
        return out

    def conditional(self, front: int) -> np.ndarray:
        """gsx_get_conditional: [R S d] of clique `front` (gsx_get_tree numbering), n_frontal x n_cols."""
        nf, nc = C.c_int32(), C.c_int32()
        self._check(self._fn("get_conditional")(self._h, C.c_int32(front), C.byref(nf), C.byref(nc), None, C.c_int64(0)),
                    "get_conditional")
        out = np.zeros(nf.value * nc.value)
        self._check(self._fn("get_conditional")(self._h, C.c_int32(front), C.byref(nf), C.byref(nc),
                                                out.ctypes.data_as(C.POINTER(C.c_double)), C.c_int64(out.size)),
                    "get_conditional")
        return out.reshape(nc.value, nf.value).T

    def lm_trial(self, relinearize=True, lam=0.0, diagonal_damping=False, min_diagonal=1e-6, max_diagonal=1e32):
        """One LM trial without the policy (gsx_lm_trial): (linear error at 0, at delta, nonlinear error of the trial)."""
        e0, ed, et = C.c_double(), C.c_double(), C.c_double()
        self._check(self._fn("lm_trial")(self._h, C.c_int32(int(relinearize)), C.c_double(lam),
                                         C.c_int32(int(diagonal_damping)), C.c_double(min_diagonal),
                                         C.c_double(max_diagonal), C.byref(e0), C.byref(ed), C.byref(et)), "lm_trial")
        return e0.value, ed.value, et.value

    # -- the iterative linear solver (include/gsx.h: gsx_solve_pcg / gsx_set_linear_solver) ---------------------------
    def solve_pcg(self, lam=0.0, diagonal_damping=False, min_diagonal=1e-6, max_diagonal=1e32, params=None,
                  want_delta=True):
        """The damped solve by preconditioned conjugate gradients: (delta or None, stats dict)."""
        prm = params if params is not None else pcg_params_default()
        out = np.zeros(self.tangent_size) if want_delta else None
        st_out, bad = A.PCGStats(), C.c_uint64(0)
        ptr = out.ctypes.data_as(C.POINTER(C.c_double)) if want_delta else None
        st = self._fn("solve_pcg")(self._h, C.c_double(lam), C.c_int32(int(diagonal_damping)), C.c_double(min_diagonal),
                                   C.c_double(max_diagonal), C.byref(prm), ptr,
                                   C.c_int64(self.tangent_size if want_delta else 0), C.byref(st_out), C.byref(bad))
        self._check(st, "solve_pcg", key=bad.value)
        return out, {k: getattr(st_out, k) for k, _ in A.PCGStats._fields_}

    def set_linear_solver(self, kind: int, params=None):
        """kind = A.SOLVER_MULTIFRONTAL or A.SOLVER_PCG (params: A.PCGParams, None = the defaults)."""
        self._check(self._fn("set_linear_solver")(self._h, C.c_int32(kind), C.byref(params) if params is not None else None),
                    "set_linear_solver")

    def smart_points(self):
        """SmartProjectionFactor::point() of every smart factor in graph order (gsx_smart_points): (points [n, 3] — NaN
        unless VALID —, status [n] — A.TRI_* or -1 when the factor was never triangulated)."""
        n = int(np.count_nonzero(self.arrays.f_type == A.F_SMART_PROJECTION))
        pts, st = np.full((n, 3), np.nan), np.full(n, -1, np.int32)
        self._check(self._fn("smart_points")(self._h, pts.ctypes.data_as(C.POINTER(C.c_double)),
                                             st.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int64(n)), "smart_points")
        return pts, st

    def stats(self) -> dict:
        s = A.SmartStats()
        self._check(self._fn("get_stats")(self._h, C.byref(s)), "get_stats")
        return s.as_dict()

    def reset_stats(self):
        self._check(self._fn("reset_stats")(self._h), "reset_stats")

    def set_profiling(self, level: int):
        self._check(self._fn("set_profiling")(self._h, C.c_int32(level)), "set_profiling")

    def synchronize(self):
        self._check(self._fn("synchronize")(self._h), "synchronize")

    def kernel_time(self, name: str):
        ms, n = C.c_double(), C.c_int64()
        self._check(self._fn("kernel_time")(self._h, name.encode(), C.byref(ms), C.byref(n)), "kernel_time")
        return ms.value, n.value


def pcg_params_default() -> A.PCGParams:
    """gsx_pcg_params_default: ConjugateGradientParameters() with the block-Jacobi preconditioner."""
    p = A.PCGParams()
    f = load().gsx_pcg_params_default
    f.restype = None
    f(C.byref(p))
    return p


def _dataset_to_arrays(ds, meta) -> A.ProblemArrays:
    lib = load()
    desc = A.ProblemDesc()
    vals, nvals = C.POINTER(C.c_double)(), C.c_int64()
    st = lib.gsx_dataset_get(ds, C.byref(desc), C.byref(vals), C.byref(nvals))
    if st != A.GSX_OK:
        lib.gsx_dataset_free(ds)
        raise A.GsxError(st, "gsx_dataset_get", "")
    nv, nf = desc.n_vars, desc.n_factors

    def arr(ptr, n, dtype):
        if int(n) == 0:      # (an empty vector hands out a null pointer: a problem without factors)
            return np.zeros(0, dtype=dtype)
        return np.ctypeslib.as_array(ptr, shape=(max(int(n), 1),))[:int(n)].astype(dtype, copy=True)
    kp = arr(desc.f_key_ptr, nf + 1, np.int32)
    mp = arr(desc.f_meas_ptr, nf + 1, np.int64)
    npx = arr(desc.f_noise_ptr, nf + 1, np.int64)
    out = A.ProblemArrays(
        var_keys=arr(desc.var_keys, nv, np.uint64), var_types=arr(desc.var_types, nv, np.int32),
        var_dims=arr(desc.var_dims, nv, np.int32), f_type=arr(desc.f_type, nf, np.int32),
        f_rows=arr(desc.f_rows, nf, np.int32), f_key_ptr=kp, f_vars=arr(desc.f_vars, kp[-1], np.int32),
        f_meas_ptr=mp, meas=arr(desc.meas, mp[-1], np.float64), f_noise_kind=arr(desc.f_noise_kind, nf, np.int32),
        f_noise_ptr=npx, noise=arr(desc.noise, npx[-1], np.float64),
        values=arr(vals, nvals.value, np.float64), meta=meta)
    lib.gsx_dataset_free(ds)
    return out


def read_g2o(path: str, is3D: bool = False) -> A.ProblemArrays:
    """Native g2o reader (gsx_read_g2o, include/gsx.h): graph + anchoring prior + initial values."""
    lib = load()
    lib.gsx_read_g2o.restype = C.c_int32
    lib.gsx_dataset_get.restype = C.c_int32
    lib.gsx_dataset_free.restype = None
    ds = C.c_void_p()
    st = lib.gsx_read_g2o(str(path).encode(), C.c_int32(1 if is3D else 0), C.byref(ds))
    if st != A.GSX_OK:
        raise A.GsxError(st, "gsx_read_g2o", str(path))
    return _dataset_to_arrays(ds, dict(kind="pose3" if is3D else "pose2", source=str(path)))


def load2d(path: str, model_sigmas=None, max_index: int = 0, smart: bool = True,
           noise_format: int = A.NOISE_FORMAT_AUTO, kernel: int = 0) -> A.ProblemArrays:
    """load2D of the reference (gsx_load2d, include/gsx.h): TORO / "graph" 2-D files with poses, landmarks, odometry and
    bearing-range measurements; landmark j has key Symbol('l', j)."""
    lib = load()
    lib.gsx_load2d.restype = C.c_int32
    lib.gsx_dataset_get.restype = C.c_int32
    lib.gsx_dataset_free.restype = None
    ds = C.c_void_p()
    ms = None
    if model_sigmas is not None:
        ms = np.ascontiguousarray(model_sigmas, dtype=np.float64)
        assert ms.size == 3
    st = lib.gsx_load2d(str(path).encode(), None if ms is None else ms.ctypes.data_as(C.POINTER(C.c_double)),
                        C.c_int64(max_index), C.c_int32(int(smart)), C.c_int32(noise_format), C.c_int32(kernel),
                        C.byref(ds))
    if st != A.GSX_OK:
        raise A.GsxError(st, "gsx_load2d", str(path))
    return _dataset_to_arrays(ds, dict(kind="planar", source=str(path)))


def read_bal(path: str, priors: bool = False) -> A.ProblemArrays:
    """Native BAL reader (gsx_read_bal, include/gsx.h)."""
    lib = load()
    lib.gsx_read_bal.restype = C.c_int32
    lib.gsx_dataset_get.restype = C.c_int32
    lib.gsx_dataset_free.restype = None
    ds = C.c_void_p()
    st = lib.gsx_read_bal(str(path).encode(), C.c_int32(1 if priors else 0), C.byref(ds))
    if st != A.GSX_OK:
        raise A.GsxError(st, "gsx_read_bal", str(path))
    return _dataset_to_arrays(ds, dict(kind="bal", source=str(path)))


def write_g2o(path: str, arrays: A.ProblemArrays, packed_values) -> None:
    """Native g2o writer (gsx_write_g2o, include/gsx.h)."""
    lib = load()
    lib.gsx_write_g2o.restype = C.c_int32
    vals = np.ascontiguousarray(packed_values, dtype=np.float64)
    desc = arrays.desc()
    st = lib.gsx_write_g2o(C.byref(desc), vals.ctypes.data_as(C.POINTER(C.c_double)), C.c_int64(vals.size),
                           str(path).encode())
    if st != A.GSX_OK:
        raise A.GsxError(st, "gsx_write_g2o", str(path))


def save2d(path: str, arrays: A.ProblemArrays, packed_values, model_sigmas) -> None:
    """save2D of the reference (gsx_save2d, include/gsx.h): TORO VERTEX2 / EDGE2 file."""
    lib = load()
    lib.gsx_save2d.restype = C.c_int32
    vals = np.ascontiguousarray(packed_values, dtype=np.float64)
    ms = np.ascontiguousarray(model_sigmas, dtype=np.float64)
    assert ms.size == 3
    desc = arrays.desc()
    st = lib.gsx_save2d(C.byref(desc), vals.ctypes.data_as(C.POINTER(C.c_double)), C.c_int64(vals.size),
                        ms.ctypes.data_as(C.POINTER(C.c_double)), str(path).encode())
    if st != A.GSX_OK:
        raise A.GsxError(st, "gsx_save2d", str(path))


def write_bal(path: str, arrays: A.ProblemArrays, packed_values) -> None:
    """writeBALfromValues of the reference (gsx_write_bal, include/gsx.h)."""
    lib = load()
    lib.gsx_write_bal.restype = C.c_int32
    vals = np.ascontiguousarray(packed_values, dtype=np.float64)
    desc = arrays.desc()
    st = lib.gsx_write_bal(C.byref(desc), vals.ctypes.data_as(C.POINTER(C.c_double)), C.c_int64(vals.size),
                           str(path).encode())
    if st != A.GSX_OK:
        raise A.GsxError(st, "gsx_write_bal", str(path))


def dogleg_point(delta: float, dx_u, dx_n) -> np.ndarray:
    """DoglegOptimizerImpl::ComputeDoglegPoint (gsx_dogleg_point, host)."""
    u = np.ascontiguousarray(dx_u, dtype=np.float64)
    n = np.ascontiguousarray(dx_n, dtype=np.float64)
    out = np.zeros_like(u)
    f = load().gsx_dogleg_point
    f.restype = C.c_int32
    st = f(C.c_double(delta), u.ctypes.data_as(C.POINTER(C.c_double)), n.ctypes.data_as(C.POINTER(C.c_double)),
           C.c_int64(u.size), out.ctypes.data_as(C.POINTER(C.c_double)))
    if st != A.GSX_OK:
        raise A.GsxError(st, "gsx_dogleg_point", "")
    return out


# ---- Pose3 initialization (include/gsx.h: InitializePose3) -----------------------------------------------------------
def _raise_init(st, what):
    if st == A.GSX_E_INDETERMINATE:
        raise A.IndeterminantLinearSystemException(None, what)
    if st != A.GSX_OK:
        raise A.GsxError(st, what, "")


def _n_pose3(arrays) -> int:
    return int(np.count_nonzero(arrays.var_types == A.VAR_POSE3))


def init_pose3_params_default() -> A.InitPose3Params:
    p = A.InitPose3Params()
    f = load().gsx_init_pose3_params_default
    f.restype = None
    f(C.byref(p))
    return p


def initialize_pose3(arrays: A.ProblemArrays, given=None, params: A.InitPose3Params = None, device: int = 0):
    """gsx_initialize_pose3: (packed Values of `arrays`, gradient iterations executed)."""
    f = load().gsx_initialize_pose3
    f.restype = C.c_int32
    desc = arrays.desc()
    out = np.zeros(int(arrays.state_offsets()[-1]))
    it = C.c_int32(0)
    g = None if given is None else np.ascontiguousarray(given, dtype=np.float64)
    st = f(C.byref(desc), None if g is None else A._dptr(g), C.c_int64(0 if g is None else g.size),
           None if params is None else C.byref(params), C.c_int32(device), A._dptr(out), C.c_int64(out.size), C.byref(it))
    _raise_init(st, "gsx_initialize_pose3")
    return out, int(it.value)


def pose3_orientations_chordal(arrays: A.ProblemArrays, device: int = 0) -> np.ndarray:
    """gsx_pose3_orientations_chordal: (P, 3, 3) rotations of the POSE3 variables, in the order of `arrays`."""
    f = load().gsx_pose3_orientations_chordal
    f.restype = C.c_int32
    desc = arrays.desc()
    out = np.zeros(9 * _n_pose3(arrays))
    _raise_init(f(C.byref(desc), C.c_int32(device), A._dptr(out), C.c_int64(out.size)), "gsx_pose3_orientations_chordal")
    return out.reshape(-1, 3, 3)


def pose3_orientations_gradient(arrays: A.ProblemArrays, given, max_iter: int = 10000, set_ref_frame: bool = True,
                                device: int = 0):
    """gsx_pose3_orientations_gradient: ((P, 3, 3) rotations, iterations executed)."""
    f = load().gsx_pose3_orientations_gradient
    f.restype = C.c_int32
    desc = arrays.desc()
    g = None if given is None else np.ascontiguousarray(given, dtype=np.float64)
    out = np.zeros(9 * _n_pose3(arrays))
    it = C.c_int32(0)
    st = f(C.byref(desc), None if g is None else A._dptr(g), C.c_int64(0 if g is None else g.size), C.c_int32(max_iter),
           C.c_int32(int(set_ref_frame)), C.c_int32(device), A._dptr(out), C.c_int64(out.size), C.byref(it))
    _raise_init(st, "gsx_pose3_orientations_gradient")
    return out.reshape(-1, 3, 3), int(it.value)


def pose3_compute_poses(arrays: A.ProblemArrays, rot, single_iter: bool = True, fill=None, device: int = 0) -> np.ndarray:
    """gsx_pose3_compute_poses: packed Values of `arrays`; what the pose graph does not hold keeps the entries of `fill`."""
    f = load().gsx_pose3_compute_poses
    f.restype = C.c_int32
    desc = arrays.desc()
    r = np.ascontiguousarray(rot, dtype=np.float64).reshape(-1)
    n = int(arrays.state_offsets()[-1])
    out = np.zeros(n) if fill is None else np.array(fill, dtype=np.float64).reshape(-1).copy()
    st = f(C.byref(desc), A._dptr(r), C.c_int64(r.size), C.c_int32(int(single_iter)), C.c_int32(device), A._dptr(out),
           C.c_int64(out.size))
    _raise_init(st, "gsx_pose3_compute_poses")
    return out


def closest_rotations(m, device: int = 0) -> np.ndarray:
    """gsx_closest_rotations: Rot3::ClosestTo of every 3 x 3 matrix of `m` (n, 3, 3)."""
    f = load().gsx_closest_rotations
    f.restype = C.c_int32
    a = np.ascontiguousarray(m, dtype=np.float64).reshape(-1, 9)
    out = np.zeros_like(a)
    _raise_init(f(A._dptr(a), C.c_int64(a.shape[0]), C.c_int32(device), A._dptr(out)), "gsx_closest_rotations")
    return out.reshape(-1, 3, 3)


INIT_TIMING_NAMES = ("relaxed_analysis_host_ms", "chordal_blocks_ms", "three_relaxed_solves_ms", "projection_ms",
                     "anchor_analysis_host_ms", "gauss_newton_ms", "gradient_ms", "gradient_iterations")


def pose3_init_timings() -> dict:
    """gsx_pose3_init_timings: the stage times of the last initializer call of the process."""
    f = load().gsx_pose3_init_timings
    f.restype = C.c_int32
    out = np.zeros(len(INIT_TIMING_NAMES))
    _raise_init(f(A._dptr(out), C.c_int32(out.size)), "gsx_pose3_init_timings")
    return dict(zip(INIT_TIMING_NAMES, (float(x) for x in out)))


def pose3_init_structure(arrays: A.ProblemArrays):
    """gsx_pose3_init_structure (host): (edge_from, edge_to, adjacency lists per node); node P = the anchor."""
    f = load().gsx_pose3_init_structure
    f.restype = C.c_int32
    desc = arrays.desc()
    ne = C.c_int32(0)
    _raise_init(f(C.byref(desc), C.byref(ne), None, None, None, None, C.c_int64(0)), "gsx_pose3_init_structure")
    n = ne.value
    P = _n_pose3(arrays)
    ef, et = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    ap, adj = np.zeros(P + 2, np.int32), np.zeros(max(2 * n, 1), np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    _raise_init(f(C.byref(desc), C.byref(ne), ip(ef), ip(et), ip(ap), ip(adj), C.c_int64(2 * n)), "gsx_pose3_init_structure")
    return ef[:n], et[:n], [adj[ap[i]:ap[i + 1]].tolist() for i in range(P + 1)]


# ---- Pose2 initialization (include/gsx.h: lago) ----------------------------------------------------------------------
def _n_pose2(arrays) -> int:
    return int(np.count_nonzero(arrays.var_types == A.VAR_POSE2))


def _given(given):
    g = None if given is None else np.ascontiguousarray(given, dtype=np.float64)
    return g, (None if g is None else A._dptr(g)), C.c_int64(0 if g is None else g.size)


def lago_initialize(arrays: A.ProblemArrays, use_odometric_path: bool = True, given=None, device: int = 0) -> np.ndarray:
    """gsx_lago_initialize: packed Values of `arrays`."""
    f = load().gsx_lago_initialize
    f.restype = C.c_int32
    desc = arrays.desc()
    out = np.zeros(int(arrays.state_offsets()[-1]))
    g, gp, gn = _given(given)
    st = f(C.byref(desc), C.c_int32(int(use_odometric_path)), gp, gn, C.c_int32(device), A._dptr(out), C.c_int64(out.size))
    _raise_init(st, "gsx_lago_initialize")
    return out


def lago_initialize_with_guess(arrays: A.ProblemArrays, given, device: int = 0) -> np.ndarray:
    """gsx_lago_initialize_with_guess: packed Values of `arrays`, (x, y) of `given` and lago's theta."""
    f = load().gsx_lago_initialize_with_guess
    f.restype = C.c_int32
    desc = arrays.desc()
    out = np.zeros(int(arrays.state_offsets()[-1]))
    g, gp, gn = _given(given)
    _raise_init(f(C.byref(desc), gp, gn, C.c_int32(device), A._dptr(out), C.c_int64(out.size)),
                "gsx_lago_initialize_with_guess")
    return out


def lago_initialize_orientations(arrays: A.ProblemArrays, use_odometric_path: bool = True, device: int = 0) -> np.ndarray:
    """gsx_lago_initialize_orientations: one unwrapped angle per POSE2 variable, in the order of `arrays`."""
    f = load().gsx_lago_initialize_orientations
    f.restype = C.c_int32
    desc = arrays.desc()
    out = np.zeros(_n_pose2(arrays))
    st = f(C.byref(desc), C.c_int32(int(use_odometric_path)), C.c_int32(device), A._dptr(out), C.c_int64(out.size))
    _raise_init(st, "gsx_lago_initialize_orientations")
    return out


def lago_structure(arrays: A.ProblemArrays, use_odometric_path: bool = True) -> dict:
    """gsx_lago_structure (host): edge_from, edge_to, parent, delta (node P = the anchor), tree_ids, chord_ids, max_depth."""
    f = load().gsx_lago_structure
    f.restype = C.c_int32
    desc = arrays.desc()
    ne, nt, depth = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    odo = C.c_int32(int(use_odometric_path))
    _raise_init(f(C.byref(desc), odo, C.byref(ne), None, None, None, None, None, None, None, None), "gsx_lago_structure")
    n, P = ne.value, _n_pose2(arrays)
    ef, et, ti, ci = (np.zeros(max(n, 1), np.int32) for _ in range(4))
    parent, delta = np.zeros(P + 1, np.int32), np.zeros(P + 1)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    _raise_init(f(C.byref(desc), odo, C.byref(ne), ip(ef), ip(et), ip(parent), A._dptr(delta), C.byref(nt), ip(ti), ip(ci),
                  C.byref(depth)), "gsx_lago_structure")
    return dict(edge_from=ef[:n], edge_to=et[:n], parent=parent, delta=delta, tree_ids=ti[:nt.value],
                chord_ids=ci[:n - nt.value], max_depth=int(depth.value))


def lago_thetas_to_root(parent, delta, device: int = 0) -> np.ndarray:
    """gsx_lago_thetas_to_root: the sum of `delta` from every node of the forest `parent` (a root: itself) to its root."""
    f = load().gsx_lago_thetas_to_root
    f.restype = C.c_int32
    p = np.ascontiguousarray(parent, dtype=np.int32)
    d = np.ascontiguousarray(delta, dtype=np.float64)
    if p.shape != d.shape or p.ndim != 1:
        raise ValueError("parent and delta: one entry per node")
    out = np.zeros(max(p.size, 1))
    _raise_init(f(p.ctypes.data_as(C.POINTER(C.c_int32)), A._dptr(d), C.c_int64(p.size), C.c_int32(device), A._dptr(out)),
                "gsx_lago_thetas_to_root")
    return out[:p.size]


def lago_regularized_measurements(arrays: A.ProblemArrays, use_odometric_path: bool = True, device: int = 0) -> np.ndarray:
    """gsx_lago_regularized_measurements: the regularized deltaTheta of every pose-graph edge, in edge order."""
    f = load().gsx_lago_regularized_measurements
    f.restype = C.c_int32
    desc = arrays.desc()
    ne = C.c_int32(0)
    g = load().gsx_lago_structure
    g.restype = C.c_int32
    _raise_init(g(C.byref(desc), C.c_int32(int(use_odometric_path)), C.byref(ne), None, None, None, None, None, None, None,
                  None), "gsx_lago_structure")
    out = np.zeros(max(ne.value, 1))
    st = f(C.byref(desc), C.c_int32(int(use_odometric_path)), C.c_int32(device), A._dptr(out), C.c_int64(ne.value))
    _raise_init(st, "gsx_lago_regularized_measurements")
    return out[:ne.value]


LAGO_TIMING_NAMES = ("orientation_analysis_host_ms", "theta_to_root_ms", "orientation_blocks_ms", "orientation_solve_ms",
                     "pose_analysis_host_ms", "pose_blocks_ms", "pose_solve_ms", "compose_ms")


def lago_timings() -> dict:
    """gsx_lago_timings: the stage times of the last lago call of the process."""
    f = load().gsx_lago_timings
    f.restype = C.c_int32
    out = np.zeros(len(LAGO_TIMING_NAMES))
    _raise_init(f(A._dptr(out), C.c_int32(out.size)), "gsx_lago_timings")
    return dict(zip(LAGO_TIMING_NAMES, (float(x) for x in out)))


# ---- landmark triangulation (include/gsx.h: gsx_triangulate*) -----------------------------------------------------------
def triangulation_params_default() -> A.TriangulationParams:
    p = A.TriangulationParams()
    f = load().gsx_triangulation_params_default
    f.restype = None
    f(C.byref(p))
    return p


def triangulate(camera_kind: int, cameras, calibrations, track_ptr, obs_camera, obs_xy, params: A.TriangulationParams = None,
                device: int = 0, with_counts: bool = False):
    """gsx_triangulate: (points (n, 3), statuses (n,)[, LM counts (n, 2)]).  cameras (n_cam, 12) Pose3 states with
    calibrations (1 or n_cam, 5), or (n_cam, 17) camera states with calibrations None."""
    f = load().gsx_triangulate
    f.restype = C.c_int32
    width = 17 if camera_kind == A.CAMERA_CAL3BUNDLER else 12
    cam = np.ascontiguousarray(cameras, dtype=np.float64).reshape(-1, width)
    cal = None if calibrations is None else np.ascontiguousarray(calibrations, dtype=np.float64).reshape(-1, 5)
    ptr = np.ascontiguousarray(track_ptr, dtype=np.int64)
    oc = np.ascontiguousarray(obs_camera, dtype=np.int32)
    xy = np.ascontiguousarray(obs_xy, dtype=np.float64).reshape(-1, 2)
    if ptr.size < 1 or oc.size != xy.shape[0] or int(ptr[-1]) != oc.size:
        raise ValueError("track_ptr must index obs_camera / obs_xy")
    n = ptr.size - 1
    points, status, counts = np.zeros((max(n, 1), 3)), np.zeros(max(n, 1), np.int32), np.zeros((max(n, 1), 2), np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    st = f(C.c_int32(camera_kind), A._dptr(cam) if cam.size else None, C.c_int32(cam.shape[0]),
           None if cal is None or cal.size == 0 else A._dptr(cal), C.c_int32(0 if cal is None else cal.shape[0]),
           ptr.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int64(n), ip(oc) if oc.size else None,
           A._dptr(xy) if xy.size else None, None if params is None else C.byref(params), C.c_int32(device),
           A._dptr(points), ip(status), ip(counts) if with_counts else None)
    _raise_init(st, "gsx_triangulate")
    return (points[:n], status[:n], counts[:n]) if with_counts else (points[:n], status[:n])


def triangulation_tracks(arrays: A.ProblemArrays):
    """gsx_triangulation_tracks (host): (landmark variable indices, track_ptr, factor index per observation)."""
    f = load().gsx_triangulation_tracks
    f.restype = C.c_int32
    desc = arrays.desc()
    nl, no = C.c_int32(0), C.c_int64(0)
    _raise_init(f(C.byref(desc), C.byref(nl), C.byref(no), None, None, None), "gsx_triangulation_tracks")
    lm, ptr, of = np.zeros(max(nl.value, 1), np.int32), np.zeros(nl.value + 1, np.int64), np.zeros(max(no.value, 1), np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    _raise_init(f(C.byref(desc), C.byref(nl), C.byref(no), ip(lm), ptr.ctypes.data_as(C.POINTER(C.c_int64)), ip(of)),
                "gsx_triangulation_tracks")
    return lm[:nl.value], ptr, of[:no.value]


def triangulate_landmarks(arrays: A.ProblemArrays, values=None, params: A.TriangulationParams = None, device: int = 0):
    """gsx_triangulate_landmarks: (packed Values with the VALID landmarks overwritten, status per landmark in the order of
    triangulation_tracks)."""
    f = load().gsx_triangulate_landmarks
    f.restype = C.c_int32
    desc = arrays.desc()
    v = np.ascontiguousarray(arrays.values if values is None else values, dtype=np.float64)
    out = np.zeros(max(v.size, 1))
    status = np.zeros(max(arrays.n_vars, 1), np.int32)
    nl = C.c_int32(0)
    st = f(C.byref(desc), A._dptr(v), C.c_int64(v.size), None if params is None else C.byref(params), C.c_int32(device),
           A._dptr(out), status.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nl))
    _raise_init(st, "gsx_triangulate_landmarks")
    return out[:v.size], status[:nl.value]


TRIANGULATE_TIMING_NAMES = ("classes_host_ms", "cameras_ms", "short_tracks_ms", "long_tracks_ms", "total_host_ms")


def triangulate_timings() -> dict:
    """gsx_triangulate_timings: the stage times of the last triangulation call of the process."""
    f = load().gsx_triangulate_timings
    f.restype = C.c_int32
    out = np.zeros(len(TRIANGULATE_TIMING_NAMES))
    _raise_init(f(A._dptr(out), C.c_int32(out.size)), "gsx_triangulate_timings")
    return dict(zip(TRIANGULATE_TIMING_NAMES, (float(x) for x in out)))


# ---- translation averaging (include/gsx.h: gsx_mfas_*, gsx_translation_*) ------------------------------------------------
def mfas_outlier_weights(key1, key2, edge_dirs=None, proj_dirs=None, weights=None, device: int = 0, want_weights: bool = True,
                         want_ordering: bool = False) -> dict:
    """gsx_mfas_outlier_weights: MFAS for D projection directions at once.  Either edge_dirs (E, 3) and proj_dirs (D, 3), or
    weights (D, E).  Returns mean (E,), and when asked for weights (D, E) and ordering (D, n_nodes) keys."""
    f = load().gsx_mfas_outlier_weights
    f.restype = C.c_int32
    k1 = np.ascontiguousarray(key1, dtype=np.uint64).reshape(-1)
    k2 = np.ascontiguousarray(key2, dtype=np.uint64).reshape(-1)
    if k1.shape != k2.shape:
        raise ValueError("key1 and key2: one entry per edge")
    ne = k1.size
    if edge_dirs is not None:
        ed = np.ascontiguousarray(edge_dirs, dtype=np.float64).reshape(-1, 3)
        pd = np.ascontiguousarray(proj_dirs, dtype=np.float64).reshape(-1, 3)
        if ed.shape[0] != ne:
            raise ValueError("edge_dirs: three doubles per edge")
        nd, w = pd.shape[0], None
    else:
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1, max(ne, 1)) if ne else np.zeros((1, 1))
        nd, ed, pd = w.shape[0], None, None
    n_nodes = np.unique(np.concatenate([k1, k2])).size
    mean = np.zeros(max(ne, 1))
    ow = np.zeros((max(nd, 1), max(ne, 1))) if want_weights else None
    oo = np.zeros((max(nd, 1), max(n_nodes, 1)), dtype=np.uint64) if want_ordering else None
    kp = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    st = f(kp(k1) if ne else None, kp(k2) if ne else None, C.c_int64(ne), None if ed is None else A._dptr(ed),
           None if pd is None else A._dptr(pd), None if w is None else A._dptr(w), C.c_int32(nd), C.c_int32(device),
           A._dptr(mean), None if ow is None else A._dptr(ow), None if oo is None else kp(oo))
    _raise_init(st, "gsx_mfas_outlier_weights")
    out = dict(mean=mean[:ne])
    if want_weights:
        out["weights"] = ow[:nd, :ne]
    if want_ordering:
        out["ordering"] = oo[:nd, :n_nodes]
    return out


MFAS_TIMING_NAMES = ("adjacency_host_ms", "mfas_ms", "mean_ms", "total_host_ms")


def mfas_timings() -> dict:
    """gsx_mfas_timings: the stage times of the last MFAS call of the process."""
    f = load().gsx_mfas_timings
    f.restype = C.c_int32
    out = np.zeros(len(MFAS_TIMING_NAMES))
    _raise_init(f(A._dptr(out), C.c_int32(out.size)), "gsx_mfas_timings")
    return dict(zip(MFAS_TIMING_NAMES, (float(x) for x in out)))


def translation_params_default() -> A.TranslationParams:
    p = A.TranslationParams()
    f = load().gsx_translation_params_default
    f.restype = None
    f(C.byref(p))
    return p


def _translation_input(unit, scale, between, given):
    """gsx_translation_input and the arrays it points into.  unit / between: lists of (key1, key2, 3 doubles, noise kind,
    noise parameters); given: {key: 3 doubles}."""
    keep = []

    def pack(edges):
        k1 = np.array([e[0] for e in edges], dtype=np.uint64)
        k2 = np.array([e[1] for e in edges], dtype=np.uint64)
        z = np.array([np.asarray(e[2], dtype=float).reshape(3) for e in edges], dtype=np.float64).reshape(-1)
        kind = np.array([e[3] for e in edges], dtype=np.int32)
        params = [np.asarray(e[4], dtype=float).reshape(-1) for e in edges]
        ptr = np.concatenate([[0], np.cumsum([q.size for q in params])]).astype(np.int64)
        noise = np.concatenate(params + [np.zeros(1)])
        keep.extend([k1, k2, z, kind, ptr, noise])
        if not edges:
            return 0, None, None, None, None, None, None
        return (len(edges), k1.ctypes.data_as(C.POINTER(C.c_uint64)), k2.ctypes.data_as(C.POINTER(C.c_uint64)), A._dptr(z),
                kind.ctypes.data_as(C.POINTER(C.c_int32)), ptr.ctypes.data_as(C.POINTER(C.c_int64)), A._dptr(noise))
    u, b = pack(list(unit)), pack(list(between))
    gk = np.array(sorted(given), dtype=np.uint64)
    gv = np.array([np.asarray(given[int(k)], dtype=float).reshape(3) for k in gk], dtype=np.float64).reshape(-1)
    keep.extend([gk, gv])
    inp = A.TranslationInput(u[0], u[1], u[2], u[3], u[4], u[5], u[6], float(scale), b[0], b[1], b[2], b[3], b[4], b[5], b[6],
                             gk.size, gk.ctypes.data_as(C.POINTER(C.c_uint64)) if gk.size else None,
                             A._dptr(gv) if gk.size else None)
    return inp, keep


def translation_recovery_problem(unit, scale=1.0, between=(), given=None, params: A.TranslationParams = None):
    """gsx_translation_recovery_problem (host): (ProblemArrays with the initial values, {merged key: its representative})."""
    lib = load()
    f = lib.gsx_translation_recovery_problem
    f.restype = C.c_int32
    lib.gsx_dataset_get.restype = C.c_int32
    lib.gsx_dataset_free.restype = None
    unit, between = list(unit), list(between)
    inp, keep = _translation_input(unit, scale, between, given or {})
    p = params if params is not None else translation_params_default()
    n = max(2 * len(unit), 1)
    mk, mi, nm = np.zeros(n, np.uint64), np.zeros(n, np.uint64), C.c_int64(0)
    ds = C.c_void_p()
    st = f(C.byref(inp), C.byref(p), C.byref(ds), mk.ctypes.data_as(C.POINTER(C.c_uint64)),
           mi.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(nm))
    _raise_init(st, "gsx_translation_recovery_problem")
    arrays = _dataset_to_arrays(ds, dict(kind="translation"))
    return arrays, {int(a): int(b) for a, b in zip(mk[:nm.value], mi[:nm.value])}


def translation_recovery(unit, scale=1.0, between=(), given=None, params: A.TranslationParams = None, device: int = 0):
    """gsx_translation_recovery: ({key: translation}, LM result dict)."""
    f = load().gsx_translation_recovery
    f.restype = C.c_int32
    unit, between = list(unit), list(between)
    inp, keep = _translation_input(unit, scale, between, given or {})
    p = params if params is not None else translation_params_default()
    n = max(2 * (len(unit) + len(between)), 1)
    keys, out, n_out, r = np.zeros(n, np.uint64), np.zeros(3 * n), C.c_int64(0), A.LMResult()
    st = f(C.byref(inp), C.byref(p), C.c_int32(device), keys.ctypes.data_as(C.POINTER(C.c_uint64)), A._dptr(out),
           C.byref(n_out), C.byref(r))
    _raise_init(st, "gsx_translation_recovery")
    result = {int(k): out[3 * i:3 * i + 3].copy() for i, k in enumerate(keys[:n_out.value])}
    return result, dict(initial_error=r.initial_error, final_error=r.final_error, final_lambda=r.final_lambda,
                        iterations=r.iterations, inner_iterations=r.inner_iterations)


def product_backend(arrays: A.ProblemArrays, device: int = 0) -> ProductBackend:
    return ProductBackend(arrays, device)
