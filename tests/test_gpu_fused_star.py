"""Star leaves eliminated straight from [A b] (kernels.hip: front_star_leaf_kernel) against the two-step path (star
assembly of the H panels, then front_leaf), which a handle created under GSX_FUSED_STAR=0 keeps: bit for bit.

Both handles see the same arrays and the same ordering, so every comparison below is np.array_equal (or ==), never a
tolerance: solves at lambda I and with diagonal damping, the linearized errors, LM trials and whole LM traces, the
conditionals of landmark cliques, diag(H) and Dogleg after a fused step, robust noise, a landmark seen by more than 64
cameras, a repeated camera-landmark pair, and the failures a cheirality or an indefinite landmark produces.
"""
import numpy as np
import pytest

from gtsam_petercdev_amd import _abi as A
from gtsam_petercdev_amd import datasets

from ._switches import switches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from gtsam_petercdev_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the HIP path has no fallback"
    return _lib


def _handles(gpu, arr, ordering=None):
    """(fused handle, two-step handle) with the same ordering (the switch is read when a handle is created)."""
    fused = gpu.product_backend(arr)
    with switches(GSX_FUSED_STAR="0"):
        two = gpu.product_backend(arr)
    if ordering is None:
        ordering = fused.compute_ordering(A.ORDER_SCHUR)
    fused.set_ordering(ordering)
    two.set_ordering(ordering)
    return fused, two


def _landmark_cliques(be, arr, k=4):
    """A few cliques whose only frontal variable is a landmark (spread over the tree numbering; the tiny dubrovnik
    bundle under its reference ordering has none)."""
    _, fronts = be.get_tree()
    ids = [c for c, (f, _) in enumerate(fronts) if len(f) == 1 and arr.var_types[f[0]] == A.VAR_VECTOR]
    assert ids or arr.n_vars < 20
    return [ids[i] for i in np.linspace(0, len(ids) - 1, min(k, len(ids))).astype(int)]


def _bal49():
    return datasets.synth_bal_arrays(49, 7776, 31843, seed=42, long_range=0.3)


def _dubrovnik(gpu, golden_dir):
    return gpu.read_bal(golden_dir + "/dubrovnik-3-7-pre.txt")


def _huber(arr, k=1.5):
    """Every projection factor under a Huber loss."""
    kinds, ptr, vals = [], [0], []
    for f in range(arr.n_factors):
        p = arr.noise[arr.f_noise_ptr[f]:arr.f_noise_ptr[f + 1]]
        kind = int(arr.f_noise_kind[f])
        if arr.f_type[f] == A.F_SFM:
            kind |= A.NOISE_ROBUST_HUBER
            p = np.concatenate([p, [k]])
        kinds.append(kind)
        vals.append(p)
        ptr.append(ptr[-1] + p.size)
    return A.ProblemArrays(arr.var_keys, arr.var_types, arr.var_dims, arr.f_type, arr.f_rows, arr.f_key_ptr, arr.f_vars,
                           arr.f_meas_ptr, arr.meas, kinds, ptr, np.concatenate(vals), arr.values, dict(arr.meta))


def _sfm_pairs(arr):
    kp = arr.f_key_ptr
    return [(int(arr.f_vars[kp[f]]), int(arr.f_vars[kp[f] + 1]), f) for f in range(arr.n_factors)
            if arr.f_type[f] == A.F_SFM]


def _wide_landmark():
    """A bundle whose first landmark is seen by every one of 90 cameras (the factor list of its clique spans two
    64-factor chunks of the fused kernel), measurements copied from the landmark's own observations."""
    arr = datasets.synth_bal_arrays(90, 120, 1500, seed=23, long_range=0.5)
    pairs = _sfm_pairs(arr)
    lm = pairs[0][1]
    seen = {c for c, l, _ in pairs if l == lm}
    f0 = pairs[0][2]
    meas = arr.meas[arr.f_meas_ptr[f0]:arr.f_meas_ptr[f0 + 1]]
    noise = arr.noise[arr.f_noise_ptr[f0]:arr.f_noise_ptr[f0 + 1]]
    cams = [v for v in range(arr.n_vars) if arr.var_types[v] == A.VAR_CAMERA]
    for c in cams:
        if c not in seen:
            arr = arr.with_factor(A.F_SFM, [c, lm], 2, meas, int(arr.f_noise_kind[f0]), noise)
    assert sum(1 for _, l, _ in _sfm_pairs(arr) if l == lm) > 64
    return arr


def _repeated_pair():
    """One camera-landmark observation twice: that landmark is not a star variable (two factors share a partner block),
    its clique takes the two-step path inside a fused launch group."""
    arr = datasets.synth_bal_arrays(30, 400, 2400, seed=24, long_range=0.3)
    c, l, f0 = _sfm_pairs(arr)[5]
    meas = arr.meas[arr.f_meas_ptr[f0]:arr.f_meas_ptr[f0 + 1]] + 0.25
    noise = arr.noise[arr.f_noise_ptr[f0]:arr.f_noise_ptr[f0 + 1]]
    return arr.with_factor(A.F_SFM, [c, l], 2, meas, int(arr.f_noise_kind[f0]), noise)


def _check_linear(gpu, arr, ordering=None, lams=(1e-3, 1.0)):
    fb, tb = _handles(gpu, arr, ordering)
    fb.linearize()
    tb.linearize()
    assert np.array_equal(fb.jacobians(), tb.jacobians())
    for lam in lams:
        df, dt = fb.solve(lam, False), tb.solve(lam, False)
        assert np.array_equal(df, dt), (lam, float(np.max(np.abs(df - dt))))
        assert fb.linear_error() == tb.linear_error()
        for c in _landmark_cliques(fb, arr):
            assert np.array_equal(fb.conditional(c), tb.conditional(c)), (lam, c)
    df, dt = fb.solve(1e-4, True), tb.solve(1e-4, True)      # diagonal damping: diag(H) of every panel
    assert np.array_equal(df, dt)
    assert fb.linear_error() == tb.linear_error()
    assert np.array_equal(fb.hessian_diagonal(), tb.hessian_diagonal())
    assert fb.lm_trial(True, 1e-3) == tb.lm_trial(True, 1e-3)
    assert fb.lm_trial(False, 1e-1) == tb.lm_trial(False, 1e-1)       # a second lambda on the same linearization
    assert fb.lm_trial(False, 1e-2, diagonal_damping=True) == tb.lm_trial(False, 1e-2, diagonal_damping=True)
    return fb, tb


def _check_lm(fb, tb, iters=6):
    p = A.lm_params_legacy()
    p.max_iterations = iters
    rf, rt = fb.lm_optimize(p), tb.lm_optimize(p)
    for k in rf:
        if isinstance(rf[k], np.ndarray):
            assert np.array_equal(rf[k], rt[k]), k
        else:
            assert rf[k] == rt[k], k
    assert np.array_equal(fb.get_values(), tb.get_values())


def test_bal49_bitwise(gpu):
    arr = _bal49()
    fb, tb = _check_linear(gpu, arr)
    _check_lm(fb, tb)


def test_dubrovnik_bitwise(gpu, golden_dir):
    arr = _dubrovnik(gpu, golden_dir)
    order = np.load(golden_dir + "/dubrovnik_colamd_ordering.npy")
    fb, tb = _check_linear(gpu, arr, order)
    p = A.lm_params_legacy()
    rf, rt = fb.lm_optimize(p), tb.lm_optimize(p)
    assert rf["final_error"] == rt["final_error"] and rf["iterations"] == rt["iterations"]
    assert np.array_equal(fb.get_values(), tb.get_values())


def test_bal1723_bitwise(gpu):
    arr = datasets.synth_bal_arrays(1723, 156502, 678718, seed=42, long_range=0.3)
    fb, tb = _handles(gpu, arr)
    fb.linearize()
    tb.linearize()
    for lam in (1e-5, 1e-2):
        assert np.array_equal(fb.solve(lam, False), tb.solve(lam, False)), lam
        assert fb.linear_error() == tb.linear_error()
    for c in _landmark_cliques(fb, arr, 6):
        assert np.array_equal(fb.conditional(c), tb.conditional(c)), c
    assert np.array_equal(fb.solve(1e-5, True), tb.solve(1e-5, True))
    assert np.array_equal(fb.hessian_diagonal(), tb.hessian_diagonal())
    assert fb.lm_trial(True, 1e-5) == tb.lm_trial(True, 1e-5)
    _check_lm(fb, tb, iters=3)


def test_dogleg_after_a_fused_step(gpu):
    arr = _bal49()
    fb, tb = _handles(gpu, arr)
    fb.linearize()
    tb.linearize()
    assert np.array_equal(fb.solve(1e-3, False), tb.solve(1e-3, False))   # a fused factorization first
    rf, rt = fb.dogleg_optimize(1.0, 5), tb.dogleg_optimize(1.0, 5)
    assert rf["final_error"] == rt["final_error"] and rf["iterations"] == rt["iterations"]
    assert np.array_equal(fb.get_values(), tb.get_values())


def test_huber_bitwise(gpu):
    arr = _huber(datasets.synth_bal_arrays(40, 2000, 9000, seed=25, long_range=0.3))
    fb, tb = _check_linear(gpu, arr)
    _check_lm(fb, tb, iters=4)


def test_landmark_seen_by_more_than_64_cameras(gpu):
    arr = _wide_landmark()
    fb, tb = _check_linear(gpu, arr)
    _check_lm(fb, tb, iters=4)


def test_repeated_camera_landmark_pair(gpu):
    arr = _repeated_pair()
    fb, tb = _check_linear(gpu, arr)
    _check_lm(fb, tb, iters=4)


def test_failures_reported_identically(gpu):
    # an indefinite system (negative damping): every landmark pivot fails; the first failing front and its key agree
    arr = _bal49()
    fb, tb = _handles(gpu, arr)
    fb.linearize()
    tb.linearize()
    keys = []
    for be in (fb, tb):
        with pytest.raises(A.IndeterminantLinearSystemException) as ei:
            be.solve(-1e6, False)
        keys.append((ei.value.key, str(ei.value)))
    assert keys[0] == keys[1]
    # and the handles agree again at a positive damping
    assert np.array_equal(fb.solve(1e-3, False), tb.solve(1e-3, False))
    # a landmark behind a camera: its factor is zeroed (cheirality), both handles count it and solve alike
    arr = datasets.synth_bal_arrays(30, 400, 2400, seed=26, long_range=0.3)
    so = arr.state_offsets()
    lm = _sfm_pairs(arr)[0][1]
    vals = arr.values.copy()
    vals[so[lm]:so[lm + 1]] *= -50.0
    arr = A.ProblemArrays(arr.var_keys, arr.var_types, arr.var_dims, arr.f_type, arr.f_rows, arr.f_key_ptr, arr.f_vars,
                          arr.f_meas_ptr, arr.meas, arr.f_noise_kind, arr.f_noise_ptr, arr.noise, vals, dict(arr.meta))
    fb, tb = _handles(gpu, arr)
    fb.linearize()
    tb.linearize()
    assert fb.stats()["n_cheirality"] == tb.stats()["n_cheirality"]
    res = []
    for be in (fb, tb):
        try:
            res.append(be.solve(0.0, False))
        except A.IndeterminantLinearSystemException as e:
            res.append((e.key, str(e)))
    assert type(res[0]) is type(res[1])
    if isinstance(res[0], np.ndarray):
        assert np.array_equal(res[0], res[1])
    else:
        assert res[0] == res[1]
    assert fb.lm_trial(False, 1e-3) == tb.lm_trial(False, 1e-3)
