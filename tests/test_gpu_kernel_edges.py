"""Every linearize_* kernel, the error kernels and retract_kernel at the edges of their branches, against the
50-digit restatement of tests/_mp_restatement.py (pinned by tests/test_host_restatement.py; NOT a twin of
csrc/device_geometry.h as oracle/geometry.h is).  A sweep packs its cases into ONE graph, factor i = case i, several hundred
factors and never a multiple of 256: one handle and one gsx_linearize judge all of it, across block boundaries.

Bounds.  [A b] and states: the project's rule, atol = 1e-13 max(1, max |expected|), over the whole graph as in
tests/test_gpu_factor_types.py AND per block (per variable for states) — a block of entries O(1) is not excused by a
neighbour of entries 1e8.  The three SO(3) ladders hold the graph-wide form only: their angle pi - 0.04 sits just outside
the near-pi branch, where theta / (2 sin theta) amplifies the rounding of the rotation matrix by theta / (4 sin^2 theta) =
490 and the translation part of Pose3::Logmap multiplies that by |T|; a float64 numpy port of the reference's formulas is
itself 0.5 - 0.8 of the per-block bound away from the 50-digit value there (5.7e-12 on a block of largest entry 71, every
worst case at that angle), so per block the comparison would measure the number format, not the kernel.  Their worst
per-block ratio is printed.  Graph error: error_bound of tests/test_gpu_factor_types.py.  Steps: the pattern and
the 1e-6 of check_steps there, against a dense solve of the restated system.

Thresholds are approached to a relative 1e-9 and no closer (the device contracts to FMA).  Where a threshold is straddled the
rotation / offset that decides is an INPUT (identity partner poses), so that both sides see the same doubles.

Inputs are shaped so that the float64 evaluation is well conditioned, because the bound above is about the kernel, not about
the conditioning of its input: a camera-frame depth of 1e-6 is a point 1e-6 from the camera centre (p - t exact), not the
cancelled difference of O(1) coordinates; robust corners carry residuals of many ulps of the prediction (pixel families:
sigmas of hundreds of pixels), see the note in tests/_factor_restatement.random_graph."""
import math

import mpmath as mp
import numpy as np
import pytest

from gtsam_petercdev_amd import _abi as A, _lib
from tests import _factor_restatement as R
from tests import _mp_restatement as M
from tests.test_gpu_factor_types import backend, error_bound

pytestmark = pytest.mark.gpu

P2, P3, V, CAM = A.VAR_POSE2, A.VAR_POSE3, A.VAR_VECTOR, A.VAR_CAMERA
EYE = np.eye(3)
LOSSES = {"huber": A.NOISE_ROBUST_HUBER, "tukey": A.NOISE_ROBUST_TUKEY, "cauchy": A.NOISE_ROBUST_CAUCHY}


class Graph:
    """Variables in ascending key order, factors in case order; arrays() appends one soft prior a variable (after the
    cases, so factor i stays case i) to make the Hessian regular for the solve check."""

    def __init__(self):
        self.vars, self.vals, self.factors, self.prior_sigma = [], [], [], []

    def var(self, vt, dim, state, prior_sigma=0.5):
        self.vars.append((len(self.vars), vt, dim))
        self.vals.append(np.asarray(state, float))
        self.prior_sigma.append(prior_sigma)
        return len(self.vars) - 1

    def factor(self, ft, vs, m, z, kind=A.NOISE_UNIT, params=()):
        self.factors.append((ft, list(vs), m, np.asarray(z, float), kind, params))
        return len(self.factors) - 1

    def arrays(self, priors=True):
        factors = list(self.factors)
        if priors:
            for (v, _vt, dim), st, sg in zip(self.vars, self.vals, self.prior_sigma):
                factors.append((A.F_PRIOR, [v], dim, st, A.NOISE_ISOTROPIC, [sg]))
        return R.make_arrays(self.vars, factors, np.concatenate(self.vals))


def blocks(arr, flat):
    off = arr.jacobian_offsets()
    return [flat[off[f]:off[f + 1]] for f in range(arr.n_factors)]


def judge(arr, what, n_cases=None, solve=True, no_solve_reason=None, ragged=True, per_block=True, graph_wide_only=()):
    """One handle, one gsx_linearize: every [A b] block, the graph error and (solve=True) one damped step at lambda 0 and
    1e-3 against the restatement.  Returns (device blocks, restated blocks, device cheirality count, restated flags)."""
    n_cases = arr.n_factors if n_cases is None else n_cases
    assert n_cases % 256 != 0 or not ragged
    be = backend(arr)
    be.linearize()
    got = be.jacobians()
    want_blocks, flags = [], []
    for f in range(arr.n_factors):
        Ab, cheir = M.linearized(arr, arr.values, f)
        want_blocks.append(Ab.reshape(-1, order="F"))
        flags.append(cheir)
    want = np.concatenate(want_blocks)
    assert got.shape == want.shape
    got_blocks = blocks(arr, got)
    worst_ratio, worst_abs, worst_f = 0.0, 0.0, -1
    for f, (g, w) in enumerate(zip(got_blocks, want_blocks)):
        assert np.all(np.isfinite(g)), (what, f)
        d = float(np.max(np.abs(g - w)))
        ratio = d / (1e-13 * max(1.0, float(np.max(np.abs(w)))))
        if ratio > worst_ratio and f not in graph_wide_only:
            worst_ratio, worst_abs, worst_f = ratio, d, f
    scale = max(1.0, float(np.max(np.abs(want))))
    eg, ew = be.error(), M.graph_error(arr, arr.values)
    print(f"{what}: {n_cases} cases ({arr.n_factors} factors), worst |[A b] - restated| = {worst_abs:.3e} at factor {worst_f} = "
          f"{worst_ratio:.3f} of its bound 1e-13 max(1, max |block|); graph-wide {float(np.max(np.abs(got - want))):.3e} against "
          f"{1e-13 * scale:.3e}; error {eg:.12g} vs {ew:.12g} (diff {abs(eg - ew):.3e}, bound {error_bound(arr, scale, ew):.3e})")
    assert float(np.max(np.abs(got - want))) <= 1e-13 * scale, (what, worst_f, worst_abs)
    if per_block:
        assert worst_ratio <= 1.0, (what, worst_f, worst_abs)
    assert abs(eg - ew) <= error_bound(arr, scale, ew), (what, eg, ew)
    n_cheir = be.stats()["n_cheirality"]
    if solve:
        J, b = M.dense_system(arr, arr.values, blocks=[w.reshape(int(arr.f_rows[f]), -1, order="F") for f, w in enumerate(want_blocks)])
        H, g = J.T @ J, J.T @ b
        for lam in (0.0, 1e-3):
            want_d = np.linalg.solve(H + lam * np.eye(H.shape[0]), g)
            got_d = be.solve(lam, False)
            rel = float(np.linalg.norm(got_d - want_d) / np.linalg.norm(want_d))
            print(f"{what}: lambda {lam:g}, dim {H.shape[0]}, |step - dense| / |dense| = {rel:.3e}")
            assert rel <= 1e-6, (what, lam, rel)
    else:
        print(f"{what}: no step check — {no_solve_reason}")
        assert no_solve_reason
    be.close()
    return got_blocks, want_blocks, n_cheir, flags


# ---- rotations of the ladder -------------------------------------------------------------------------------------------
def rot_exact(axis, angle):
    """exp(angle [axis]x) at 50 digits, rounded to doubles; angle = pi exactly: 2 a a' - I in doubles, so that W = 0."""
    a = np.asarray(axis, float)
    if angle == math.pi:
        return 2.0 * np.outer(a, a) - EYE
    am = M.vec(a)
    K = M.skew(am)
    Rm = M.lin((1, M.eye3()), (mp.sin(mp.mpf(angle)), K), (1 - mp.cos(mp.mpf(angle)), M.mm(K, K)))
    return np.array([[float(x) for x in row] for row in Rm])


def unit(v):
    v = np.asarray(v, float)
    return v / np.linalg.norm(v)


LADDER = [0.0, 1e-12, 1e-10 * (1 - 1e-9), 1e-10 * (1 + 1e-9), 1e-8, 1e-3 * (1 - 1e-9), 1e-3 * (1 + 1e-9),
          math.sqrt(1e-5) * (1 - 1e-9), math.sqrt(1e-5) * (1 + 1e-9), 0.5, 2.0]
NEAR_PI = [math.pi - 0.04, math.pi - 0.03, math.pi - 1e-4, math.pi - 1e-9, math.pi]
DOMINANT = [unit([1, 0.3, -0.2]), unit([0.25, 1, 0.4]), unit([-0.3, 0.2, 1])]
TIES = [unit([1, 1, 0.3]), unit([1, 0.3, 1]), unit([0.3, 1, 1]), unit([1, 1, 1])]


def ladder_cases(rng):
    """(residual rotation, translation scale, exact): exact = the partner poses carry identity rotations, so the residual
    the kernel sees IS this matrix (needed at thresholds, ties and W = 0); otherwise random partner rotations."""
    out = []
    for scale in (1.0, 100.0):
        for ang in LADDER:
            for a in [unit(rng.normal(size=3)) for _ in range(4)]:
                out.append((rot_exact(a, ang), scale, True))
            if ang in (0.5, 2.0, 1e-8):
                out.append((rot_exact(unit(rng.normal(size=3)), ang), scale, False))
        for ang in NEAR_PI:
            for a in DOMINANT + TIES:
                for sgn in (1.0, -1.0):
                    out.append((rot_exact(sgn * a, ang), scale, True))
            if ang != math.pi:
                for a in DOMINANT:
                    out.append((rot_exact(a, ang), scale, False))
    return out


def compose64(p, q):
    """p * q of two (R, t) in 50 digits, rounded to doubles."""
    Rm, t = M.pose3_compose((M.mat3(p[0]), M.vec(p[1])), (M.mat3(q[0]), M.vec(q[1])))
    return np.array([[float(x) for x in row] for row in Rm]), M.to_f64(t)


def branch_census(arr, values, what, want):
    """Which Logmap branches the residual rotations of the sweep's factors sit in, by the restatement's float64 rule."""
    seen = {}
    for f in range(arr.n_factors):
        ft, vt, st, z = M.factor_inputs(arr, values, f)
        if ft == A.F_BETWEEN and vt[0] == P3:
            res = M.pose3_between(M.pose3_of(z), M.pose3_between(M.pose3_of(st[0]), M.pose3_of(st[1])))
        elif ft == A.F_PRIOR and vt[0] in (P3, CAM):
            res = M.pose3_between(M.pose3_of(st[0][:12]), M.pose3_of(z[:12]))
        else:
            continue
        b = M.so3_logmap_branch(res[0])
        w = M.so3_logmap(res[0])
        if float(mp.sqrt(M.dot(w, w))) < 1e-10:
            b += "/t<1e-10"
        seen[b] = seen.get(b, 0) + 1
    print(f"{what}: Logmap branches {seen}")
    assert want <= set(seen), (want, seen)


ALL_BRANCHES = {"pi0", "pi1", "pi2", "normal", "taylor", "taylor/t<1e-10"}


def test_so3_ladder_in_between_pose3():
    """The residual rotation z^-1 x1^-1 x2 of BetweenFactor<Pose3> over the angle ladder: both Taylor branches and their
    switches, the |w| < 1e-10 branch of Pose3::Logmap, and near pi the three permutations, the `>` ties, both signs of W and
    W = 0, with translations of O(1) and O(100)."""
    rng = np.random.default_rng(101)
    g = Graph()
    for Rres, scale, exact in ladder_cases(rng):
        res = (Rres, scale * rng.uniform(-1, 1, 3))
        if exact:
            x1 = (EYE, scale * rng.uniform(-1, 1, 3))
            z = (EYE, scale * rng.uniform(-1, 1, 3))
        else:
            x1 = (R.random_rot3(rng, 1.5), scale * rng.uniform(-1, 1, 3))
            z = (R.random_rot3(rng, 1.5), scale * rng.uniform(-1, 1, 3))
        x2 = compose64(compose64(x1, z), res)
        a = g.var(P3, 6, R.pose3_state(*x1))
        b = g.var(P3, 6, R.pose3_state(*x2))
        g.factor(A.F_BETWEEN, [a, b], 6, R.pose3_state(*z), A.NOISE_DIAGONAL, rng.uniform(0.5, 2.0, 6))
    arr = g.arrays()
    branch_census(arr, arr.values, "BETWEEN<Pose3> ladder", ALL_BRANCHES)
    judge(arr, "BETWEEN<Pose3> ladder", n_cases=len(g.factors), per_block=False)


@pytest.mark.parametrize("vt", [P3, CAM])
def test_so3_ladder_in_priors(vt):
    """x^-1 z of PriorFactor<Pose3> and of the pose part of PriorFactor<PinholeCamera<Cal3Bundler>> over the same ladder; a
    graph of priors only, so the generic list runs in a launch of its own."""
    rng = np.random.default_rng(102 + vt)
    g = Graph()
    for Rres, scale, exact in ladder_cases(rng):
        x = (EYE if exact else R.random_rot3(rng, 1.5), scale * rng.uniform(-1, 1, 3))
        zp = compose64(x, (Rres, scale * rng.uniform(-1, 1, 3)))
        xs, zs = R.pose3_state(*x), R.pose3_state(*zp)
        if vt == CAM:
            cal = np.array([500.0, -0.1, 0.02, 3.0, 4.0])
            xs, zs = np.concatenate([xs, cal]), np.concatenate([zs, cal + [7.0, 0.05, -0.01, 0.0, 0.0]])
        v = g.var(vt, A.TANGENT_DIM[vt], xs)
        g.factor(A.F_PRIOR, [v], A.TANGENT_DIM[vt], zs, A.NOISE_ISOTROPIC, [rng.uniform(0.5, 2.0)])
    arr = g.arrays()
    name = "PRIOR<Pose3> ladder" if vt == P3 else "PRIOR<Camera> ladder"
    branch_census(arr, arr.values, name, ALL_BRANCHES)
    judge(arr, name, n_cases=len(g.factors), per_block=False)


def check_retract(arr, delta, what):
    be = backend(arr)
    be.retract(delta, commit=True, want_error=False)
    got = be.get_values()
    be.close()
    want = M.retract_values(arr, arr.values, delta)
    so = arr.state_offsets()
    worst = 0.0
    for v in range(arr.n_vars):
        gv, wv = got[so[v]:so[v + 1]], want[so[v]:so[v + 1]]
        d = float(np.max(np.abs(gv - wv)))
        worst = max(worst, d / (1e-13 * max(1.0, float(np.max(np.abs(wv))))))
        assert d <= 1e-13 * max(1.0, float(np.max(np.abs(wv)))), (what, v, gv, wv)
    print(f"{what}: {arr.n_vars} variables, worst |state - restated| = {worst:.3f} of its bound 1e-13 max(1, max |state|)")
    return got, want


def test_so3_ladder_in_retract():
    """retract_kernel on POSE3 and CAMERA: the rotation part of the step over the ladder (the w.w <= 1e-5 switch of
    Pose3::Expmap on both sides, large angles up to pi), steps in f, k1, k2 that differ from one another, u0 and v0 carried;
    and VECTOR / POSE2 variables in the same launch."""
    rng = np.random.default_rng(104)
    g = Graph()
    delta = []
    for scale in (1.0, 100.0):
        for ang in LADDER + NEAR_PI:
            for vt in (P3, CAM):
                for a in DOMINANT + TIES[:2]:
                    xs = R.pose3_state(R.random_rot3(rng, 1.5), scale * rng.uniform(-1, 1, 3))
                    d = np.concatenate([ang * a, scale * rng.uniform(-1, 1, 3)])
                    if vt == CAM:
                        xs = np.concatenate([xs, [500.0, -0.1, 0.02, 3.0, 4.0]])
                        d = np.concatenate([d, [11.0, -0.07, 0.013]])
                    g.var(vt, A.TANGENT_DIM[vt], xs)
                    delta.append(d)
    for n in (1, 2, 3, 6, 9):
        g.var(V, n, rng.uniform(-3, 3, n))
        delta.append(rng.uniform(-1, 1, n))
    g.var(P2, 3, [1.0, -2.0, 0.7])
    delta.append(np.array([0.3, 0.2, -0.4]))
    arr = g.arrays()
    assert arr.n_vars > 256 and arr.n_vars % 256 != 0
    got, _ = check_retract(arr, np.concatenate(delta), "retract ladder")
    so = arr.state_offsets()
    cams = [v for v in range(arr.n_vars) if arr.var_types[v] == CAM]
    assert all(np.array_equal(got[so[v] + 15:so[v] + 17], [3.0, 4.0]) for v in cams)


# ---- Pose2 at the wrap -------------------------------------------------------------------------------------------------
WRAP_OFFSETS = [1e-3, 1e-6, 1e-9 * math.pi]


def test_pose2_wraps_at_pi():
    """BetweenFactor<Pose2> and PriorFactor<Pose2> with states outside (-pi, pi] and residual angles within 1e-3 of +-pi on
    both sides (the error wraps through atan2), and retract steps that carry theta across +-pi."""
    rng = np.random.default_rng(105)
    g = Graph()
    raw = []
    thetas = [0.3, -2.0, 4.0, -5.5, 7.0, 3 * math.pi + 0.1, -3.0, 3.1]
    residuals = [s * (math.pi + t * o) for s in (1, -1) for t in (1, -1) for o in WRAP_OFFSETS] + [0.0, 1.0, -2.5, 3.0]
    while len(g.factors) < 300:
        for r in residuals:
            th1, thz = thetas[len(g.factors) % len(thetas)], rng.uniform(-1, 1)
            a = g.var(P2, 3, [rng.uniform(-5, 5), rng.uniform(-5, 5), th1])
            b = g.var(P2, 3, [rng.uniform(-5, 5), rng.uniform(-5, 5), th1 + thz + r])
            g.factor(A.F_BETWEEN, [a, b], 3, [rng.uniform(-1, 1), rng.uniform(-1, 1), thz], A.NOISE_DIAGONAL, rng.uniform(0.5, 2, 3))
            raw.append(r)
            v = g.var(P2, 3, [rng.uniform(-5, 5), rng.uniform(-5, 5), th1])
            g.factor(A.F_PRIOR, [v], 3, [rng.uniform(-5, 5), rng.uniform(-5, 5), th1 - r], A.NOISE_ISOTROPIC, [0.7])
            raw.append(r)
    arr = g.arrays()
    got, want, _, _ = judge(arr, "Pose2 wrap", n_cases=len(g.factors))
    wrapped = 0
    for f, r in enumerate(raw):
        W, _, _ = R.whitener(arr, f)
        e_theta = -(np.linalg.solve(W, got[f].reshape(3, -1, order="F")[:, -1]))[2]
        assert -math.pi <= e_theta <= math.pi, (f, e_theta)
        if abs(r) > math.pi:
            wrapped += 1
            assert abs(e_theta - (r - math.copysign(2 * math.pi, r))) <= 1e-12, (f, r, e_theta)
        else:
            assert abs(e_theta - r) <= 1e-12, (f, r, e_theta)
    assert wrapped >= 40
    # retract across +-pi: theta + dtheta leaves (-pi, pi] and comes back wrapped
    g2, delta = Graph(), []
    for th in thetas + [math.pi - 1e-3, -math.pi + 1e-3, 3.14159, -3.14159]:
        for dth in (1e-2, -1e-2, 2e-3, -2e-3, 3.0, -3.0, 6.5):
            g2.var(P2, 3, [rng.uniform(-5, 5), rng.uniform(-5, 5), th])
            delta.append([rng.uniform(-1, 1), rng.uniform(-1, 1), dth])
    arr2 = g2.arrays()
    got_v, want_v = check_retract(arr2, np.concatenate(delta), "Pose2 retract across +-pi")
    th_out = got_v[2::3]
    assert np.all(th_out > -math.pi - 1e-15) and np.all(th_out <= math.pi)
    raw_sum = np.array([g2.vals[i][2] + delta[i][2] for i in range(arr2.n_vars)])
    assert np.sum(np.abs(raw_sum) > math.pi) >= 20
    assert np.max(np.abs(np.angle(np.exp(1j * (th_out - raw_sum))))) <= 1e-13 * 4


# ---- cameras -----------------------------------------------------------------------------------------------------------
def camera_pose(rng):
    return R.random_rot3(rng, 1.2), rng.uniform(-5, 5, 3)


def test_sfm_distortion_depth_and_cheirality():
    """GSX_F_SFM: k1, k2 of both signs with r = u^2 + v^2 of O(1) (g moves by O(1)), camera-frame depths from 1e-6 up, a few
    points behind the camera (zeroed block, status count = restated count), as test_stereo_cheirality_on_the_device."""
    rng = np.random.default_rng(106)
    g = Graph()
    depths = [1e-6, 1e-5, 1e-3, 0.1, 1.0, 7.0, 40.0]
    behind = []
    ks = [(0.45, 0.3), (-0.4, 0.25), (0.35, -0.3), (-0.3, -0.2), (0.0, 0.0), (1.2, 0.8)]
    gmin, gmax = 1.0, 1.0
    while len(g.factors) < 330:
        k1, k2 = ks[len(g.factors) % len(ks)]
        qz = depths[(len(g.factors) // len(ks)) % len(depths)]
        if len(g.factors) % 41 == 7:
            qz = -qz
            behind.append(len(g.factors))
        Rm, t = camera_pose(rng)
        q = abs(qz) * np.array([rng.uniform(-0.9, 0.9), rng.uniform(-0.9, 0.9), 0.0]) + [0.0, 0.0, qz]
        f = rng.uniform(400, 600)
        cam = np.concatenate([R.pose3_state(Rm, t), [f, k1, k2, rng.uniform(-5, 5), rng.uniform(-5, 5)]])
        pt = t + Rm @ q
        res = M.sfm_project(cam, pt, want_H=True)
        big = 1.0 if res is None else max(float(abs(x)) for H in res[1:] for row in H for x in row)
        if res is not None:
            r2 = (q[0] / q[2]) ** 2 + (q[1] / q[2]) ** 2
            gval = 1 + (k1 + k2 * r2) * r2
            gmin, gmax = min(gmin, gval), max(gmax, gval)
        sg = min(0.5, 1.0 / big)   # a prior as stiff as the factor: the step check stays well conditioned at depth 1e-6
        a = g.var(CAM, 9, cam, sg)
        b = g.var(V, 3, pt, sg)
        z = (M.to_f64(res[0]) if res is not None else np.zeros(2)) + rng.normal(0, 30.0, 2)
        kind, params = R.noise_of(rng, ("unit", "isotropic", "diagonal", "gaussian")[len(g.factors) % 4], 2)
        g.factor(A.F_SFM, [a, b], 2, z, kind, params)
    arr = g.arrays()
    print(f"SFM sweep: distortion factor g between {gmin:.3f} and {gmax:.3f}, depths {depths}")
    assert gmax - gmin >= 1.0
    got, want, n_cheir, flags = judge(arr, "SFM distortion / depth / cheirality", n_cases=len(g.factors))
    flagged = [f for f in range(len(g.factors)) if flags[f]]
    assert set(behind) <= set(flagged) and n_cheir == len(flagged) and 0 < n_cheir < 20
    for f in flagged:
        assert not np.any(got[f])


def test_projection_with_skew():
    """GSX_F_PROJECTION: Cal3_S2 with non-zero skew of both signs and fx != fy; a few points behind the camera (zero
    Jacobians, the constant error 2 fx)."""
    rng = np.random.default_rng(107)
    g = Graph()
    behind = []
    while len(g.factors) < 300:
        Rm, t = camera_pose(rng)
        qz = rng.uniform(2.0, 9.0)
        if len(g.factors) % 53 == 5:
            qz = -qz
            behind.append(len(g.factors))
        q = np.array([rng.uniform(-0.8, 0.8) * abs(qz), rng.uniform(-0.8, 0.8) * abs(qz), qz])
        K = [rng.uniform(400, 600), rng.uniform(250, 390), rng.choice([-1, 1]) * rng.uniform(5, 80), rng.uniform(300, 340),
             rng.uniform(220, 260)]
        pose, pt = R.pose3_state(Rm, t), t + Rm @ q
        res = M.s2_project(pose, pt, K, want_H=False)
        z = (M.to_f64(res[0]) if res is not None else np.zeros(2)) + rng.normal(0, 30.0, 2)
        a, b = g.var(P3, 6, pose), g.var(V, 3, pt)
        kind, params = R.noise_of(rng, ("unit", "isotropic", "diagonal", "gaussian", "huber")[len(g.factors) % 5], 2)
        g.factor(A.F_PROJECTION, [a, b], 2, np.concatenate([z, K]), kind, params)
    arr = g.arrays()
    got, want, _, flags = judge(arr, "PROJECTION skew", n_cases=len(g.factors))
    assert [f for f in range(len(g.factors)) if flags[f]] == behind
    for f in behind:
        assert not np.any(got[f][:18]) and np.any(got[f][18:])


def test_bearing_range_guards():
    """GSX_F_BEARINGRANGE with the point at a distance n on both sides of the 1e-5 guard of Rot2::relativeBearing (bearing 0
    and a zero derivative below it), well away from it, and at the r <= 1e-10 guard of norm2 (the range's row of ones)."""
    rng = np.random.default_rng(108)
    g = Graph()
    ns = [0.0, 5e-11, 1e-6, 1e-5 * (1 - 1e-9), 1e-5 * (1 + 1e-9), 3e-5, 1e-3, 1.0, 25.0]
    below = 0
    while len(g.factors) < 300:
        n = ns[len(g.factors) % len(ns)]
        pose = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-math.pi, math.pi)])
        phi = rng.uniform(-math.pi, math.pi)
        pt = pose[:2] + n * np.array([math.cos(phi), math.sin(phi)])
        a, b = g.var(P2, 3, pose), g.var(V, 2, pt)
        kind, params = R.noise_of(rng, ("unit", "isotropic", "diagonal", "gaussian")[len(g.factors) % 4], 2)
        f = g.factor(A.F_BEARINGRANGE, [a, b], 2, [rng.uniform(-1, 1), n + rng.uniform(-0.5, 0.5)], kind, params)
        below += n < 1e-5
    arr = g.arrays()
    got, want, _, _ = judge(arr, "BEARINGRANGE guards", n_cases=len(g.factors))
    zero_rows = sum(1 for f in range(len(g.factors))
                    if not np.any(M.evaluate(arr, arr.values, f)[1][0][0]))
    assert zero_rows == below and below >= 100


# ---- noise models and robust corners in every family -------------------------------------------------------------------
FAMILIES = ["prior_vector", "prior_pose2", "prior_pose3", "prior_camera", "between_vector", "between_pose2", "between_pose3",
            "sfm", "projection", "bearingrange", "range_pose2_point2", "range_pose2_pose2", "range_pose3_point3",
            "range_pose3_pose3", "bearing", "stereo"]
PIXELS = ("sfm", "projection", "stereo")
ROWS = {"prior_vector": 3, "prior_pose2": 3, "prior_pose3": 6, "prior_camera": 9, "between_vector": 3, "between_pose2": 3,
        "between_pose3": 6, "sfm": 2, "projection": 2, "bearingrange": 2, "stereo": 3}
EVEN_FAMILIES = {"sfm": 26, "projection": 20, "between_pose3": 78, "bearingrange": 12, "range_pose2_point2": 6,
                 "range_pose3_point3": 10, "bearing": 6, "stereo": 30}


def noise_model(rng, base, m, s):
    """(kind, parameters, W) of a base model whose sigmas are of size s: whitened = W @ unwhitened."""
    if base == "unit":
        return A.NOISE_UNIT, [], np.eye(m)
    if base == "isotropic":
        sg = s * rng.uniform(0.5, 2.0)
        return A.NOISE_ISOTROPIC, [sg], np.eye(m) / sg
    if base == "diagonal":
        sg = s * rng.uniform(0.5, 2.0, m)
        return A.NOISE_DIAGONAL, list(sg), np.diag(1.0 / sg)
    if base == "gaussian":   # a full upper triangle
        U = (np.triu(rng.uniform(0.2, 0.5, (m, m)) * rng.choice([-1, 1], (m, m)), 1) * min(1.0, 2.0 / m) + np.diag(rng.uniform(0.8, 1.6, m))) / s
        return A.NOISE_GAUSSIAN, list(U.reshape(-1)), U
    sg = s * rng.uniform(0.5, 2.0, m)   # constrained, no zero sigma: the weights mu are carried and not used
    return A.NOISE_CONSTRAINED, list(sg) + list(rng.uniform(10, 1000, m)), np.diag(1.0 / sg)


def pose2_state(rng):
    return np.array([rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-3, 3)])


def pose3_state(rng):
    return R.pose3_state(R.random_rot3(rng, 1.2), rng.uniform(-5, 5, 3))


def in_front(rng, pose):
    Rm, t = R.pose3_of(pose)
    qz = rng.uniform(3.0, 8.0)
    return t + Rm @ np.array([rng.uniform(-0.6, 0.6) * qz, rng.uniform(-0.6, 0.6) * qz, qz])


def add_case(g, rng, fam, base, loss=None, level=None):
    """One factor of `fam` on fresh variables, noise `base` (+ robust `loss`), whose whitened residual has norm level * k
    (or a random O(1) norm without a loss): the residual xi = W^-1 (norm * u) is put into the measurement EXACTLY
    (z = h(x) (-) xi in the chart the factor's error uses).  Returns (factor index, k)."""
    m = ROWS.get(fam, 1)
    # sigmas of the size of the residual wanted: the residual must be many ulps of the prediction it is the difference to,
    # because a robust weight hands ulp(h) / |b| on to every entry of the block (pixels: h of O(500); ranges: h of O(10))
    s = 300.0 if fam in PIXELS else (1.0 if fam.startswith("range_") else 0.1)
    kind, params, W = noise_model(rng, base, m, s)
    k = (1.5 * s if base == "unit" else 1.5) * rng.uniform(0.8, 1.2)
    norm = level * k if loss else (s if base == "unit" else 1.0) * rng.uniform(0.3, 2.0)
    u = rng.normal(size=m)
    xi = np.linalg.solve(W, norm * u / np.linalg.norm(u))
    if loss:
        kind, params = kind | LOSSES[loss], list(params) + [k]
    if fam.startswith("prior_"):
        vt = {"prior_vector": V, "prior_pose2": P2, "prior_pose3": P3, "prior_camera": CAM}[fam]
        x = {V: lambda: rng.uniform(-3, 3, 3), P2: lambda: pose2_state(rng), P3: lambda: pose3_state(rng),
             CAM: lambda: np.concatenate([pose3_state(rng), [500.0, -0.1, 0.02, 3.0, 4.0]])}[vt]()
        v = g.var(vt, m, x)
        return g.factor(A.F_PRIOR, [v], m, M.retract(vt, x, -xi), kind, params), k      # e = -Local(x, z) = xi
    if fam == "between_vector":
        x1, x2 = rng.uniform(-3, 3, 3), rng.uniform(-3, 3, 3)
        return g.factor(A.F_BETWEEN, [g.var(V, 3, x1), g.var(V, 3, x2)], 3, (x2 - x1) - xi, kind, params), k
    if fam == "between_pose2":
        x1, x2 = pose2_state(rng), pose2_state(rng)
        h = M.pose2_compose_cs(M.pose2_inverse_cs(M.pose2_cs(M.vec(x1))), M.pose2_cs(M.vec(x2)))
        z = M.to_f64(M.pose2_chart(M.pose2_compose_cs(h, M.pose2_inverse_cs(M.pose2_cs(M.vec(xi))))))   # z^-1 h = (xi)
        return g.factor(A.F_BETWEEN, [g.var(P2, 3, x1), g.var(P2, 3, x2)], 3, z, kind, params), k
    if fam == "between_pose3":
        x1, x2 = pose3_state(rng), pose3_state(rng)
        h = M.pose3_state(M.pose3_between(M.pose3_of(x1), M.pose3_of(x2)))
        z = M.retract(P3, h, -xi)                                                      # z^-1 h = Expmap(xi)
        return g.factor(A.F_BETWEEN, [g.var(P3, 6, x1), g.var(P3, 6, x2)], 6, z, kind, params), k
    if fam in ("sfm", "projection", "stereo"):
        pose = pose3_state(rng)
        pt = in_front(rng, pose)
        if fam == "sfm":
            x = np.concatenate([pose, [rng.uniform(400, 600), -0.15, 0.05, 3.0, 4.0]])
            ft, vs, tail = A.F_SFM, [g.var(CAM, 9, x), g.var(V, 3, pt)], []
        elif fam == "projection":
            x, tail = pose, [520.0, 470.0, 12.0, 320.0, 240.0]
            ft, vs = A.F_PROJECTION, [g.var(P3, 6, x), g.var(V, 3, pt)]
        else:
            x, tail = pose, list(R.STEREO_K)
            ft, vs = A.F_STEREO, [g.var(P3, 6, x), g.var(V, 3, pt)]
        vts = [CAM if fam == "sfm" else P3, V]
        h, _, cheir = M.evaluate_mp(ft, vts, [x, pt], [0.0] * m + tail, want_H=False)
        assert not cheir
        return g.factor(ft, vs, m, np.concatenate([M.to_f64(h) - xi, tail]), kind, params), k
    if fam in ("bearingrange", "bearing", "range_pose2_point2", "range_pose2_pose2"):
        x = pose2_state(rng)
        other_pose = fam == "range_pose2_pose2"
        reach = rng.uniform(2, 9) if fam.startswith("range_") else rng.uniform(0.5, 1.0)   # (bearing-range: a range of O(sigma))
        y = pose2_state(rng) if other_pose else x[:2] + reach * np.array([math.cos(x[2] + 0.8), math.sin(x[2] + 0.8)])
        ft = {"bearingrange": A.F_BEARINGRANGE, "bearing": A.F_BEARING}.get(fam, A.F_RANGE)
        vs = [g.var(P2, 3, x), g.var(P2, 3, y) if other_pose else g.var(V, 2, y)]
        h, _, _ = M.evaluate_mp(ft, [P2, P2 if other_pose else V], [x, y], [0.0] * m, want_H=False)
        return g.factor(ft, vs, m, M.to_f64(h) - xi, kind, params), k
    x = pose3_state(rng)
    other_pose = fam == "range_pose3_pose3"
    y = pose3_state(rng) if other_pose else rng.uniform(-8, 8, 3)
    vs = [g.var(P3, 6, x), g.var(P3, 6, y) if other_pose else g.var(V, 3, y)]
    h, _, _ = M.evaluate_mp(A.F_RANGE, [P3, P3 if other_pose else V], [x, y], [0.0], want_H=False)
    return g.factor(A.F_RANGE, vs, 1, M.to_f64(h) - xi, kind, params), k


BASES = ("unit", "isotropic", "diagonal", "gaussian", "constrained")
LEVELS = (0.5, 1 - 1e-9, 1 + 1e-9, 3.0)


def corner_cases():
    """(family, base, loss, level): every base model alone, and every one a robust loss may wrap under Huber, Tukey and
    Cauchy at 0.5 k, k (1 - 1e-9), k (1 + 1e-9) and 3 k.  gsx_create refuses a robust loss on GSX_NOISE_CONSTRAINED (its
    parameter list has no place for k: include/gsx.h), which test_robust_on_constrained_is_refused pins."""
    out = []
    for fam in FAMILIES:
        for base in BASES:
            out.append((fam, base, None, None))
            if base != "constrained":
                out += [(fam, base, loss, level) for loss in LOSSES for level in LEVELS]
    return out


def whitened_norm(arr, f):
    e, _, _ = M.evaluate(arr, arr.values, f)
    W, _, _ = R.whitener(arr, f)
    return float(np.linalg.norm(W @ e))


def test_noise_models_and_robust_corners_in_every_family():
    rng = np.random.default_rng(109)
    g, meta = Graph(), []
    for fam, base, loss, level in corner_cases():
        f, k = add_case(g, rng, fam, base, loss, level)
        meta.append((fam, base, loss, level, k))
    arr = g.arrays()
    assert len(meta) == 16 * 53
    for f, (fam, base, loss, level, k) in enumerate(meta):
        if loss:   # the residual sits where it was put: within 1e-11 of level * k, i.e. on its side of k
            assert abs(whitened_norm(arr, f) / (level * k) - 1.0) <= 1e-11, (f, fam, base, loss, level)
    # Tukey just inside k: the weight 1 - d^2 / k^2 = 2e-9 is a cancelled difference that carries the rounding of d = |b|,
    # 2 ulp(h) / |b| = 2e-14 absolute, onto entries that are up to 1e2 before the weight and 1e-7 after it: 1e-12 on a block
    # whose own bound would be 1e-13 (1.3e-13 / 1.6e-13 seen, BETWEEN<Pose3> and RANGE).  Those 64 blocks are held to the
    # graph-wide rule only; float64 cannot do better whoever evaluates the weight.
    inside = {f for f, mt in enumerate(meta) if mt[2] == "tukey" and mt[3] == 1 - 1e-9}
    got, want, n_cheir, flags = judge(arr, "noise models x robust corners, all families", n_cases=len(meta), graph_wide_only=inside)
    assert n_cheir == 0 and not any(flags)
    dead = [f for f, mt in enumerate(meta) if mt[2] == "tukey" and mt[3] > 1]
    assert len(dead) == 16 * 4 * 2
    for f in dead:
        assert not np.any(got[f]), (f, meta[f])
    alive = [f for f, mt in enumerate(meta) if mt[2] == "tukey" and mt[3] == 1 - 1e-9]
    assert all(np.any(got[f]) for f in alive)


def test_tukey_beyond_k_is_exactly_zero_and_costs_k_squared_over_six():
    """A graph of nothing but Tukey factors beyond k, every family and base model: all of [A b] is exactly zero and the graph
    error is the sum of the constants k^2 / 6."""
    rng = np.random.default_rng(110)
    g, ks = Graph(), []
    for rep in range(2):
        for fam in FAMILIES:
            for base in BASES[:4]:
                for level in (1 + 1e-9, 3.0):
                    _, k = add_case(g, rng, fam, base, "tukey", level)
                    ks.append(k)
    arr = g.arrays(priors=False)
    assert arr.n_factors == 256 and len(ks) == 256   # a full last block on purpose here: the other sweeps leave it ragged
    be = backend(arr)
    be.linearize()
    got = be.jacobians()
    eg, ew = be.error(), math.fsum(k * k / 6.0 for k in ks)
    be.close()
    print(f"Tukey beyond k: {arr.n_factors} factors, nonzeros in [A b]: {int(np.count_nonzero(got))}, error {eg:.15g} vs sum k^2/6 "
          f"{ew:.15g} (no step check: rank deficient by construction, every block is zero)")
    assert not np.any(got)
    assert abs(eg - ew) <= 1e-13 * ew


def test_robust_on_constrained_is_refused():
    g = Graph()
    v = g.var(V, 2, [0.0, 1.0])
    g.factor(A.F_PRIOR, [v], 2, [0.5, 0.5], A.NOISE_CONSTRAINED | A.NOISE_ROBUST_HUBER, [1.0, 1.0, 10.0, 10.0, 1.3])
    with pytest.raises(A.GsxError) as ei:
        _lib.ProductBackend(g.arrays(priors=False))
    assert ei.value.status == A.GSX_E_INVALID


# ---- the two store paths of whiten_store -------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", sorted(EVEN_FAMILIES))
def test_both_store_paths(fam):
    """whiten_store takes 16-byte stores only when M * NC is even and the block's offset is 16-byte aligned.  Two copies of
    one sweep of an even-sized family: behind an odd-sized block (a POSE2-POSE2 range factor, 1 x 7) every offset is odd,
    with nothing in front every offset is even.  Both copies against the restatement, and bit-identical to each other."""
    size = EVEN_FAMILIES[fam]
    copies = {}
    for lead in (True, False):
        rng = np.random.default_rng(111)
        g = Graph()
        if lead:
            a, b = g.var(P2, 3, [0.0, 0.0, 0.1]), g.var(P2, 3, [3.0, 4.0, -0.2])
            g.factor(A.F_RANGE, [a, b], 1, [4.5], A.NOISE_ISOTROPIC, [0.3])
        bases = BASES[:4]
        for i in range(301):
            loss = (None, "huber", "cauchy", "tukey")[i % 4]
            add_case(g, rng, fam, bases[(i // 4) % 4], loss, rng.uniform(0.3, 2.5) if loss else None)
        arr = g.arrays()
        off = arr.jacobian_offsets()
        first = 1 if lead else 0
        assert np.all(np.diff(off)[first:first + 301] == size)
        parity = set(int(o) % 2 for o in off[first:first + 301])
        copies[lead] = (arr, parity, first)
    assert copies[True][1] == {1} and copies[False][1] == {0}, (copies[True][1], copies[False][1])
    print(f"{fam}: M*NC = {size}; offsets behind the 1x7 block all odd (scalar stores), without it all even (16-byte stores)")
    got = {}
    for lead in (True, False):
        arr, _, first = copies[lead]
        blk, _, _, _ = judge(arr, f"{fam} store path, offsets {'odd' if lead else 'even'}", n_cases=301 + first)
        got[lead] = blk[first:first + 301]
    for f in range(301):
        assert np.array_equal(got[True][f], got[False][f]), (fam, f)


# ---- generic factors riding in another family's launch -----------------------------------------------------------------
def add_generic(g, rng, count, anchor):
    """`count` generic factors: first a prior on each variable of `anchor` (the main families' variables, so that the graph
    is regular once they are all covered), then priors of every variable type and vector-betweens of dimension 1, 2, 3, 6, 9
    (each behind the priors of its two variables) on fresh variables.  Returns whether every anchor got its prior."""
    n = 0
    for v in anchor:
        if n == count:
            return False
        _, vt, dim = g.vars[v]
        g.factor(A.F_PRIOR, [v], dim, g.vals[v], A.NOISE_ISOTROPIC, [0.4])
        n += 1
    unit_i = 0
    while n < count:
        kind_i = unit_i % 8
        unit_i += 1
        if kind_i < 5:
            d = (1, 2, 3, 6, 9)[kind_i]
            x1, x2 = rng.uniform(-3, 3, d), rng.uniform(-3, 3, d)
            a = g.var(V, d, x1)
            g.factor(A.F_PRIOR, [a], d, x1 + rng.normal(0, 0.1, d), *noise_model(rng, BASES[unit_i % 4], d, 0.3)[:2])
            n += 1
            if n == count:
                break
            b = g.var(V, d, x2)
            g.factor(A.F_PRIOR, [b], d, x2 + rng.normal(0, 0.1, d), A.NOISE_ISOTROPIC, [0.5])
            n += 1
            if n == count:
                break
            g.factor(A.F_BETWEEN, [a, b], d, (x2 - x1) + rng.normal(0, 0.1, d), *noise_model(rng, BASES[(unit_i + 1) % 4], d, 0.3)[:2])
            n += 1
        else:
            vt = (P2, P3, CAM)[kind_i - 5]
            x = {P2: lambda: pose2_state(rng), P3: lambda: pose3_state(rng),
                 CAM: lambda: np.concatenate([pose3_state(rng), [500.0, -0.1, 0.02, 3.0, 4.0]])}[vt]()
            dim = A.TANGENT_DIM[vt]
            v = g.var(vt, dim, x)
            g.factor(A.F_PRIOR, [v], dim, M.retract(vt, x, rng.normal(0, 0.05, dim)), A.NOISE_DIAGONAL, list(rng.uniform(0.3, 1.0, dim)))
            n += 1
    return True


MAINS = {"none": [], "sfm": ["sfm"], "between_pose2": ["between_pose2"], "between_pose3": ["between_pose3"],
         "projection": ["projection"],
         "all": ["sfm", "between_pose2", "between_pose3", "projection", "bearingrange", "range_pose2_point2", "range_pose2_pose2",
                 "range_pose3_point3", "range_pose3_pose3", "bearing", "stereo"]}


@pytest.mark.parametrize("count", [0, 1, 255, 256, 257, 600])
@pytest.mark.parametrize("main", sorted(MAINS))
def test_generic_factors_riding_in_another_launch(main, count):
    """Priors and vector-betweens are linearized in the first (gn + 255) >> 8 blocks of the first of the SFM / BETWEEN<Pose2>
    / BETWEEN<Pose3> launches present, or in a launch of their own: gn on both sides of 256, with no other family, with one
    (a carrier, or PROJECTION which carries nothing) and with all.  (0 generic factors and no other family is the empty
    graph: nothing to run.)"""
    if main == "none" and count == 0:
        return
    rng = np.random.default_rng(112 + count)
    g = Graph()
    n_main = 125 if len(MAINS[main]) == 1 else 11   # at most 250 variables: 255 generic priors cover them all
    for fam in MAINS[main]:
        for i in range(n_main):
            add_case(g, rng, fam, BASES[i % 4])
    anchor = list(range(len(g.vars)))
    covered = add_generic(g, rng, count, anchor)
    arr = g.arrays(priors=False)
    n_generic = int(np.sum((arr.f_type == A.F_PRIOR) | ((arr.f_type == A.F_BETWEEN) & (arr.var_types[arr.f_vars[arr.f_key_ptr[:-1]]] == V))))
    assert n_generic == count
    what = f"riders: {count} generic factors, main families: {main}"
    judge(arr, what, ragged=False, solve=covered,
          no_solve_reason=None if covered else "rank deficient by construction: fewer generic priors than main-family variables")
