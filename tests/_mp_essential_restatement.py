"""The Unit3 and EssentialMatrix variables and the epipolar factors of tests/_essential_restatement.py at the 50 digits
of tests/_mp_restatement.py, from the same reference lines.  Branches (CalculateBestAxis, the epsilon branches of the
Unit3 charts, the Logmap branches) are decided on the float64 values, as the device and the reference decide them."""
import functools

import mpmath as mp
import numpy as np

from gtsam_petercdev_amd import _abi as A
from tests import _essential_restatement as S
from tests import _factor_restatement as R
from tests import _mp_absolute_restatement as MA
from tests import _mp_restatement as M

UNIT3, ESSENTIAL = S.UNIT3, S.ESSENTIAL
EPS = float(np.finfo(float).eps)
rows3, tr, hstack, normalize, unit3_basis = MA.rows3, MA.tr, MA.hstack, MA.normalize, MA.unit3_basis


def unit3_retract(p, v):
    xi = M.mv(unit3_basis(p), v)
    theta = mp.sqrt(M.dot(xi, xi))
    st = mp.mpf(1) if float(theta) < EPS else mp.sin(theta) / theta
    return normalize(M.add(M.scal(mp.cos(theta), p), M.scal(st, xi)))


def unit3_local(p, q):
    x = M.dot(p, q)
    z = 1 - x * x
    x64 = S.dot64(p, q)                      # the branch is decided on the float64 dot product, as the device decides it
    if 1.0 - x64 * x64 < EPS:
        if x64 <= 0:
            return [mp.pi, mp.mpf(0)]
        y = 1 - (x - 1) / 3
    else:
        y = mp.acos(x) / mp.sqrt(z)
    return M.mv(tr(unit3_basis(p)), M.scal(y, M.sub(q, M.scal(x, p))))


def e_of(s):
    return rows3(s[:9]), s[9:12]


def vm(v, Mx):
    return M.mv(tr(Mx), v)


def epipolar(Rm, t, vA, vB):
    E = M.mm(M.skew(t), Rm)
    HR = vm(vA, M.mm(E, M.skew(M.scal(-1, vB))))
    HD = vm(vA, M.mm(M.skew(M.scal(-1, M.mv(Rm, vB))), unit3_basis(t)))
    return M.dot(vA, M.mv(E, vB)), [HR + HD]


def calibrate(K, p):
    fx, fy, s, u0, v0 = K
    du, dv = p[0] - u0, p[1] - v0
    ydv = dv / fy
    pt = [(du - s * ydv) / fx, ydv]
    z = mp.mpf(0)
    return pt, [[-pt[0] / fx, s * ydv / (fx * fy), -pt[1] / fx, -1 / fx, s / (fx * fy)], [z, -pt[1] / fy, z, z, -1 / fy]]


def depth(Rm, t, d, z):
    dP1, pn, f = z[:3], z[3:5], z[5]
    Rt = M.tr3(Rm)
    dP2 = M.mv(Rt, M.sub(dP1, M.scal(d, t)))
    u, v = dP2[0] / dP2[2], dP2[1] / dP2[2]
    fz = f / dP2[2]
    fDpn = [[fz, mp.mpf(0), -fz * u], [mp.mpf(0), fz, -fz * v]]
    DdP2_E = hstack(M.skew(dP2), M.neg(M.mm(Rt, [[d * b for b in row] for row in unit3_basis(t)])))
    Dd = M.mv(fDpn, M.mv(Rt, t))
    return [f * (u - pn[0]), f * (v - pn[1])], M.mm(fDpn, DdP2_E), [[-Dd[0]], [-Dd[1]]]


def evaluate_mp(ftype, vt, st, z, want_H=True):
    st, z = [M.vec(s) for s in st], M.vec(z)
    one = mp.mpf(1)
    if ftype == S.F_E:
        e, H = epipolar(*e_of(st[0]), z[:3], z[3:6])
        return [e], [H], False
    if ftype == S.F_E_CALIB:
        Rm, t = e_of(st[0])
        (cA, DA), (cB, DB) = calibrate(st[1], z[:2]), calibrate(st[1], z[2:4])
        vA, vB = cA + [one], cB + [one]
        E = M.mm(M.skew(t), Rm)
        e, HE = epipolar(Rm, t, vA, vB)
        gA, gB = M.mv(E, vB)[:2], vm(vA, E)[:2]
        HK = M.add(vm(gA, DA), vm(gB, DB))
        return [e], [HE, [HK]], False
    if ftype == S.F_E_DEPTH:
        Rm, t = e_of(st[0])
        d = st[1][0]
        if len(z) == 6:
            e, DE, Dd = depth(Rm, t, d, z)
            return e, [DE, Dd], False
        C = rows3(z[6:15])
        q = normalize(M.mv(C, t))
        Hp = M.mm(tr(unit3_basis(q)), M.mm(C, unit3_basis(t)))
        zero = mp.mpf(0)
        HE = [list(C[i]) + [zero, zero] for i in range(3)] + [[zero] * 3 + list(Hp[i]) for i in range(2)]
        e, DE, Dd = depth(M.mm(M.mm(C, Rm), M.tr3(C)), q, d, z)
        return e, [M.mm(DE, HE), Dd], False
    if ftype == S.F_E_CONSTRAINT:
        h = M.pose3_between(M.pose3_of(st[0]), M.pose3_of(st[1]))
        Rh, th = h
        n2 = M.dot(th, th)
        n = mp.sqrt(n2)
        dirn = [x / n for x in th]
        Dn = [[((n2 if i == j else 0) - th[i] * th[j]) / (n2 * n) for j in range(3)] for i in range(3)]
        G = M.mm(tr(unit3_basis(dirn)), M.mm(Dn, Rh))
        zero = mp.mpf(0)
        D = [[one if i == j else zero for j in range(6)] for i in range(3)] + [[zero] * 3 + list(G[i]) for i in range(2)]
        Rz, tz = e_of(z)
        e = M.so3_logmap(M.mm(M.tr3(Rz), Rh)) + unit3_local(tz, dirn)
        return e, [M.neg(M.mm(D, M.pose3_adjoint(M.pose3_inverse(h)))), D], False
    if ftype == A.F_PRIOR and vt[0] == UNIT3:
        return [-x for x in unit3_local(st[0], z)], [M.identity(2)], False
    if ftype == A.F_PRIOR and vt[0] == ESSENTIAL:
        return [-x for x in local_mp(ESSENTIAL, st[0], z)], [M.identity(5)], False
    return MA.evaluate_mp(ftype, vt, st, z, want_H)


def retract_mp(vtype, state, d):
    if vtype == UNIT3:
        return unit3_retract(M.vec(state), M.vec(d))
    if vtype == ESSENTIAL:
        state, d = M.vec(state), M.vec(d)
        Y = M.mm(rows3(state[:9]), M.so3_expmap(d[:3]))
        return Y[0] + Y[1] + Y[2] + unit3_retract(state[9:12], d[3:5])
    return MA.retract_mp(vtype, state, d)


def local_mp(vtype, x, y):
    x, y = M.vec(x), M.vec(y)
    if vtype == UNIT3:
        return unit3_local(x, y)
    (Rx, tx), (Ry, ty) = e_of(x), e_of(y)
    return M.so3_logmap(M.mm(M.tr3(Rx), Ry)) + unit3_local(tx, ty)


def retract(vtype, state, d):
    return M.to_f64(retract_mp(vtype, state, d))


def local(vtype, x, y):
    return M.to_f64(local_mp(vtype, x, y))


def retract_values(arr, values, delta):
    so, to = arr.state_offsets(), arr.tangent_offsets()
    out = values.copy()
    for v in range(arr.n_vars):
        out[so[v]:so[v + 1]] = retract(int(arr.var_types[v]), values[so[v]:so[v + 1]], delta[to[v]:to[v + 1]])
    return out


def evaluate(arr, values, f):
    e, Hs, cheir = evaluate_mp(*M.factor_inputs(arr, values, f))
    return M.to_f64(e), [np.array([[float(x) for x in row] for row in H], dtype=float) for H in Hs], cheir


def true_jacobians(arr, values, f, step="1e-20"):
    """Central differences of the 50-digit error in the variables' tangent spaces: one m x d float64 matrix per key."""
    ftype, vt, st, z = M.factor_inputs(arr, values, f)
    h = mp.mpf(step)
    out = []
    for k, v in enumerate(R.factor_parts(arr, f)[1]):
        d = int(arr.var_dims[v])
        cols = []
        for j in range(d):
            es = []
            for sgn in (1, -1):
                dx = [mp.mpf(0)] * d
                dx[j] = sgn * h
                moved = list(st)
                moved[k] = retract_mp(vt[k], st[k], dx)
                es.append(evaluate_mp(ftype, vt, moved, z, want_H=False)[0])
            cols.append([(a - b) / (2 * h) for a, b in zip(*es)])
        out.append(np.array([[float(cols[j][i]) for j in range(d)] for i in range(len(cols[0]))], dtype=float))
    return out


linearized = functools.partial(R.linearized, evaluate=evaluate)
jacobians = functools.partial(R.jacobians, evaluate=evaluate)
factor_error = functools.partial(R.factor_error, evaluate=evaluate)
graph_error = functools.partial(R.graph_error, evaluate=evaluate)
dense_system = functools.partial(R.dense_system, evaluate=evaluate)
