"""The absolute-measurement factors and the Rot3 variable of tests/_absolute_restatement.py at the 50 digits of
tests/_mp_restatement.py, from the same reference lines.  Branches (CalculateBestAxis, the Logmap branches, the Rot2
renormalisation) are decided on the float64 values, as the device and the reference decide them."""
import functools

import mpmath as mp
import numpy as np

from gtsam_petercdev_amd import _abi as A
from tests import _absolute_restatement as S
from tests import _factor_restatement as R
from tests import _mp_restatement as M

ROT3 = S.ROT3


def rows3(s):
    s = M.vec(s)
    return [s[0:3], s[3:6], s[6:9]]


def hstack(*Ms):
    return [sum((list(Mx[i]) for Mx in Ms), []) for i in range(len(Ms[0]))]


def normalize(v):
    n = mp.sqrt(M.dot(v, v))
    return [x / n for x in v]


def unit3_basis(n):
    """3 x 2, the axis chosen on the float64 direction."""
    axis = [mp.mpf(0)] * 3
    axis[S.best_axis([float(x) for x in n])] = mp.mpf(1)
    b1 = normalize(M.cross(n, axis))
    b2 = M.cross(n, b1)
    return [[b1[i], b2[i]] for i in range(3)]


def tr(Mx):
    return [[Mx[j][i] for j in range(len(Mx))] for i in range(len(Mx[0]))]


def attitude(Rm, n_ref, b):
    q = normalize(M.mv(Rm, b))
    B, Bq = unit3_basis(n_ref), unit3_basis(q)
    HR = M.neg(M.mm(tr(Bq), M.mm(Rm, M.skew(b))))
    return M.mv(tr(B), q), M.mm(M.mm(tr(B), Bq), HR)


def evaluate_mp(ftype, vt, st, z, want_H=True):
    st, z = [M.vec(s) for s in st], M.vec(z)
    Z3 = M.zeros(3, 3)
    if ftype == S.F_GPS:
        Rm, t = rows3(st[0][:9]), st[0][9:12]
        if len(st) == 2 or len(z) == 6:
            bL = st[1] if len(st) == 2 else z[3:6]
            e = M.sub(M.add(t, M.mv(Rm, bL)), z[:3])
            H1 = hstack(M.neg(M.mm(Rm, M.skew(bL))), Rm)
            return e, [H1, Rm] if len(st) == 2 else [H1], False
        return M.sub(t, z), [hstack(Z3, Rm)], False
    if ftype == S.F_TRANS:
        if vt[0] == A.VAR_POSE2:
            c, s = mp.cos(st[0][2]), mp.sin(st[0][2])
            return M.sub(st[0][:2], z), [[[c, -s, mp.mpf(0)], [s, c, mp.mpf(0)]]], False
        return M.sub(st[0][9:12], z), [hstack(Z3, rows3(st[0][:9]))], False
    if ftype == S.F_ROT:
        if vt[0] == A.VAR_POSE2:
            zero = mp.mpf(0)
            e = M.pose2_between([zero, zero, z[0]], [zero, zero, st[0][2]])[2]
            return [e], [[[zero, zero, mp.mpf(1)]]], False
        return M.so3_logmap(M.mm(M.tr3(rows3(z)), rows3(st[0][:9]))), [hstack(M.identity(3), Z3)], False
    if ftype == S.F_ATT:
        e, H = attitude(rows3(st[0][:9]), z[:3], z[3:6])
        return e, [H if vt[0] == ROT3 else hstack(H, M.zeros(2, 3))], False
    if ftype == S.F_MAG:
        if vt[0] == A.VAR_POSE2:
            c, s = mp.cos(st[0][2]), mp.sin(st[0][2])
            q = [c * z[2] + s * z[3], -s * z[2] + c * z[3]]
            zero = mp.mpf(0)
            return M.sub(M.add(q, z[4:6]), z[:2]), [[[zero, zero, q[1]], [zero, zero, -q[0]]]], False
        q = M.mv(M.tr3(rows3(st[0][:9])), z[3:6])
        H = M.skew(q)
        return M.sub(M.add(q, z[6:9]), z[:3]), [H if vt[0] == ROT3 else hstack(H, Z3)], False
    if vt[0] == ROT3 and ftype == A.F_PRIOR:
        return [-x for x in M.so3_logmap(M.mm(M.tr3(rows3(st[0])), rows3(z)))], [M.identity(3)], False
    if vt[0] == ROT3 and ftype == A.F_BETWEEN:
        h = M.mm(M.tr3(rows3(st[0])), rows3(st[1]))
        return M.so3_logmap(M.mm(M.tr3(rows3(z)), h)), [M.neg(M.tr3(h)), M.identity(3)], False
    return M.evaluate_mp(ftype, vt, st, z, want_H)


def retract_mp(vtype, state, d):
    if vtype == ROT3:
        Y = M.mm(rows3(state), M.so3_expmap(M.vec(d)))
        return Y[0] + Y[1] + Y[2]
    return M.retract_mp(vtype, state, d)


def retract(vtype, state, d):
    return M.to_f64(retract_mp(vtype, state, d))


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
    """Central differences of the 50-digit error in the variables' tangent spaces (tests/_mp_restatement.true_jacobians
    with this module's charts): one m x d float64 matrix per key."""
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
