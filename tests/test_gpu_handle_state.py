"""The handle's state machine, pinned: which entry points answer and what they answer after every event that changes
the values, the [A b] blocks, the tree or the resident factorization.

Every (event, reader) pair starts from a handle of its own that has linearized and solved at lambda = 0.  The table
below holds what the reader answers after the event:

  ok     GSX_OK, and the output is bit for bit that of a FRESH handle brought to the same graph, values and ordering by the
         plain route (set_values, set_ordering, linearize, solve at lambda = 0)
  old    GSX_OK, and the output is bit for bit what the handle held BEFORE the event: gsx_get_conditional tests only that a
         successful factorization is resident, not that it belongs to the current values, so after an event that moves the
         values without touching the arena it serves the factorization of the previous linearization
  trial  GSX_OK, and the output is bit for bit that of a fresh handle that took the same damped step (linearize, solve at
         the trial's lambda): the step and the factorization of a trial that was not taken stay readable
  state  GSX_E_STATE
  indet  GSX_E_INDETERMINATE

The table was derived from the flag writes of the entry points in csrc/ and describes what the library does, not what
it should do.  Two departures from a literal "apply the event, call the reader": (1) the rejected trial is gsx_lm_trial
(the trial without the policy, which never takes it) with a lambda of 1e-6 on a handle prepared at values far from the
optimum, where the nearly undamped step overshoots: the event asserts that the trial error rose; (2) the
failing factorization needs a gauge-free graph, on which no lambda = 0 solve succeeds, so that event — the Gauss-Newton
run of test_failed_factorization_is_not_reused — has a graph and a test of its own, and no preparation.  The graphs of
the parity suite carry no GSX_F_LINEAR factor: one unary linear factor is appended to each graph here so that
gsx_set_block_jacobians has a block to rewrite.
"""
import numpy as np
import pytest

import gtsam_petercdev_amd as gt
from gtsam_petercdev_amd import _abi as A
from gtsam_petercdev_amd.graph import Pose2, Values, NonlinearFactorGraph, PriorFactor, BetweenFactor, noiseModel

from tests.test_gpu_parity import PROBLEMS

pytestmark = pytest.mark.gpu

LAM_TRIAL = 1e-6


@pytest.fixture(scope="module")
def gpu():
    from gtsam_petercdev_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the HIP path has no fallback"
    return _lib


def _chain(prior):
    fg = NonlinearFactorGraph()
    if prior:
        fg.add(PriorFactor(0, Pose2(0, 0, 0), noiseModel.Isotropic.Sigma(3, 0.1)))
    for i in range(5):
        fg.add(BetweenFactor(i, i + 1, Pose2(1, 0, 0.1), noiseModel.Isotropic.Sigma(3, 0.1)))
    v = Values()
    for i in range(6):
        v.insert(i, Pose2(1.0 * i + 0.05 * i, 0.02 * i, 0.1 * i))
    return fg.to_arrays(v)


def _linear_block(d, seed):
    """[A b] of a unary linear factor on a variable of dimension d: d rows, column-major."""
    rng = np.random.default_rng(seed)
    return np.concatenate([np.eye(d) * 0.5 + 0.05 * rng.normal(size=(d, d)), 0.01 * rng.normal(size=(d, 1))], axis=1)


def _with_linear(arr, var, seed):
    d = int(arr.var_dims[var])
    return arr.with_factor(A.F_LINEAR, [var], d, _linear_block(d, seed).reshape(-1, order="F"), A.NOISE_UNIT)


class Graph:
    def __init__(self, gpu, arr, pcg, kinds, far):
        self.pcg = pcg
        n = arr.n_vars
        self.arr = _with_linear(arr, n - 1, 1)               # the graph of the handle
        self.f_lin = self.arr.n_factors - 1
        self.block2 = _linear_block(int(arr.var_dims[n - 1]), 2)
        self.arr_block2 = _with_linear(arr, n - 1, 2)        # ... after gsx_set_block_jacobians(block2)
        self.arr_grown = _with_linear(self.arr, n - 2, 3)    # ... after gsx_update added one factor
        be = gpu.product_backend(self.arr)
        self.ord0 = be.compute_ordering(kinds[0]) if kinds else np.array(self.arr.var_keys)
        self.ord1 = be.compute_ordering(kinds[1]) if kinds else np.array(self.arr.var_keys[::-1])
        self.x0 = self.arr.values.copy()
        # where a Gauss-Newton step goes: valid states to move variables to
        be.set_ordering(self.ord0)
        be.linearize()
        be.solve(0.0, False)
        be.retract(None, commit=True, want_error=False)
        self.x1 = be.get_values()
        # far from the optimum (`far` standard deviations in every tangent direction): a Gauss-Newton step overshoots there
        # (chosen on the CPU oracle: the error rises tenfold on the chain, twentyfold on pose3, by orders on bal_small)
        be.set_values(self.x0)
        be.retract(far * np.random.default_rng(4).normal(size=be.tangent_size), commit=True, want_error=False)
        self.x_far = be.get_values()
        be.close()
        off = np.concatenate([[0], np.cumsum(self.arr.state_dims())])
        self.moved = np.arange(max(1, n // 40))
        self.moved_states = np.concatenate([self.x1[off[i]:off[i + 1]] for i in self.moved])
        self.key = int(self.arr.var_keys[n // 2])

    def handle(self, gpu, arr=None, x=None, ordering=None, amalgamation=None):
        be = gpu.product_backend(self.arr if arr is None else arr)
        if self.pcg:
            be.set_linear_solver(A.SOLVER_PCG)
        if amalgamation is not None:
            be.set_amalgamation(*amalgamation)
        if x is not None:
            be.set_values(x)
        be.set_ordering(self.ord0 if ordering is None else ordering)
        return be

    def prepared(self, gpu, x=None):
        be = self.handle(gpu, x=x)
        be.linearize()
        be.solve(0.0, False)
        return be


_graphs = {}


def _graph(gpu, name):
    if name not in _graphs:
        if name.startswith("chain"):
            _graphs[name] = Graph(gpu, _chain(prior=True), name == "chain_pcg", None, 1.0)
        elif name == "pose3":
            _graphs[name] = Graph(gpu, PROBLEMS["pose3"], False, (A.ORDER_ND, A.ORDER_MINDEGREE), 1.0)
        else:
            _graphs[name] = Graph(gpu, PROBLEMS["bal_small"], False, (A.ORDER_SCHUR_ND, A.ORDER_SCHUR), 0.6)
    return _graphs[name]


def _plain(be, x):
    """The plain route to "linearized and solved at lambda = 0" on a handle that has its ordering."""
    be.set_values(x)
    be.linearize()
    try:
        be.solve(0.0, False, want_delta=False)
    except gt.IndeterminantLinearSystemException:
        pass


def _root(be):
    parent, _ = be.get_tree()
    return max(f for f, p in enumerate(parent) if p < 0)


def _groups(be):
    """gsx_get_hessian_groups as one array (host side: it answers in every state that has an ordering)."""
    g = be.hessian_groups()
    return np.concatenate([g[k] for k in ("class", "group", "position", "bundle", "bundle_size")] + [[int(g["fused_diag_star"])]])


READERS = [
    ("get_jacobians", lambda be, g: be.jacobians()),
    ("hessian_diagonal", lambda be, g: be.hessian_diagonal()),
    ("solve_0", lambda be, g: be.solve(0.0, False)),
    ("solve_1e-3", lambda be, g: be.solve(1e-3, False)),
    ("backsubstitute_wildfire", lambda be, g: np.append(*be.backsubstitute_wildfire(0.0))),
    ("relinearize_partial_none", lambda be, g: np.array([v for _, v in sorted(be.relinearize_partial([]).items())])),
    ("marginal_covariance", lambda be, g: be.marginal_covariance(g.key)),
    ("get_conditional_root", lambda be, g: be.conditional(_root(be))),
    ("linear_error", lambda be, g: np.array(be.linear_error())),
    ("retract_no_delta", lambda be, g: np.array([be.retract(None, commit=False)])),
    ("get_hessian_groups", lambda be, g: _groups(be)),
    ("get_hessian_panel", lambda be, g: np.concatenate([a.ravel() for a in be.hessian_panel(g.key)])),
]


def _lm_accept(be, g):
    p = A.lm_params_legacy()
    be.lm_reset(p)
    e0 = be.error()
    e1, _ = be.lm_iterate(p)
    assert e1 < e0 and not np.array_equal(be.get_values(), g.x0)   # a trial was taken


def _lm_trial_rejected(be, g):
    e0 = be.error()
    _, _, e1 = be.lm_trial(True, LAM_TRIAL)
    assert e1 > e0, (e0, e1)   # LM would reject it


def _update(be, g):
    be.update(g.arr_grown, np.append(np.arange(g.arr.n_factors), -1), np.zeros(0))


EVENTS = {
    "set_values": lambda be, g: be.set_values(g.x1),
    "retract_commit": lambda be, g: be.retract(None, commit=True, want_error=False),
    "gn_iteration": lambda be, g: be.gn_optimize(max_iterations=1),
    "dogleg_iteration": lambda be, g: be.dogleg_optimize(delta_initial=1.0, max_iterations=1),
    "lm_iteration_accepted": _lm_accept,
    "lm_trial_rejected": _lm_trial_rejected,
    "set_block_jacobians": lambda be, g: be.set_block_jacobians(g.f_lin, [g.block2]),
    "set_ordering": lambda be, g: be.set_ordering(g.ord1),
    "relinearize_partial_moved": lambda be, g: be.relinearize_partial(g.arr.var_keys[g.moved], g.moved_states),
    "update_one_factor": _update,
}

#              jac      hdiag    solve 0  solve l  wildfire relin    marginal cond     lin.err  retract  h.groups h.panel
_MOVED = ("state", "state", "state", "state", "state", "state", "ok", "old", "state", "state", "ok", "state")
_BLOCKS = ("ok", "ok", "ok", "ok", "state", "state", "ok", "state", "state", "state", "ok", "ok")
_ALL_OK = ("ok",) * 12
TABLE = {
    # the values moved, the arena was left alone: everything asks for a linearization, the marginal makes its own, and
    # the conditional is the previous linearization's
    "set_values": _MOVED,
    "retract_commit": _MOVED,
    "gn_iteration": _MOVED,        # (its factorization is that of the linearization at the values it started from)
    "dogleg_iteration": _MOVED,
    # LM drops the factorization with the values it accepted
    "lm_iteration_accepted": ("state", "state", "state", "state", "state", "state", "ok", "state", "state", "state", "ok",
                              "state"),
    # a damped factorization and its step are resident: no undamped one for the wildfire pass / the partial update
    "lm_trial_rejected": ("ok", "ok", "ok", "ok", "state", "state", "ok", "trial", "trial", "trial", "ok", "ok"),
    # new blocks / a new tree / a new graph under the same linearization point: linearized, nothing else
    "set_block_jacobians": _BLOCKS,
    "set_ordering": _BLOCKS,
    "update_one_factor": _BLOCKS,
    # the factorization is current, its back-substitution is not
    "relinearize_partial_moved": ("ok", "ok", "ok", "ok", "ok", "ok", "ok", "ok", "state", "state", "ok", "ok"),
}
# a PCG handle factors nothing in its drivers: the linearize of the iteration / trial drops the resident factorization
# and no new one arrives; Dogleg refuses the handle and leaves it as it was
TABLE_PCG = dict(TABLE)
TABLE_PCG["gn_iteration"] = _MOVED[:7] + ("state",) + _MOVED[8:]
TABLE_PCG["dogleg_iteration"] = _ALL_OK
TABLE_PCG["lm_trial_rejected"] = ("ok", "ok", "ok", "ok", "state", "state", "ok", "state", "trial", "trial", "ok", "ok")
EVENT_STATUS_PCG = {"dogleg_iteration": A.GSX_E_STATE}


def _call(fn, *args):
    """(status, output) of an entry point through the exceptions of the Python layer."""
    try:
        return A.GSX_OK, fn(*args)
    except gt.IndeterminantLinearSystemException:
        return A.GSX_E_INDETERMINATE, None
    except gt.GsxError as e:
        return e.status, None


_STATUS = {"ok": A.GSX_OK, "old": A.GSX_OK, "trial": A.GSX_OK, "state": A.GSX_E_STATE, "indet": A.GSX_E_INDETERMINATE}


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("event", list(EVENTS))
@pytest.mark.parametrize("name", ["chain", "pose3", "bal_small", "chain_pcg"])
def test_readers_after_event(gpu, name, event):
    g = _graph(gpu, name)
    row = (TABLE_PCG if g.pcg else TABLE)[event]
    want_event = EVENT_STATUS_PCG.get(event, A.GSX_OK) if g.pcg else A.GSX_OK
    start = g.x_far if event == "lm_trial_rejected" else None   # (None: the graph's initial values)
    # where the event leaves the handle: graph, values, ordering
    probe = g.prepared(gpu, start)
    st, _ = _call(EVENTS[event], probe, g)
    assert st == want_event, (name, event, st)
    arr_post = {"set_block_jacobians": g.arr_block2, "update_one_factor": g.arr_grown}.get(event, g.arr)
    x_post, ord_post = probe.get_values(), probe.get_ordering()
    # (gsx_update keeps the amalgamation setting the library chose for the tree it replaces; a handle left to choose for
    #  the new ordering may choose another one, hence other cliques and other rounding: the fresh handle is given the setting)
    stats = probe.stats()
    probe.close()
    fresh = g.handle(gpu, arr_post, x_post, ord_post,
                     (stats["amalgamation_relax"], int(stats["amalgamation_max_frontal_dim"])))
    before = None
    for (rname, reader), cell in zip(READERS, row):
        be = g.prepared(gpu, start)
        st, _ = _call(EVENTS[event], be, g)
        assert st == want_event
        st, out = _call(reader, be, g)
        be.close()
        assert st == _STATUS[cell], (name, event, rname, cell, st)
        if st != A.GSX_OK:
            continue
        if cell == "old":
            if before is None:
                before = g.handle(gpu)
            _plain(before, g.x0)
            ref = reader(before, g)
        else:
            _plain(fresh, x_post)
            if cell == "trial":
                fresh.linearize()
                if g.pcg:
                    fresh.solve_pcg(LAM_TRIAL, want_delta=False)
                else:
                    fresh.solve(LAM_TRIAL, False, want_delta=False)
            ref = reader(fresh, g)
        assert _same(out, ref), (name, event, rname, cell, float(np.max(np.abs(np.asarray(out, float) - np.asarray(ref, float)))))
    fresh.close()
    if before is not None:
        before.close()


#                   jac   hdiag solve 0  solve l wildfire relin    marginal cond     lin.err  retract  h.groups h.panel
ROW_FAILED = ("ok", "ok", "indet", "ok", "state", "state", "indet", "state", "state", "state", "ok", "ok")


def test_readers_after_a_failed_factorization(gpu):
    """The gauge-free chain: a Gauss-Newton run (lambda = 0) fails — after iterations that rounding let through, so the
    values have moved by then.  The linearization and H stay, the wreck in the arena is never served, and a marginal query
    fails again.  (A handle whose solver is PCG factors nothing in its Gauss-Newton run and does not fail here: the direct
    solver only.)"""
    arr = _chain(prior=False)
    ordering = np.array(arr.var_keys)

    def handle():
        be = gpu.product_backend(arr)
        be.set_ordering(ordering)
        return be

    class G:
        key = int(arr.var_keys[2])
    fresh = handle()
    for (rname, reader), cell in zip(READERS, ROW_FAILED):
        be = handle()
        st, _ = _call(lambda: be.gn_optimize(max_iterations=3))
        assert st == A.GSX_E_INDETERMINATE
        x_post = be.get_values()
        st, out = _call(reader, be, G)
        be.close()
        assert st == _STATUS[cell], (rname, cell, st)
        if st == A.GSX_OK:
            _plain(fresh, x_post)
            assert _same(out, reader(fresh, G)), rname
    fresh.close()
