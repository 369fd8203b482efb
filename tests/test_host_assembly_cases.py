"""tests/_assembly_cases.py without a GPU: every case reaches the assembly class, bundle and group it was built for
(gsx_get_hessian_groups answers on a host-only handle), the judge accepts a float64 restatement of the panel through the
term lists and rejects each of four wrong ones on both data sets, and expected_panel agrees with mpmath at 50 digits."""
import mpmath
import numpy as np
import pytest

from gtsam_petercdev_amd import _abi as A
from gtsam_petercdev_amd import _lib

from tests import _assembly_cases as AC


@pytest.mark.parametrize("name", list(AC.CASES))
def test_case_reaches_its_class(name):
    case = AC.CASES[name]
    hb = _lib.ProductBackend(case.arrays("int"), host_only=True)
    hb.set_ordering(case.ordering)
    g = hb.hessian_groups()
    hb.close()
    AC.check_groups(case, g)
    assert not g["fused_diag_star"] or case.fused
    assert g["fused_diag_star"] == case.fused   # (a host-only handle has no star leaves: the GSX_FUSED_STAR=0 plan)
    assert np.all(g["class"] >= 0)


def test_every_class_and_star_form_is_reached():
    reached = {c for case in AC.CASES.values() for c in case.expect.values()}
    assert reached == set(range(6))
    sizes = {s for case in AC.CASES.values() for s in case.bundles.values()}
    assert {0, 1, 2, 4, 5} <= sizes
    assert any(case.fused for case in AC.CASES.values())


@pytest.mark.parametrize("cls", range(6), ids=AC.NAMES)
def test_partial_case_marks_a_strict_inner_part_of_its_group(cls):
    pc = AC.partial_case(cls)
    hb = _lib.ProductBackend(pc.arr, host_only=True)
    hb.set_amalgamation(0.0, 128)
    hb.set_ordering(pc.ordering)
    AC.check_partial_groups(pc, hb.hessian_groups())
    _, fronts = hb.get_tree()
    hb.close()
    assert len(fronts) >= AC.N_PADS


def test_host_only_handle_refuses_a_panel():
    case = AC.CASES["heavy_terms_97"]
    hb = _lib.ProductBackend(case.arrays("int"), host_only=True)
    with pytest.raises(A.GsxError) as e:
        hb.hessian_groups()
    assert e.value.status == A.GSX_E_STATE
    hb.set_ordering(case.ordering)
    with pytest.raises(A.GsxError) as e:
        hb.hessian_panel(0)
    # (no device here, or a device but no values on it: either way there is nothing to assemble from)
    assert e.value.status in (A.GSX_E_NO_DEVICE, A.GSX_E_STATE)
    hb.close()


# the restatement walks the heavy kernel's four chunks; the cases have at least 64 terms, several partners, factors of
# equal rows
@pytest.mark.parametrize("data", AC.DATA)
@pytest.mark.parametrize("name", ["heavy_terms_97", "heavy_terms_261", "tile_terms_64"])
def test_judge_accepts_the_restatement_and_rejects_every_mutation(name, data):
    case = AC.CASES[name]
    arr = case.arrays(data)
    jac = AC.host_jacobians(arr)
    if data == "int":
        assert np.all(jac == np.round(jac)) and np.max(np.abs(jac)) <= 8
    p = AC.expected_panel(arr, jac, 0, case.ordering)
    cls = case.expect[0]
    ok, worst, k = AC.judge(AC.restated_panel(arr, jac, 0, case.ordering), p, cls, data)
    print("%s %s: restatement %.2f u, k <= %d" % (name, data, worst, k))
    assert ok
    for mut in AC.MUTATIONS:
        ok, worst, _ = AC.judge(AC.restated_panel(arr, jac, 0, case.ordering, mutation=mut), p, cls, data)
        assert not ok, (name, data, mut, worst)


def test_judge_rejects_a_panel_of_another_shape():
    case = AC.CASES["tile_cols_16"]
    arr = case.arrays("int")
    jac = AC.host_jacobians(arr)
    p = AC.expected_panel(arr, jac, 0)
    assert not AC.judge(np.asarray(p.exact, float)[:-1], p, AC.TILE, "int")[0]
    assert AC.judge(np.asarray(p.exact, float), p, AC.TILE, "int")[0]


def _mp_panel(arr, jac, var):
    """The panel from the definition in mpmath: an independent loop over scalars, index order = elimination order."""
    off = arr.jacobian_offsets()
    dims = [int(d) for d in arr.var_dims]
    facs = []
    for f in range(arr.n_factors):
        vs = [int(v) for v in arr.f_vars[arr.f_key_ptr[f]:arr.f_key_ptr[f + 1]]]
        if var in vs:
            facs.append((f, vs))
    later = sorted({u for _, vs in facs for u in vs if u > var})
    rows = [(var, k) for k in range(dims[var])] + [(u, k) for u in later for k in range(dims[u])] + [(-1, 0)]
    out = [[mpmath.mpf(0)] * dims[var] for _ in rows]
    for f, vs in facs:
        m = int(arr.f_rows[f])
        col = {v: sum(dims[w] for w in vs[:i]) for i, v in enumerate(vs)}
        col[-1] = sum(dims[w] for w in vs)
        e = lambda r, c: mpmath.mpf(float(jac[off[f] + c * m + r]))
        for i, (u, k) in enumerate(rows):
            if u in col:
                for j in range(dims[var]):
                    out[i][j] += mpmath.fsum(e(r, col[u] + k) * e(r, col[var] + j) for r in range(m))
    return out


@pytest.mark.parametrize("name,var", [("tile_ternary_first_and_middle", 1), ("light_rows_1_3_5_9", 0)])
def test_expected_panel_against_mpmath(name, var):
    case = AC.CASES[name]
    arr = case.arrays("real")
    jac = AC.host_jacobians(arr)
    p = AC.expected_panel(arr, jac, var, case.ordering)
    with mpmath.workdps(50):
        ref = _mp_panel(arr, jac, var)
        assert (len(ref), len(ref[0])) == p.exact.shape
        for i in range(p.exact.shape[0]):
            for j in range(p.exact.shape[1]):
                # longdouble sums of at most a few dozen products: 2^-60 of |A_B|'|A_A| is far below the unit judged in
                hi = float(p.exact[i, j])
                got = mpmath.mpf(hi) + mpmath.mpf(float(p.exact[i, j] - AC.LD(hi)))   # (all 64 bits)
                err = abs(got - ref[i][j])
                assert err <= mpmath.mpf(2) ** -58 * mpmath.mpf(float(p.mag[i, j])), (i, j, err)
        assert any(ref[i][j] != 0 for i in range(len(ref)) for j in range(len(ref[0])))
