"""The restatement of the border (tests/_append_refs.py) against the oracle, on the inputs the GPU tests run
(tests/_append_cases.py), and the refusals of the Python front end that need no device call.

For every patch of every fp64 case:
    kappa2(L') <= 10^3                                         (the cases are chosen so; the GPU bound relies on it)
    the bordered L' and c' of the restatement agree with oracle.fit_patch on the extended point set, and L' with
    oracle.cholesky_lower of the extended K + sigma2 I, within ONE unit e = (n + m + 32) u kappa2(L') max |L'|, u = 2^-53.
The fp32 cases share the geometry (points rounded to fp32, a larger sigma2): their kappa2 is asserted too.
"""
import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import mixture as M
from oracle import oracle as O
import _append_cases as AC
import _append_refs as AR


def _cases(dtype):
    return {name: (case, fams, s2) for name, case, fams, s2 in AC.all_cases(dtype)}


NAMES = [name for name, _, _, _ in AC.all_cases("f64")]


@pytest.mark.parametrize("name", NAMES)
def test_border_restatement_matches_the_oracle(name):
    case, fams, s2 = _cases("f64")[name]
    worst = {}
    for r in range(case.P):
        oth = AC.FAMILIES[fams[r]][1]
        n, m = case.sizes[r]
        de = None if case.de is None else case.de[r]
        fit = O.fit_patch(oth, case.Xe[r], case.ye[r], s2[r], want_K=True, diag=de)
        assert fit["info"] == 0, (name, r)
        U = fit["K"].copy()
        U[np.diag_indices(n + m)] += s2[r]
        kappa = AR.kappa_of(U)
        assert kappa <= AC.KAPPA_MAX, (name, r, kappa)
        ref = AR.border_ref(oth, case.Xs[r], case.ys[r], s2[r], case.Xn[r], case.yn[r],
                            None if case.ds is None else case.ds[r], None if case.dn is None else case.dn[r])
        e = AR.unit(n + m, "f64", kappa, ref["L"])
        st, Lc = O.cholesky_lower(U)
        assert st == 0
        got = dict(L_fit=AR.ratio(fit["L"], ref["L"], e), L_chol=AR.ratio(Lc, ref["L"], e),
                   c_chol=AR.ratio(fit["c_chol"], ref["c"], e), c_lu=AR.ratio(fit["c_lu"], ref["c"], e))
        for k, v in got.items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= 1.0, (name, r, n, m, k, v, kappa)
    print("APPEND_REF", name, {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("name", NAMES)
def test_fp32_cases_are_as_well_conditioned(name):
    case, fams, s2 = _cases("f32")[name]
    for r in range(case.P):
        oth = AC.FAMILIES[fams[r]][1]
        U = O.kernel_matrix(oth, case.Xe[r]) + s2[r] * np.eye(len(case.Xe[r]))
        if case.de is not None:
            U[np.diag_indices(len(U))] += case.de[r]
        assert AR.kappa_of(U) <= AC.KAPPA_MAX, (name, r)


def test_the_cases_cover_the_edges():
    sizes = AC.MAIN_SIZES + AC.TALL_SIZES
    grown = {(n, n + m) for n, m in sizes}
    assert grown >= {(1, 2), (1, 128), (30, 35), (31, 32), (32, 33), (96, 128), (127, 128), (129, 256), (272, 298),
                     (300, 301), (513, 520), (672, 673), (865, 896)}
    assert (128, 0) in sizes and any(m == 0 and n % 128 for n, m in sizes)
    # every count of 32-row pairs in the last block row, before and after
    assert {((n - 1) % 128) // 32 + 1 for n, _ in sizes} == {1, 2, 3, 4}
    # every column width of the border kernel, and m on both sides of each switch between two widths
    every = [nm for _, case, _, _ in AC.all_cases("f64") for nm in case.sizes]
    assert set(AC.WIDTH_SIZES) <= set(every)
    assert {AC.column_width(m) for _, m in every if m} == {16, 32, 64, 128}
    assert {m for _, m in every} >= {16, 17, 32, 33, 64, 65}
    assert AC.column_width(64) == 64 and sum(1 for _, m in AC.WIDTH_SIZES if AC.column_width(m) == 64) >= 4
    for n, m in sizes + every:
        assert n + m <= 128 * ((n + 127) // 128)


# ------------------------------------------------------------------------------------------ refusals without a device call
def test_append_items_groups_and_validates():
    n = np.array([30, 128, 5])
    Xn = [np.zeros((2, 2)), np.zeros((0, 2)), np.ones((1, 2))]
    yn = [np.array([1.0, 2.0]), np.zeros(0), np.array([3.0])]
    x, y, diag, patch, parts = M.append_items(Xn, yn, None, n, 2)
    assert x.shape == (3, 2) and np.array_equal(y, [1.0, 2.0, 3.0]) and diag is None
    assert patch.dtype == np.int32 and np.array_equal(patch, [0, 0, 2])
    assert [p.shape for p in parts] == [(2, 2), (0, 2), (1, 2)]
    _, _, diag, _, _ = M.append_items(Xn, yn, [np.array([0.1, 0.2]), None, np.array([0.3])], n, 2)
    assert np.array_equal(diag, [0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="one array of new points per patch: got 2 for 3 patches"):
        M.append_items(Xn[:2], yn, None, n, 2)
    with pytest.raises(ValueError, match="one vector of new targets per patch"):
        M.append_items(Xn, yn[:1], None, n, 2)
    with pytest.raises(ValueError, match=r"patch 0: new points must have shape \(m, 2\)"):
        M.append_items([np.zeros((2, 3)), Xn[1], Xn[2]], yn, None, n, 2)
    with pytest.raises(ValueError, match="patch 0: 1 targets for 2 new points"):
        M.append_items(Xn, [np.zeros(1), yn[1], yn[2]], None, n, 2)
    with pytest.raises(ValueError, match="patch 2: 2 addends for 1 new points"):
        M.append_items(Xn, yn, [None, None, np.zeros(2)], n, 2)
    with pytest.raises(ValueError, match="patch 2: non-finite"):
        M.append_items(Xn, [yn[0], yn[1], np.array([np.nan])], None, n, 2)
    with pytest.raises(ValueError, match="patch 0: non-finite"):
        M.append_items([np.array([[np.inf, 0.0], [0.0, 0.0]]), Xn[1], Xn[2]], yn, None, n, 2)
    # a full patch, and one row too many
    with pytest.raises(ValueError, match=r"patch 1 has 0 free rows \(n = 128\), 1 rows asked for"):
        M.append_items([Xn[1], np.zeros((1, 2)), Xn[1]], [yn[1], np.zeros(1), yn[1]], None, n, 2)
    with pytest.raises(ValueError, match=r"patch 0 has 98 free rows \(n = 30\), 99 rows asked for"):
        M.append_items([np.zeros((99, 2)), Xn[1], Xn[1]], [np.zeros(99), yn[1], yn[1]], None, n, 2)


def test_append_counts_limit():
    n = np.full(200, 1)
    M.check_append_counts(np.full(200, 81), n)                   # 16200 items
    with pytest.raises(ValueError, match="16400 items in one call, the limit is 16384"):
        M.check_append_counts(np.full(200, 82), n)


class _Unfitted:
    """the state flags of a DeviceModel without a device behind it"""
    _has_factor, _has_targets, _from_tree = False, True, False
    _need, _need_appendable = M.DeviceModel._need, M.DeviceModel._need_appendable
    _need_tree_model = M.DeviceModel._need_tree_model
    append, append_global = M.DeviceModel.append, M.DeviceModel.append_global


def test_state_refusals_need_no_device():
    m = _Unfitted()
    with pytest.raises(pmk.PmkError, match="no factor"):
        m.append([], [])
    m._has_factor, m._has_targets = True, False
    with pytest.raises(pmk.PmkError, match="append: a model built from factors holds no targets"):
        m.append([], [])
    m._has_targets = True
    with pytest.raises(pmk.PmkError, match="append_global: the model was built from lists of patches"):
        m.append_global(np.zeros((1, 2)), np.zeros(1))
    m._from_tree = True
    with pytest.raises(pmk.PmkError, match="append: a model built by from_tree takes append_global"):
        m.append([], [])
    eta = pmk.MixtureGPType([np.zeros((3, 2))], [])
    with pytest.raises(pmk.PmkError, match="fitmixtureGP_ must run before appendmixtureGP_"):
        pmk.appendmixtureGP_(eta, [np.zeros((1, 2))], [np.zeros(1)])
