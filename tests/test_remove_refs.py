"""The restatement of the row deletion (tests/_remove_refs.py) against the Cholesky factor of the reduced matrix and the
oracle, on the inputs the GPU tests run (tests/_remove_cases.py), and the refusals of the Python front end that need no
device call.

For every patch of every fp64 case:
    kappa2(L) <= 10^3 for the full patch (the GPU unit is made of it) and for the reduced one
    the swept L' and c' agree with cholesky_ld of U[keep, keep] and with oracle.fit_patch on the reduced set within ONE
    unit e = (n + 32) u kappa2(L) max |L|, u = 2^-53
    nothing appears right of j + s_j (the band claim): exactly zero
    the reduced model's mean at a removed point is y_i - c_i / d_i of the full one, d = diag(U^-1), and its variance
    plus sigma2 (plus the addend) is 1 / d_i
The fp32 cases share the geometry (points rounded to fp32, a larger sigma2): their kappa2 is asserted too.
"""
import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import mixture as M
from oracle import oracle as O
import _remove_cases as RC
import _remove_refs as RR
from _loo_refs import LD, forward_ld, linv_colnorms_ld


def _cases(dtype):
    return {name: (case, fams, s2) for name, case, fams, s2 in RC.all_cases(dtype)}


NAMES = [name for name, _, _, _ in RC.all_cases("f64")]


@pytest.mark.parametrize("name", NAMES)
def test_sweep_matches_the_cholesky_of_the_reduced_matrix_and_the_oracle(name):
    case, fams, s2 = _cases("f64")[name]
    worst = {}
    for r in range(case.P):
        oth = RC.FAMILIES[fams[r]][1]
        n, rows = len(case.Xs[r]), case.rows[r]
        ds = None if case.ds is None else case.ds[r]
        dr = None if case.dr is None else case.dr[r]
        kappa = RR.kappa_of(RR.gram(oth, case.Xs[r], s2[r], ds))
        assert kappa <= RC.KAPPA_MAX, (name, r, kappa)
        assert RR.kappa_of(RR.gram(oth, case.Xr[r], s2[r], dr)) <= RC.KAPPA_MAX, (name, r)
        ref = RR.remove_ref(oth, case.Xs[r], case.ys[r], s2[r], rows, ds)
        assert ref["fill"] == 0.0, (name, r, ref["fill"])                      # the band claim
        assert np.all(np.diag(ref["L"]) > 0)
        # a new diagonal is at least the old one of the row it came from
        keep = case.keep[r]
        assert np.all(np.diag(ref["L"]) >= np.diag(ref["L_full"])[keep]), (name, r)
        fit = O.fit_patch(oth, case.Xr[r], case.yr[r], s2[r], want_K=True, diag=dr)
        assert fit["info"] == 0, (name, r)
        e = RR.unit(n, "f64", kappa, ref["L_full"])
        got = dict(L_chol=RR.ratio(ref["L"], ref["L_chol"], e), c_chol=RR.ratio(ref["c"], ref["c_chol"], e),
                   L_fit=RR.ratio(fit["L"], ref["L"], e), c_fit=RR.ratio(fit["c_chol"], ref["c"], e),
                   L_fit_chol=RR.ratio(fit["L"], ref["L_chol"], e))
        for k, v in got.items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= 1.0, (name, r, n, len(rows), k, v, kappa)
    print("REMOVE_REF", name, {k: "%.3g" % v for k, v in worst.items()})


@pytest.mark.parametrize("name", NAMES)
def test_fp32_cases_are_as_well_conditioned(name):
    case, fams, s2 = _cases("f32")[name]
    for r in range(case.P):
        oth = RC.FAMILIES[fams[r]][1]
        for X, d in ((case.Xs[r], None if case.ds is None else case.ds[r]), (case.Xr[r], None if case.dr is None else case.dr[r])):
            U = O.kernel_matrix(oth, X) + s2[r] * np.eye(len(X))
            if d is not None:
                U[np.diag_indices(len(U))] += d
            assert RR.kappa_of(U) <= RC.KAPPA_MAX, (name, r)


@pytest.mark.parametrize("name", ["small", "tiles", "addends"])
def test_the_reduced_model_predicts_the_leave_one_out_value(name):
    """one removed row at a time: mean(x_i | the others) = y_i - c_i / d_i and var + sigma2 (+ addend_i) = 1 / d_i"""
    case, fams, s2 = _cases("f64")[name]
    for r in range(case.P):
        oth = RC.FAMILIES[fams[r]][1]
        X, y, ds = case.Xs[r], np.asarray(case.ys[r], dtype=LD), None if case.ds is None else case.ds[r]
        n = len(X)
        if n < 2 or not len(case.rows[r]):
            continue
        U = RR.gram(oth, X, s2[r], ds)
        full = RR.remove_ref(oth, X, case.ys[r], s2[r], [], ds)
        kappa = RR.kappa_of(U)
        d = linv_colnorms_ld(full["L"])
        for i in sorted({int(case.rows[r][0]), int(case.rows[r][-1])}):
            red = RR.delete_rows_ld(full["L"], full["z"], [i])
            keep = np.setdiff1d(np.arange(n), [i])
            kq = U[keep, i]
            mean = kq @ red["c"]
            w = forward_ld(red["L"], kq)
            var_noisy = U[i, i] - w @ w
            # both sides are long-double solves with U: each within (n + 32) 2^-64 cond2(U) of its terms' magnitudes
            tol = (n + 32) * 2.0 ** -64 * kappa ** 2
            scale = float(np.abs(y).max() + np.abs(full["c"]).max() * np.abs(U).max())
            assert abs(mean - (y[i] - full["c"][i] / d[i])) <= tol * scale, (name, r, i)
            assert abs(var_noisy - 1 / d[i]) <= tol * float(U[i, i]), (name, r, i)


def test_the_cases_cover_the_edges():
    every = [(n, tuple(rows)) for _, case, _, _ in RC.all_cases("f64") for n, rows in case.sizes]
    shrunk = {(n, n - len(rows)) for n, rows in every}
    assert shrunk >= {(2, 1), (33, 32), (130, 129), (300, 296), (300, 300 - RC.MAX_ROWS), (384, 383), (384, 380)}
    assert {(2, (0,)), (2, (1,)), (33, (0,)), (33, (31,)), (33, (32,)), (130, (0,)), (130, (127,)), (130, (128,)),
            (130, (129,)), (300, (5, 127, 128, 299)), (384, (383,)), (384, (380, 381, 382, 383))} <= set(every)
    assert any(len(rows) == RC.MAX_ROWS and rows[0] == 0 and rows[-1] == n - 1 for n, rows in every)
    assert any(not rows for _, rows in every)
    assert {case.D for _, case, _, _ in RC.all_cases("f64")} == {1, 2, 4}
    for n, rows in every:
        assert len(rows) <= min(RC.removable(n), RC.MAX_ROWS) and len(set(rows)) == len(rows)
    assert RC.removable(300) == 43 and RC.removable(2) == 1 and RC.removable(128) == 127 and RC.removable(129) == 0
    assert RC.MAX_ROWS == M.MAX_REMOVE_ROWS


# ------------------------------------------------------------------------------------------ refusals without a device call
def test_remove_items_groups_and_validates():
    n = np.array([30, 300, 5])
    patch, row, parts = M.remove_items([[3, 1], np.zeros(0, dtype=np.int64), np.array([4])], n)
    assert patch.dtype == np.int32 and np.array_equal(patch, [0, 0, 2])
    assert row.dtype == np.int64 and np.array_equal(row, [1, 3, 4])
    assert [list(p) for p in parts] == [[1, 3], [], [4]]
    with pytest.raises(ValueError, match="one array of rows per patch: got 2 for 3 patches"):
        M.remove_items([[0], []], n)
    with pytest.raises(ValueError, match="patch 0: the rows must be integers"):
        M.remove_items([[0.5], [], []], n)
    with pytest.raises(ValueError, match="patch 2: a row outside 0 .. 4"):
        M.remove_items([[], [], [5]], n)
    with pytest.raises(ValueError, match="patch 0: a row outside 0 .. 29"):
        M.remove_items([[-1], [], []], n)
    with pytest.raises(ValueError, match="patch 0: a row is given twice"):
        M.remove_items([[2, 2], [], []], n)
    # the band rule and the cap
    with pytest.raises(ValueError, match=r"patch 2 has 4 removable rows \(n = 5\), 5 rows asked for"):
        M.remove_items([[], [], [0, 1, 2, 3, 4]], n)
    with pytest.raises(ValueError, match="33 rows of patch 1 in one call, the limit is 32"):
        M.remove_items([[], np.arange(33), []], n)
    with pytest.raises(ValueError, match=r"patch 1 has 43 removable rows \(n = 300\), 44 rows asked for"):
        M.remove_items([[], np.arange(44), []], n)


class _Unfitted:
    """the state flags of a DeviceModel without a device behind it"""
    _has_factor, _has_targets, _from_tree = False, True, False
    _need, _need_appendable = M.DeviceModel._need, M.DeviceModel._need_appendable
    _need_tree_model = M.DeviceModel._need_tree_model
    remove, remove_global = M.DeviceModel.remove, M.DeviceModel.remove_global


def test_state_refusals_need_no_device():
    m = _Unfitted()
    with pytest.raises(pmk.PmkError, match="no factor"):
        m.remove([])
    m._has_factor, m._has_targets = True, False
    with pytest.raises(pmk.PmkError, match="remove: a model built from factors holds no targets"):
        m.remove([])
    m._has_targets = True
    with pytest.raises(pmk.PmkError, match="remove_global: the model was built from lists of patches"):
        m.remove_global([0])
    m._from_tree = True
    with pytest.raises(pmk.PmkError, match="remove: a model built by from_tree takes remove_global"):
        m.remove([])
    eta = pmk.MixtureGPType([np.zeros((3, 2))], [])
    with pytest.raises(pmk.PmkError, match="fitmixtureGP_ must run before removemixtureGP_"):
        pmk.removemixtureGP_(eta, [[0]])
