"""Removing observations from a fitted model in place on the GPU (pmk_model_remove / pmk_model_removable, the kernel of
pmk_remove.hip; DeviceModel.remove / remove_global, removemixtureGP_).

References: the oracle on the reduced point set, and a fresh DeviceModel of the reduced lists (the fit, which the removal
does not touch).  The inputs are those of tests/_remove_cases.py, of which tests/test_remove_refs.py asserts
kappa2(L) <= 10^3 and that the long-double reflector sweep stays within one unit of the oracle.

Accuracy.  L' (all rows), c' and the recomputed -D^-1 blocks against the oracle in units
    e = (n + 32) u kappa2(L) max |L|,   u = 2^-53 (fp64) or 2^-24 (fp32),   n and L those of the patch BEFORE the call:
the resident factor carries the error of a fit of n rows and the deletion, being orthogonal, adds a term of the same form.
Bound: the project's 10 units.  The fresh device fit's own ratio is measured on the same inputs; both go to
profiles/remove_accuracy.json when the whole module runs ("REMOVE {json}" with -s).

One call takes at most PMK_REMOVE_MAX_ROWS = 32 rows of a patch, so 300 -> 257, the band's edge, is two calls (32 rows, then 11):
the cap, the band's edge, and the refusal one row beyond each.

z has no accessor: it is covered by c' (the back substitution of z') and by the bit checks of a later fit.

The `slabs` case of tests/_remove_cases.py goes through the first test like every other: full patches (n = ld) that lose
their first row, their last row or both, one run of 32 rows inside a tile and astride the tile edge, and more than 512
rows below the first removed one.  What runs after a removal on a tree-built model is in tests/test_gpu_remove_after.py.
"""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
from patchmixturekriging_amd import mixture as M
from oracle import oracle as O
import _append_cases as AC
import _cov_refs as CR
import _remove_cases as RC
import _remove_refs as RR
import _trend_refs as T
import test_gpu_append as TA
import test_gpu_append_after as TAA

pytestmark = pytest.mark.gpu

RATIO_MAX = RC.RATIO_MAX
_RECORDS = []
ACCURACY_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "remove_accuracy.json")
CASE_NAMES = [name for name, _, _, _ in RC.all_cases("f64")]
_fit, _refit, _packed, _state, _hash = TA._fit, TA._refit, TA._packed, TA._state, TA._hash


def _record(**kw):
    _RECORDS.append(kw)
    print("REMOVE " + json.dumps(kw, sort_keys=True))


@pytest.fixture(scope="module", autouse=True)
def _write_accuracy_file():
    """only a run of the whole module replaces the file"""
    yield
    if {(r["case"], r["dtype"]) for r in _RECORDS} >= {(n, d) for n in CASE_NAMES + ["band_edge", "window"] for d in ("f64", "f32")}:
        with open(ACCURACY_JSON, "w") as f:
            f.write("[\n" + ",\n".join(" " + json.dumps(r, sort_keys=True) for r in _RECORDS) + "\n]\n")


def _oracle_fit(oth, X, y, s2, d=None):
    """the oracle's fit with kappa2(L)"""
    fit = O.fit_patch(oth, X, y, s2, want_K=True, diag=d)
    assert fit["info"] == 0
    U = fit["K"].copy()
    U[np.diag_indices(len(U))] += s2
    fit["kappa"] = RR.kappa_of(U)
    return fit


def _oracles(case, fams, s2):
    """per patch (the oracle's fit of the full set, of the reduced set): kappa2 and max |L| of the first make the unit"""
    full, red = [], []
    for r in range(case.P):
        oth = RC.FAMILIES[fams[r]][1]
        full.append(_oracle_fit(oth, case.Xs[r], case.ys[r], s2[r], None if case.ds is None else case.ds[r]))
        red.append(_oracle_fit(oth, case.Xr[r], case.yr[r], s2[r], None if case.dr is None else case.dr[r]))
    return full, red


def _block_tol(e, dtype, Lss, N):
    """a recomputed -D^-1 block against the fresh fit's, as tests/test_gpu_append.py bounds it: each device L' is within 10 e
    of the oracle entry by entry, so the 32 x 32 blocks L_ss differ by dL, |dL|_F <= 32 * 20 e, and N = -L_ss^-1 moves by
    N dL N to first order; each inversion adds its own 32 u |N|_2^2 |L_ss|_2 at most"""
    k = len(Lss)
    N2 = np.linalg.norm(N[:k, :k], 2)
    return N2 ** 2 * (32 * 2 * RATIO_MAX * e + 2 * 32 * RR.U_OF[dtype] * np.linalg.norm(Lss, 2))


def _check_patch(r, n, rows, keep, before, after, fresh, full, red, dtype, split, label):
    """the bit claims and the accuracy of one patch -> dict of ratios"""
    (L0, c0, inv0), (L1, c1, inv1), (Lf, cf, invf) = before, after, fresh
    m, n1 = len(rows), n - len(rows)
    assert L1.shape == (n1, n1)
    if m == 0:
        # a patch that lost nothing: every bit (the split path forms z and c again for every patch)
        assert np.array_equal(L1, L0) and np.array_equal(inv1, inv0), r
        assert np.array_equal(c1, c0) or split, r
        k0 = n
    else:
        k0 = int(rows[0])
        tail = keep[k0:]
        assert np.array_equal(L1[:k0, :k0], L0[:k0, :k0]), r                   # rows and columns < k0
        assert np.array_equal(L1[k0:, :k0], L0[tail, :k0]), r                  # the moved left block, from the rows it came from
        if k0 == n1:                                                            # the last rows only: no transformation at all
            assert np.array_equal(L1, L0[:n1, :n1]), r
    e = RR.unit(n, dtype, full["kappa"], full["L"])
    for b in range(inv0.shape[0]):
        if b < k0 // 32:
            assert np.array_equal(inv1[b], inv0[b]), (r, b)                     # the blocks before k0 / 32 are not written
        elif 32 * b >= n1:
            assert np.array_equal(inv1[b], invf[b]), (r, b)                     # wholly in padding: the padding's own
        else:
            Lss = red["L"][32 * b:32 * b + 32, 32 * b:32 * b + 32]
            tol = _block_tol(e, dtype, Lss, invf[b])
            assert np.abs(inv1[b] - invf[b]).max() <= tol, (r, b, np.abs(inv1[b] - invf[b]).max(), tol)
            assert np.array_equal(np.triu(inv1[b], 1), np.zeros((32, 32))), (r, b)
    got = dict(L=RR.ratio(L1, red["L"], e), c=RR.ratio(c1, red["c_chol"], e),
               L_fresh=RR.ratio(Lf, red["L"], e), c_fresh=RR.ratio(cf, red["c_chol"], e))
    print("REMOVE_PATCH", label, dtype, r, n, m, {k: round(v, 4) for k, v in got.items()})
    return got


def _check_scores_of_one_point(model, fresh, refs, case, dtype):
    """_check_scores of tests/test_gpu_append.py for a model that holds a patch of ONE point (2 -> 1).  Its bounds on log det
    and y^T c grow with n cond, which at n = 1 and cond = 1 allows two roundings, while c' = z' / L' of the deletion is a
    square root of a sum of two squares, a reflector applied to z and a division: the handful of roundings of the
    evaluation itself, for which that function adds 32 to cond in its other two bounds and the error unit adds 32 to n.
    Here n takes the same + 32 in the two bounds that have n; everything else is that function's."""
    u = RR.U_OF[dtype]
    ld_a, q_a = model.evidence()
    ld_f, q_f = fresh.evidence()
    model.loo(); fresh.loo()
    (res_a, var_a), (res_f, var_f) = model.loo_values(), fresh.loo_values()
    for r in range(case.P):
        n, cond, ymax = len(case.ye[r]), refs[r]["kappa"] ** 2, np.abs(case.ye[r]).max()
        cmax = np.abs(refs[r]["c_chol"]).max()
        assert abs(ld_a[r] - ld_f[r]) <= 2 * (n + 32) * cond * 1e-14 * (u / 2.0 ** -53), (r, ld_a[r], ld_f[r])
        assert abs(q_a[r] - q_f[r]) <= 2 * (n + 32) * cond * u * ymax * cmax, (r, q_a[r], q_f[r])
        assert np.all(np.abs(var_a[r] - var_f[r]) <= 2 * (cond + 32) * u * var_f[r]), r
        assert np.all(np.abs(res_a[r] - res_f[r]) <= 2 * (cond + 32) * u * ymax), r


def _compare(model, fresh, case, fams, s2, dtype, before, split, label):
    """everything the first test claims of a model after the removal against the fresh model of the reduced lists"""
    after, fstate = _state(model), _state(fresh)
    full, red = _oracles(case, fams, s2)
    worst = dict(L=0.0, c=0.0, L_fresh=0.0, c_fresh=0.0, kappa=0.0)
    for r in range(case.P):
        n, rows = len(case.Xs[r]), case.rows[r]
        got = _check_patch(r, n, rows, case.keep[r], before[r], after[r], fstate[r], full[r], red[r], dtype, split, label)
        for what in ((0, 1, 2) if case.ds is not None else (0, 1)):             # the packed buffers, padding included
            assert np.array_equal(_packed(model, r, what), _packed(fresh, r, what)), (r, what)
        assert np.array_equal(model.get(r, M.GET_K), fresh.get(r, M.GET_K)), r
        for k, v in got.items():
            worst[k] = max(worst[k], v)
        worst["kappa"] = max(worst["kappa"], full[r]["kappa"], red[r]["kappa"])
    _record(case=label, dtype=dtype, **worst)
    assert worst["kappa"] <= RC.KAPPA_MAX
    assert worst["L"] <= RATIO_MAX and worst["c"] <= RATIO_MAX, worst
    for f in red:
        f["c_chol"] = np.asarray(f["c_chol"])
    shim = types.SimpleNamespace(P=case.P, ye=case.yr)
    if min(len(v) for v in case.yr) >= 2:
        TA._check_scores(model, fresh, red, shim, dtype)         # the sizes it is written for: "down to two points"
    else:
        _check_scores_of_one_point(model, fresh, red, shim, dtype)
    # a fit after the removal is the fit of the fresh model, bit for bit: n, padding and host state are right
    _refit(model, fams, s2)
    assert np.array_equal(model.info(), fresh.info())
    for r, (L, c, inv) in enumerate(_state(model)):
        assert np.array_equal(L, fstate[r][0]) and np.array_equal(c, fstate[r][1]) and np.array_equal(inv, fstate[r][2]), r


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_remove_against_the_oracle_and_a_fresh_model(name, dtype):
    case, fams, s2 = {n: (c, f, s) for n, c, f, s in RC.all_cases(dtype)}[name]
    split = name == "split"
    model = _fit(case.Xs, case.ys, fams, s2, dtype, case.ds, split)
    assert np.all(model.info() == 0)
    can = model.removable()
    assert np.array_equal(can, [RC.removable(len(x)) for x in case.Xs])
    before = _state(model)
    model.loo()                                  # the leave-one-out tasks and d of the old factor exist: d goes stale
    info = model.remove(case.rows)
    assert np.all(info == 0), info
    with pytest.raises(pmk.PmkError, match="loo\\(\\) has not run"):
        model.loo_values()
    assert np.array_equal(model.n, [len(x) for x in case.Xr])
    assert np.array_equal(model.removable(), can - np.array([len(v) for v in case.rows]))
    assert all(np.array_equal(a, b) for a, b in zip(model.X, case.Xr))
    fresh = _fit(case.Xr, case.yr, fams, s2, dtype, case.dr, split)
    assert np.all(fresh.info() == 0)
    _compare(model, fresh, case, fams, s2, dtype, before, split, name)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_the_cap_the_band_edge_and_one_row_beyond_each(dtype):
    """300 -> 268 -> 257: as many rows as one call takes, then down to 128 (nt - 1) + 1; 33 rows at once are refused with -5,
    a 44th row with -4, and at the edge any row is"""
    rng = np.random.default_rng(1970)
    s2, fams = [RC.SIGMA2[dtype]], ["spline34"]
    X = RC.rnd(rng.uniform(-1.5 * (300 / 64.0) ** 0.5, 1.5 * (300 / 64.0) ** 0.5, (300, 2)), dtype)
    y = RC.target(X)
    model = _fit([X], [y], fams, s2, dtype)
    before = _state(model)
    h0 = _hash(model)
    with pytest.raises(ValueError, match="33 rows of patch 0 in one call, the limit is 32"):
        model.remove([np.arange(33)])
    rc, msg = _raw(model, [0] * 33, np.arange(33))
    assert rc == -5 and "33 rows of patch 0 in one call, the limit is PMK_REMOVE_MAX_ROWS = 32" in msg, (rc, msg)
    rc, msg = _raw(model, [0] * 44, np.arange(44))
    assert rc == -4 and "patch 0 has 43 removable rows (n = 300, nt = 3: at least 257 rows stay), 44 rows asked for" in msg, (rc, msg)
    assert _hash(model) == h0
    first = np.sort(rng.choice(300, 32, replace=False))
    assert np.all(model.remove([first]) == 0) and model.n[0] == 268 and model.removable()[0] == 11
    keep1 = np.setdiff1d(np.arange(300), first)
    second = np.sort(rng.choice(268, 11, replace=False))
    assert np.all(model.remove([second]) == 0) and model.n[0] == 257 and model.removable()[0] == 0
    keep = keep1[np.setdiff1d(np.arange(268), second)]
    h1 = _hash(model)
    rc, msg = _raw(model, [0], [256])
    assert rc == -4 and "patch 0 has 0 removable rows (n = 257, nt = 3: at least 257 rows stay), 1 rows asked for" in msg, (rc, msg)
    assert _hash(model) == h1
    # the two calls against the oracle and a fresh model of the 257 points; the bit claims of the first test hold for the
    # rows before the first row that ever left
    case = types.SimpleNamespace(P=1, Xs=[X], ys=[y], ds=None, dr=None, Xr=[np.ascontiguousarray(X[keep])], yr=[y[keep]],
                                 rows=[np.setdiff1d(np.arange(300), keep)], keep=[keep])
    fresh = _fit(case.Xr, case.yr, fams, s2, dtype)
    _compare(model, fresh, case, fams, s2, dtype, before, False, "band_edge")


# ------------------------------------------------------------------------------------------ consumers of the padding
def test_consumers_of_the_padding_agree_with_a_fresh_model():
    """evidence, loo + loo_values, queryinner with its variance, the multi-output solve with a linear trend and the item
    covariances of eight queries, on the model after the removal and on the fresh model of the reduced sets: a stale row
    in a live 32-row pair shows here.  The scores within the tolerances of _check_scores of tests/test_gpu_append.py
    (asserted by the first test on every case); here the items:
    means        c' of both models is within 10 e of the oracle (the first test), so two means differ by at most
                 sum_k |kq_k| 20 e plus 2 (n + 32) u sum_k |kq_k c_k| of their own sums (tests/test_gpu_grad.py)
    variances and covariance blocks of BOTH models within 10 units (n + 32) u kappa2(L) (k0 + |V_a| |V_b|) of the
                 long-double reference of tests/_cov_refs.py, the bound of tests/test_gpu_cov.py
    trend        the figures and bounds of tests/test_gpu_trend.py, through _trend_ratios of tests/test_gpu_append_after.py"""
    dtype, u = "f64", RR.U_OF["f64"]
    case, fams, s2 = {n: (c, f, s) for n, c, f, s in RC.all_cases(dtype)}["consumers"]
    (th, oth), P = RC.FAMILIES["spline34"], case.P
    model = _fit(case.Xs, case.ys, fams, s2, dtype)
    assert np.all(model.remove(case.rows) == 0)
    fresh = _fit(case.Xr, case.yr, fams, s2, dtype)
    full, red = _oracles(case, fams, s2)
    rng = np.random.default_rng(1990)
    root, _, _ = pmk.setuppartition(rng.uniform(-4, 4, (64, 2)), 4)                 # any tree of 8 leaves: the items name their regions
    worst = dict(mean=0.0, var=0.0, cov=0.0)
    for mdl in (model, fresh):
        mdl.set_bsp(root, 0)
    for r in range(P):
        n1 = len(case.Xr[r])
        # eight queries: at the rows that took the place of removed ones, at the last rows, and near them
        at = np.unique(np.clip(np.concatenate([case.rows[r][:3], [n1 - 1, n1 - 2, 0]]), 0, n1 - 1))
        near = case.Xr[r][rng.integers(n1, size=8 - len(at))] + rng.uniform(-0.2, 0.2, (8 - len(at), 2))
        xq = np.ascontiguousarray(np.vstack([case.Xr[r][at], near]))
        cref = CR.RegionRef(oth, case.Xr[r], s2[r])
        out = cref.cov(xq)
        assert not out["clamped"].any()
        unit = (n1 + 32) * u * out["unit"]
        e = RR.unit(len(case.Xs[r]), dtype, full[r]["kappa"], full[r]["L"])
        kq = np.abs(O.cross_kernel_matrix(oth, xq, case.Xr[r]))
        bmean = kq.sum(1) * 2 * RATIO_MAX * e + 2 * (n1 + 32) * u * (kq * np.abs(red[r]["c_chol"])[None, :]).sum(1)
        (mu_a, var_a), (mu_f, var_f) = model.queryinner(r, th, xq), fresh.queryinner(r, th, xq)
        worst["mean"] = max(worst["mean"], float((np.abs(mu_a - mu_f) / bmean).max()))
        region = np.full(8, r, dtype=np.int32)
        for mdl, var in ((model, var_a), (fresh, var_f)):
            q = TA._explicit_query(mdl, xq, region)
            q.items_cov()
            idx, S = q.item_covs(r)
            assert np.array_equal(idx, np.arange(8))
            worst["cov"] = max(worst["cov"], TA._worst_ratio(np.abs(np.asarray(S, dtype=RR.LD) - out["S"]).astype(np.float64), unit))
            worst["var"] = max(worst["var"], TA._worst_ratio(np.abs(var.astype(RR.LD) - np.diag(out["S"])).astype(np.float64),
                                                             np.diag(unit).copy()))
    print("REMOVE_CONSUMERS items", worst)
    assert worst["mean"] <= 1.0 and worst["var"] <= RATIO_MAX and worst["cov"] <= RATIO_MAX, worst
    # ---- the multi-output solve with a linear trend
    Yr = [np.stack([RC.target(x), 0.5 * x[:, 1] - 0.2 * x[:, 0] ** 2], 1) for x in case.Xr]
    region = np.sort(np.arange(16) % P).astype(np.int32)
    xq = np.vstack([case.Xr[r][rng.integers(len(case.Xr[r]))] + rng.uniform(-0.3, 0.3, 2) for r in region])
    refs = []
    for r in range(P):
        X, Y = case.Xr[r], Yr[r]
        K, H = O.kernel_matrix(oth, X), T.basis(X, "linear")
        x = xq[region == r]
        Kq, kqq, Hq = O.cross_kernel_matrix(oth, x, X), np.full(len(x), O.profile(oth, 0.0)), T.basis(x, "linear")
        ld, f = T.trend_reference(K, s2[r], Y, H), T.gls_fp64(K, s2[r], Y, H)
        refs.append(dict(ld=ld, f64=f, pred_ld=T.predict_reference(ld, Kq, kqq, Hq), pred_f64=T.predict_fp64(f, Kq, kqq, Hq),
                         kappa=TAA.kappa(K + s2[r] * np.eye(len(K)))))
    shim = types.SimpleNamespace(sizes=case.sizes, Xe=case.Xr)
    with pytest.raises(pmk.PmkError, match="no multi-output targets"):
        model.solve_multi()
    for name, mdl in (("removed", model), ("fresh", fresh)):
        mdl.set_targets_multi(Yr)
        mdl.set_trend("linear")
        mdl.solve_multi()
        w, failures = TAA._trend_ratios(mdl, shim, Yr, xq, region, refs, root)
        print("REMOVE_CONSUMERS trend", name, {k: round(v, 4) for k, v in w.items()})
        assert not failures, (name, failures)
    for r in range(P):
        assert np.array_equal(TAA._packed_multi(model, r), TAA._packed_multi(fresh, r)), r


# ------------------------------------------------------------------------------------------ the leave-one-out made real
def _queryinner_unclamped(model, r, th, xq):
    xq = np.ascontiguousarray(xq, dtype=np.float64)
    mu, var = np.empty(len(xq)), np.empty(len(xq))
    d = th.desc()
    _lib.check(model.ctx.L.pmk_model_queryinner_ex(model.h, r, C.byref(d), len(xq), M._d(xq), -np.inf, M._d(mu), M._d(var)),
               "pmk_model_queryinner_ex")
    return mu, var


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_the_leave_one_out_value_is_the_prediction_after_the_removal(dtype):
    """loo_values of the full factor, then row i really removed and the model queried at x_i: the mean is y_i - res_i and
    the variance plus sigma2 is var_i, each a device result within the unit and bound of tests/test_gpu_model_selection.py
    (cond_2 u max |y| in the residual, cond_2 u relative in d = 1 / var; cond_2 takes the + 32 of _check_scores), so the two
    differ by at most twice that.  i in the first row, the last row and on both sides of a tile edge."""
    rng = np.random.default_rng(1980)
    (th, oth), s2, u, n = RC.FAMILIES["spline34"], RC.SIGMA2[dtype], RR.U_OF[dtype], 300
    half = 1.5 * (n / 64.0) ** 0.5
    X = RC.rnd(rng.uniform(-half, half, (n, 2)), dtype)
    y = RC.target(X)
    cond = RR.kappa_of(O.kernel_matrix(oth, X) + s2 * np.eye(n)) ** 2
    worst = dict(mean=0.0, var=0.0)
    for i in (0, 127, 128, n - 1):
        model = _fit([X], [y], ["spline34"], [s2], dtype)
        model.loo()
        res, var = model.loo_values()
        assert np.all(model.remove([[i]]) == 0)
        mu, v = _queryinner_unclamped(model, 0, th, X[i:i + 1])
        rm = abs(mu[0] - (y[i] - res[0][i])) / (2 * (cond + 32) * u * np.abs(y).max())
        rv = abs(v[0] + s2 - var[0][i]) / (2 * (cond + 32) * u * var[0][i])
        print("REMOVE_LOO", dtype, i, dict(mean=rm, var=rv, cond=cond))
        worst = dict(mean=max(worst["mean"], rm), var=max(worst["var"], rv))
    assert worst["mean"] <= 1.0 and worst["var"] <= 1.0, worst


def test_remove_global_against_the_blended_leave_one_out():
    """from_tree with overlapping eps-sets: loomixtureGP_blend before, remove_global([j]) for a j of at least two patches,
    the blended predictor at x_j after.  Both are device results within cond_2 u max |y| (means) and cond_2 u (k(0) + sigma2)
    (variances) of the refit, the unit and bound of tests/test_gpu_loo_blend.py: they differ by at most twice that."""
    t = AC.Tree("f64")
    (th, oth), s2, u = AC.FAMILIES["spline34"], AC.SIGMA2["f64"], RR.U_OF["f64"]
    eta = pmk.MixtureGPType.from_tree(t.root, t.X, t.EPS)
    pmk.fitmixtureGP_(eta, t.y, th, s2)
    model = eta._model
    off0, inds0 = (a.copy() for a in model.patch_index())
    counts = np.bincount(inds0, minlength=len(t.X))
    j = int(np.nonzero(counts >= 2)[0][0])
    cond = max(np.linalg.cond(O.kernel_matrix(oth, x) + s2 * np.eye(len(x))) for x in eta.X_parts)
    Yl, Vl = pmk.loomixtureGP_blend(eta, t.root, t.RADIUS, t.DELTA, t.wth)
    q = M.DeviceQuery(model, t.X)
    total0 = q.plan(t.RADIUS, t.DELTA)
    nm0, ns0 = q.items_loo(False)
    with pytest.raises(pmk.PmkError, match="remove: a model built by from_tree takes remove_global"):
        model.remove([[0]] + [[]] * (model.P - 1))
    pmk.removemixtureGP_(eta, [j])
    assert model.N == len(t.X) and model.n.sum() == off0[-1] - counts[j]
    off1, inds1 = model.patch_index()
    model._index = None
    off2, inds2 = model.patch_index()                                           # the cached index is the library's
    assert np.array_equal(off1, off2) and np.array_equal(inds1, inds2)
    assert j not in inds1
    for r in range(model.P):
        want = inds0[off0[r]:off0[r + 1]]
        assert np.array_equal(inds1[off1[r]:off1[r + 1]], want[want != j]), r
        assert np.array_equal(eta.X_parts[r], t.X[want[want != j]]), r
        assert np.array_equal(eta.c_set[r], model.get(r, M.GET_C)), r
    Ya, Va, _ = pmk.querymixtureGP_patches(t.X[j:j + 1], eta, t.root, t.LEVELS, t.RADIUS, t.DELTA, t.wth)
    ry = abs(Ya[0] - Yl[j]) / (2 * cond * u * np.abs(t.y).max())
    rv = abs(Va[0] - Vl[j]) / (2 * cond * u * (O.profile(oth, 0.0) + s2))
    print("REMOVE_BLEND", dict(j=j, patches=int(counts[j]), dY=ry, dV=rv, cond=cond))
    assert ry <= 1.0 and rv <= 1.0, (ry, rv)
    # the leave-one-out items over the N training points: j is a member of no patch any more
    model.loo()
    q = M.DeviceQuery(model, t.X)
    assert q.plan(t.RADIUS, t.DELTA) == total0
    nm1, ns1 = q.items_loo(False)
    assert (nm1, ns1) == (nm0 - counts[j], ns0 + counts[j])
    # the *_global setters still take N values
    with pytest.raises(ValueError):
        model.set_targets_global(t.y[:-1])
    model.set_targets_global(t.y)
    with pytest.raises(pmk.PmkError, match="remove_global: the model was built from lists of patches"):
        _fit([t.X[:40]], [t.y[:40]], ["spline34"], [s2], "f64").remove_global([0])
    model.fit(th, s2)
    with pytest.raises(ValueError, match="no patch holds the global point %d" % j):
        model.remove_global([j])


# ------------------------------------------------------------------------------------------ a sliding window
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_sliding_window_of_200_points(dtype):
    """three rounds of "append 4, remove the 4 oldest" (then one of "remove 4, append 4"): n is 200 after every round, L
    and c within 10 units of the oracle on the current set, and a fit then equals the fresh model's bit for bit"""
    rng = np.random.default_rng(2000)
    (th, oth), s2 = RC.FAMILIES["spline34"], RC.SIGMA2[dtype]
    half = 1.5 * (216 / 64.0) ** 0.5
    X = RC.rnd(rng.uniform(-half, half, (216, 2)), dtype)
    y = RC.target(X)
    model = _fit([X[:200]], [y[:200]], ["spline34"], [s2], dtype)
    for k in range(3):
        new = slice(200 + 4 * k, 204 + 4 * k)
        assert np.all(model.append([X[new]], [y[new]]) == 0) and model.n[0] == 204
        assert np.all(model.remove([np.arange(4)]) == 0) and model.n[0] == 200
    assert np.all(model.remove([np.arange(4)]) == 0) and model.n[0] == 196          # append after remove
    assert np.all(model.append([X[212:216]], [y[212:216]]) == 0) and model.n[0] == 200
    cur = slice(16, 216)
    assert np.array_equal(model.X[0], X[cur])
    fit = _oracle_fit(oth, X[cur], y[cur], s2)
    e = RR.unit(204, dtype, fit["kappa"], fit["L"])
    fresh = _fit([X[cur]], [y[cur]], ["spline34"], [s2], dtype)
    got = dict(L=RR.ratio(model.get(0, M.GET_L), fit["L"], e), c=RR.ratio(model.get(0, M.GET_C), fit["c_chol"], e),
               L_fresh=RR.ratio(fresh.get(0, M.GET_L), fit["L"], e), c_fresh=RR.ratio(fresh.get(0, M.GET_C), fit["c_chol"], e))
    _record(case="window", dtype=dtype, kappa=fit["kappa"], **got)
    assert got["L"] <= RATIO_MAX and got["c"] <= RATIO_MAX, got
    for what in (0, 1):
        assert np.array_equal(_packed(model, 0, what), _packed(fresh, 0, what)), what
    model.fit(th, s2)
    for a, b in zip(_state(model)[0], _state(fresh)[0]):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------ state and refusals
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_failed_patch_takes_the_removal_and_stays_failed(dtype):
    """the duplicate-point construction of tests/test_gpu_append.py fails patch 1 at its appended row 35; the removal then
    takes its points, targets and n, keeps it failed (info names a leading minor, so 35 becomes n' = 33) and touches no
    other patch"""
    rng = np.random.default_rng(77)
    th = RC.FAMILIES["spline34"][0]
    Xs = [RC.rnd(rng.uniform(-10, 10, (n, 2)), dtype) for n in (20, 33, 12, 15)]
    ys = [RC.target(x) for x in Xs]
    model, _, info = M.fit_patches(Xs, ys, th, 0.0, dtype=dtype)
    assert np.all(info == 0)
    Xn = [np.zeros((0, 2)), np.vstack([RC.rnd(rng.uniform(-6, 6, (1, 2)), dtype), Xs[1][:1]]), np.zeros((0, 2)), np.zeros((0, 2))]
    info = model.append(Xn, [RC.target(x) for x in Xn])
    assert np.array_equal(info, [0, 35, 0, 0])
    h_others = [[a.copy() for a in s] for s in _state(model)]
    info = model.remove([[], [3, 34], [], []])
    assert np.array_equal(info, [0, 33, 0, 0]) and np.array_equal(model.n, [20, 33, 12, 15])
    # failed as after a failed fit: what reads info is NaN for it and for no other patch
    logdet, _ = model.evidence()
    assert np.isnan(logdet[1]) and np.all(np.isfinite(np.delete(logdet, 1)))
    for r in (0, 2, 3):
        assert all(np.array_equal(a, b) for a, b in zip(_state(model)[r], h_others[r])), r
    X1 = np.delete(np.vstack([Xs[1], Xn[1]]), [3, 34], axis=0)
    assert np.array_equal(model.X[1], X1)
    model.fit(th, 0.05)
    assert np.all(model.info() == 0)
    y1 = np.delete(np.concatenate([ys[1], RC.target(Xn[1])]), [3, 34])
    fresh = M.DeviceModel([Xs[0], X1, Xs[2], Xs[3]], [ys[0], y1, ys[2], ys[3]], dtype=dtype)
    fresh.fit(th, 0.05)
    for r in range(4):
        assert np.array_equal(model.get(r, M.GET_L), fresh.get(r, M.GET_L)), r
        assert np.array_equal(model.get(r, M.GET_C), fresh.get(r, M.GET_C)), r


def _raw(model, patch, row, n_items=None, null=False):
    L = model.ctx.L
    patch = np.ascontiguousarray(patch, dtype=np.int32)
    row = np.ascontiguousarray(row, dtype=np.int64)
    rc = L.pmk_model_remove(model.h, len(row) if n_items is None else n_items,
                            None if null else patch.ctypes.data_as(C.POINTER(C.c_int32)), None if null else M._i(row))
    return rc, L.pmk_last_error().decode()


def test_refusals_keep_the_model_and_name_the_cause():
    rng = np.random.default_rng(5)
    th, s2 = RC.FAMILIES["spline34"][0], 1e-2
    Xs = [rng.uniform(-3, 3, (n, 2)) for n in (30, 129, 60)]
    ys = [RC.target(x) for x in Xs]
    model = M.DeviceModel(Xs, ys)
    rc, msg = _raw(model, [0], [0])
    assert rc == -1 and "the model is not fitted" in msg, (rc, msg)
    with pytest.raises(pmk.PmkError, match="no factor"):
        model.remove([[0], [], []])
    model.fit(th, s2)
    h0 = _hash(model)
    cases = [
        (_raw(model, [3], [0]), -3, "item 0 names patch 3, outside 0 .. 2"),
        (_raw(model, [-1], [0]), -3, "names patch -1"),
        (_raw(model, [0, 0], [4, 30]), -3, "item 1 names row 30 of patch 0, outside 0 .. 29"),
        (_raw(model, [2], [-1]), -3, "item 0 names row -1 of patch 2"),
        (_raw(model, [0, 2, 0], [7, 7, 7]), -3, "item 2 gives row 7 of patch 0 a second time (first: item 0)"),
        (_raw(model, [1], [5]), -4, "patch 1 has 0 removable rows (n = 129, nt = 2: at least 129 rows stay), 1 rows asked for"),
        (_raw(model, [0] * 30, np.arange(30)), -4, "patch 0 has 29 removable rows (n = 30, nt = 1: at least 1 rows stay), 30 rows asked for"),
        (_raw(model, [2] * 33, np.arange(33)), -5, "33 rows of patch 2 in one call, the limit is PMK_REMOVE_MAX_ROWS = 32"),
        (_raw(model, [0], [0], null=True), -2, "NULL patches or rows"),
        (_raw(model, [0], [0], n_items=-1), -2, "n_items = -1"),
    ]
    for (rc, msg), want, text in cases:
        assert rc == want and text in msg, (rc, msg, text)
    assert _hash(model) == h0
    with pytest.raises(ValueError, match="patch 1 has 0 removable rows"):
        model.remove([[], [0], []])
    # nothing to remove
    assert _raw(model, [0], [0], n_items=0)[0] == 0
    assert np.all(model.remove([[], [], []]) == 0)
    assert _hash(model) == h0 and np.array_equal(model.n, [30, 129, 60])
    # a model of factors holds no targets
    loaded = M.DeviceModel.from_factors(Xs, [model.get(r, M.GET_C) for r in range(3)], [model.get(r, M.GET_L) for r in range(3)])
    loaded.set_kernels([th] * 3)
    rc, msg = _raw(loaded, [0], [0])
    assert rc == -1 and "holds no targets" in msg, (rc, msg)
    with pytest.raises(pmk.PmkError, match="holds no targets"):
        loaded.remove([[0], [], []])
    # the front end: removemixtureGP_ on lists of patches, zero-based rows
    eta = pmk.MixtureGPType(Xs, [])
    pmk.fitmixtureGP_(eta, ys, th, s2)
    pmk.removemixtureGP_(eta, [[0, 29], [], [59]])
    assert [len(x) for x in eta.X_parts] == [28, 129, 59] and np.array_equal(eta.X_parts[0], Xs[0][1:29])
    assert all(np.array_equal(eta.c_set[r], eta._model.get(r, M.GET_C)) for r in range(3))
    assert eta.L_set[0].shape == (28, 28)


def test_multi_output_state_is_discarded():
    rng = np.random.default_rng(6)
    th, s2 = RC.FAMILIES["spline34"][0], 1e-2
    Xs = [rng.uniform(-3, 3, (n, 2)) for n in (30, 132)]
    Ys = [np.stack([RC.target(x), x[:, 1]], 1) for x in Xs]
    model = M.DeviceModel(Xs, [y[:, 0].copy() for y in Ys])
    model.fit(th, s2)
    model.set_targets_multi(Ys)
    model.solve_multi()
    model.loo()
    rows = [np.array([0, 7]), np.array([131])]
    assert np.all(model.remove(rows) == 0)
    with pytest.raises(pmk.PmkError, match="no multi-output targets"):
        model.solve_multi()
    with pytest.raises(pmk.PmkError, match="loo\\(\\) has not run"):
        model.loo_values()
    Yr = [np.delete(y, r, axis=0) for y, r in zip(Ys, rows)]
    model.set_targets_multi(Yr)
    model.solve_multi()
    Cs = model.weights_multi()
    for r in range(2):
        c = model.get(r, M.GET_C)
        assert Cs[r].shape == (len(Yr[r]), 2)
        assert np.abs(Cs[r][:, 0] - c).max() <= 1e-9 * max(1.0, np.abs(c).max()), r
