"""Appending observations to a fitted model in place on the GPU (pmk_model_append / pmk_model_capacity, the kernel of
pmk_append.hip; DeviceModel.append / append_global, appendmixtureGP_).

References: the oracle on the extended point set, and a fresh DeviceModel of the extended lists (the fit, which the
append does not touch).  The inputs are those of tests/_append_cases.py, of which tests/test_append_refs.py asserts
kappa2(L') <= 10^3 and that the long-double border stays within one unit of the oracle.

Accuracy.  L' (all rows) and c' against the oracle in units
    e = (n + m + 32) u kappa2(L') max |L'|,   u = 2^-53 (fp64) or 2^-24 (fp32),
bound 10 units: the bound tests/test_gpu_cov.py gives the sweep that computes L21 here, for the same reason (a plain
LAPACK evaluation stays below one unit, tests/test_append_refs.py).  The fresh device fit's own ratio is measured on the
same inputs; both go to profiles/append_accuracy.json when the whole module runs ("APPEND {json}" with -s).

Scores after the append against the fresh model's, with cond = kappa2(L')^2: tests/test_gpu_model_selection.py holds each
device result within cond u of the truth in d = 1 / var and cond u max |y| in the residuals on patches of n >= 128, so two
device results differ by at most twice that; the patches here go down to two points, where the handful of roundings of
the evaluation itself is not covered by cond = 1.2, so cond takes the + 32 that the error unit above adds to n for the
same roundings.  log det within 2 n cond 10^-14 (scaled by u / 2^-53), y^T c within 2 n cond u max |y| max |c|.

z has no accessor: its old rows are covered by the bit checks of a later fit and by c', its new rows by c'.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
from patchmixturekriging_amd import mixture as M
from oracle import oracle as O
import _append_cases as AC
import _append_refs as AR
import _cov_refs as CR
import _grad_refs as GR
import _vgrad_refs as VR
from test_gpu_grad import _explicit_query, _worst_ratio

pytestmark = pytest.mark.gpu

RATIO_MAX = AC.RATIO_MAX
_RECORDS = []
ACCURACY_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "append_accuracy.json")
CASE_NAMES = [name for name, _, _, _ in AC.all_cases("f64")]


def _record(**kw):
    _RECORDS.append(kw)
    print("APPEND " + json.dumps(kw, sort_keys=True))


@pytest.fixture(scope="module", autouse=True)
def _write_accuracy_file():
    """only a run of the whole module replaces the file"""
    yield
    if {(r["case"], r["dtype"]) for r in _RECORDS} >= {(n, d) for n in CASE_NAMES for d in ("f64", "f32")}:
        with open(ACCURACY_JSON, "w") as f:
            f.write("[\n" + ",\n".join(" " + json.dumps(r, sort_keys=True) for r in _RECORDS) + "\n]\n")


def _fit(Xs, ys, fams, s2, dtype, ds=None, split=False):
    model = M.DeviceModel(Xs, ys, dtype=dtype)
    if split:
        assert model.ctx.L.pmk_test_model_set_split(model.h, 1) == 0
    if ds is not None:
        model.set_diag(ds)
    _refit(model, fams, s2)
    return model


def _refit(model, fams, s2):
    if len(set(fams)) == 1 and len(set(s2)) == 1:
        model.fit(AC.FAMILIES[fams[0]][0], s2[0])
    else:
        model.fit_patches([AC.FAMILIES[f][0] for f in fams], s2)


def _packed(model, r, what):
    L = model.ctx.L
    ld = C.c_int64()
    _lib.check(L.pmk_test_model_packed(model.h, r, what, C.byref(ld), None), "pmk_test_model_packed")
    out = np.empty(ld.value * (model.D if what == 0 else 1))
    _lib.check(L.pmk_test_model_packed(model.h, r, what, C.byref(ld), M._d(out)), "pmk_test_model_packed")
    return out


def _state(model):
    return [(model.get(r, M.GET_L), model.get(r, M.GET_C), model.get(r, M.GET_LINV_DIAG)) for r in range(model.P)]


def _hash(model):
    h = hashlib.sha256()
    for L, c, inv in _state(model):
        h.update(L.tobytes()); h.update(c.tobytes()); h.update(inv.tobytes())
    h.update(model.info().tobytes())
    return h.hexdigest()


def _oracle(case, fams, s2):
    """per patch: the oracle's fit of the extended set, kappa2(L') and the unit without u"""
    out = []
    for r in range(case.P):
        oth = AC.FAMILIES[fams[r]][1]
        fit = O.fit_patch(oth, case.Xe[r], case.ye[r], s2[r], want_K=True, diag=None if case.de is None else case.de[r])
        assert fit["info"] == 0
        U = fit["K"].copy()
        U[np.diag_indices(len(U))] += s2[r]
        fit["kappa"] = AR.kappa_of(U)
        out.append(fit)
    return out


def _append(model, case):
    return model.append(case.Xn, case.yn, case.dn)


def _check_scores(model, fresh, refs, case, dtype):
    u = AR.U_OF[dtype]
    ld_a, q_a = model.evidence()
    ld_f, q_f = fresh.evidence()
    model.loo(); fresh.loo()
    (res_a, var_a), (res_f, var_f) = model.loo_values(), fresh.loo_values()
    for r in range(case.P):
        n, cond, ymax = len(case.ye[r]), refs[r]["kappa"] ** 2, np.abs(case.ye[r]).max()
        cmax = np.abs(refs[r]["c_chol"]).max()
        assert abs(ld_a[r] - ld_f[r]) <= 2 * n * cond * 1e-14 * (u / 2.0 ** -53), (r, ld_a[r], ld_f[r])
        assert abs(q_a[r] - q_f[r]) <= 2 * n * cond * u * ymax * cmax, (r, q_a[r], q_f[r])
        assert np.all(np.abs(var_a[r] - var_f[r]) <= 2 * (cond + 32) * u * var_f[r]), r
        assert np.all(np.abs(res_a[r] - res_f[r]) <= 2 * (cond + 32) * u * ymax), r


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_append_against_the_oracle_and_a_fresh_model(name, dtype):
    case, fams, s2 = {n: (c, f, s) for n, c, f, s in AC.all_cases(dtype)}[name]
    split = name == "split"
    model = _fit(case.Xs, case.ys, fams, s2, dtype, case.ds, split)
    assert np.all(model.info() == 0)
    free = model.capacity()
    assert np.array_equal(free, [128 * ((n + 127) // 128) - n for n, _ in case.sizes])
    before = _state(model)
    model.loo()                                  # the leave-one-out tasks and d of the old factor exist: d goes stale
    info = _append(model, case)
    assert np.all(info == 0), info
    with pytest.raises(pmk.PmkError, match="loo\\(\\) has not run"):
        model.loo_values()
    assert np.array_equal(model.n, [n + m for n, m in case.sizes])
    assert np.array_equal(model.capacity(), free - np.array([m for _, m in case.sizes]))
    after = _state(model)
    fresh = _fit(case.Xe, case.ye, fams, s2, dtype, case.de, split)
    assert np.all(fresh.info() == 0)
    fstate = _state(fresh)
    refs = _oracle(case, fams, s2)
    worst = dict(L=0.0, c=0.0, L_fresh=0.0, c_fresh=0.0, kappa=0.0)
    for r, (n, m) in enumerate(case.sizes):
        (L0, c0, inv0), (L1, c1, inv1) = before[r], after[r]
        # ---- bits: the old rows and columns of L and the -D^-1 blocks that do not meet the new rows
        assert L1.shape == (n + m, n + m)
        assert np.array_equal(L1[:n, :n], L0), r
        assert np.array_equal(L1[:n, n:], np.zeros((n, m))), r
        touched = set(range(n // 32, (n + m - 1) // 32 + 1)) if m else set()
        for b in range(inv0.shape[0]):
            if b not in touched:
                assert np.array_equal(inv1[b], inv0[b]), (r, b)
            else:
                # a recomputed block against the fresh fit's: each device L' is within 10 e of the oracle entry by entry, so
                # the 32 x 32 blocks L_ss differ by dL, |dL|_F <= 32 * 20 e, and N = -L_ss^-1 moves by N dL N to first order:
                # |dN| <= |N|_2^2 |dL|_F; each inversion adds its own 32 u |N|_2^2 |L_ss|_2 at most
                e = AR.unit(n + m, dtype, refs[r]["kappa"], refs[r]["L"])
                Lss = refs[r]["L"][32 * b:32 * b + 32, 32 * b:32 * b + 32]
                k = len(Lss)                                    # the last block of a patch may be cut by n + m
                N2 = np.linalg.norm(fstate[r][2][b][:k, :k], 2)
                tol = N2 ** 2 * (32 * 2 * RATIO_MAX * e + 2 * 32 * AR.U_OF[dtype] * np.linalg.norm(Lss, 2))
                assert np.abs(inv1[b] - fstate[r][2][b]).max() <= tol, (r, b, np.abs(inv1[b] - fstate[r][2][b]).max(), tol)
                assert np.array_equal(np.triu(inv1[b], 1), np.zeros((32, 32))), (r, b)
        if m == 0:
            assert np.array_equal(c1, c0) or split, r         # the split path forms z and c again for every patch
        # ---- bits: the packed buffers, padding included, and K
        for what in ((0, 1, 2) if case.ds is not None else (0, 1)):
            assert np.array_equal(_packed(model, r, what), _packed(fresh, r, what)), (r, what)
        assert np.array_equal(model.get(r, M.GET_K), fresh.get(r, M.GET_K)), r
        # ---- accuracy against the oracle, the fresh fit beside it
        e = AR.unit(n + m, dtype, refs[r]["kappa"], refs[r]["L"])
        got = dict(L=AR.ratio(L1, refs[r]["L"], e), c=AR.ratio(c1, refs[r]["c_chol"], e),
                   L_fresh=AR.ratio(fstate[r][0], refs[r]["L"], e), c_fresh=AR.ratio(fstate[r][1], refs[r]["c_chol"], e))
        print("APPEND_PATCH", name, dtype, r, n, m, {k: round(v, 4) for k, v in got.items()})
        for k, v in got.items():
            worst[k] = max(worst[k], v)
        worst["kappa"] = max(worst["kappa"], refs[r]["kappa"])
    _record(case=name, dtype=dtype, **worst)
    assert worst["kappa"] <= AC.KAPPA_MAX
    assert worst["L"] <= RATIO_MAX and worst["c"] <= RATIO_MAX, worst
    _check_scores(model, fresh, refs, case, dtype)
    # ---- a fit after the append is the fit of the fresh model, bit for bit: n, padding and host state are right
    _refit(model, fams, s2)
    assert np.array_equal(model.info(), fresh.info())
    for r, (L, c, inv) in enumerate(_state(model)):
        assert np.array_equal(L, fstate[r][0]) and np.array_equal(c, fstate[r][1]) and np.array_equal(inv, fstate[r][2]), r


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_three_appends_of_one_point_against_one_of_three(dtype):
    case, fams, s2 = {n: (c, f, s) for n, c, f, s in AC.all_cases(dtype)}["three"]
    one = _fit(case.Xs, case.ys, fams, s2, dtype)
    assert np.all(_append(one, case) == 0)
    three = _fit(case.Xs, case.ys, fams, s2, dtype)
    for k in range(3):
        assert np.all(three.append([x[k:k + 1] for x in case.Xn], [y[k:k + 1] for y in case.yn]) == 0)
    assert np.array_equal(three.n, one.n)
    refs = _oracle(case, fams, s2)
    for r, (n, m) in enumerate(case.sizes):
        for what in (0, 1):
            assert np.array_equal(_packed(three, r, what), _packed(one, r, what)), (r, what)
        e = AR.unit(n + m, dtype, refs[r]["kappa"], refs[r]["L"])
        for mdl in (one, three):
            assert AR.ratio(mdl.get(r, M.GET_L), refs[r]["L"], e) <= RATIO_MAX, r
            assert AR.ratio(mdl.get(r, M.GET_C), refs[r]["c_chol"], e) <= RATIO_MAX, r
        # the first new row is the same border of the same factor in both
        assert np.array_equal(three.get(r, M.GET_L)[n, :n + 1], one.get(r, M.GET_L)[n, :n + 1]), r


# ------------------------------------------------------------------------------------------ through the blend
def _blend_weights(off, t, plane, hp_v, owth, j):
    """w, S, wn, dw [m, D], dwn [m, D] of query j as pmk_query_mix_multi / _mix_grad / _mix_vgrad take them (items in the
    order of the mix, home last), in double"""
    it = np.arange(off[j], off[j + 1])
    tt = np.asarray(t, dtype=AR.LD)[it]
    w = GR.phi(owth, np.abs(tt))
    w[-1] = AR.LD(1)
    nv = np.zeros((len(it), hp_v.shape[1]), dtype=AR.LD)
    nv[:-1] = np.asarray(hp_v, dtype=AR.LD)[plane[it[:-1]]]
    dw = -(GR.psi(owth, np.abs(tt)) * tt)[:, None] * nv
    dw[-1] = AR.LD(0)
    S = w.sum()
    wn = w / S
    dwn = (dw - wn[:, None] * dw.sum(0)[None, :]) / S
    f = lambda a: np.asarray(a, dtype=np.float64)
    return it, f(w), float(S), f(wn), f(dw), f(dwn)


def test_append_global_through_the_blend():
    """The appended model against a from_tree model of the extended global array, through querymixtureGP_patches,
    querymixtureGP_cov and querymixtureGP_grad(..., variance=True).  Both models plan the same items with the same
    weights (same tree, same points), so two results differ by what their items differ, blended, plus the blend's own
    rounding; each bound is the sum of the two models' unit bounds, the units those calls' own tests use:

    covariance   every region block and the blended matrix of BOTH models within 10 units of the long-double reference of
                 tests/_cov_refs.py, as tests/test_gpu_cov.py holds them (units (n + 32) u kappa2(L) (k0 + |V_a| |V_b|))
    variances    an item's v within 10 (n + 32) u vunit and its gradient within 10 (n + 32) u unit_d of the truth
                 (tests/_vgrad_refs.py, the bound of tests/test_gpu_vgrad.py): twice that between the models
    means        c' of both models within 10 e of the oracle (asserted here; e of tests/_append_refs.py), so the weights
                 differ by dC <= 20 e and an item's mean by sum_k |kq_k| dC, its gradient by sum_k |g_k,d| dC, plus the
                 (n + 32) u sum_k |kq_k c_k| (resp. |g_k,d c_k|) of each model's own sum, the bound of tests/test_gpu_grad.py
    blend        Y = sum wn u, V = sum wn^2 v, dY = sum [w G + (u - Y) dw] / S, dV = sum [wn^2 GV + 2 wn v dwn] carry the item
                 bounds through their weights; their own rounding is 16 m u of the sum of their terms' magnitudes per model
                 (tests/test_gpu_grad.py, tests/test_gpu_vgrad.py)."""
    t = AC.Tree("f64")
    (th, oth), s2, u = AC.FAMILIES["spline34"], AC.SIGMA2["f64"], AR.U_OF["f64"]
    owth = O.kernel(O.SPLINE34, 1 / t.RADIUS)
    eta = pmk.MixtureGPType.from_tree(t.root, t.X, t.EPS)
    pmk.fitmixtureGP_(eta, t.y, th, s2)
    model = eta._model
    off0, inds0 = (a.copy() for a in model.patch_index())
    first = model.N
    # expected items from the oracle's assignment of the new points
    ob = O.BSP(t.X, t.LEVELS)
    ooff, oinds, oloff, olists = ob.assign(t.Xnew, t.EPS)
    mult = np.diff(oloff)
    assert (mult == 1).any() and (mult == 2).any() and (mult >= 3).any(), mult
    pmk.appendmixtureGP_(eta, t.Xnew, t.ynew)
    assert model.N == first + len(t.Xnew) and model.n.sum() == off0[-1] + mult.sum()
    off1, inds1 = model.patch_index()
    for r in range(model.P):
        want = np.concatenate([inds0[off0[r]:off0[r + 1]], first + oinds[ooff[r]:ooff[r + 1]]])
        assert np.array_equal(inds1[off1[r]:off1[r + 1]], want), r
        assert np.array_equal(eta.X_parts[r], t.Xall[want]), r
    eta2 = pmk.MixtureGPType.from_tree(t.root, t.Xall, t.EPS)
    pmk.fitmixtureGP_(eta2, t.yall, th, s2)
    fresh = eta2._model
    off2, inds2 = fresh.patch_index()
    assert np.array_equal(off1, off2) and np.array_equal(inds1, inds2)
    P, Xs = model.P, eta2.X_parts
    nr = [len(x) for x in Xs]
    dC, Cw, vrefs = [], [], []
    for r in range(P):
        fit = O.fit_patch(oth, Xs[r], t.yall[inds2[off2[r]:off2[r + 1]]], s2, want_K=True)
        kappa = AR.kappa_of(fit["K"] + s2 * np.eye(nr[r]))
        assert kappa <= AC.KAPPA_MAX
        e = AR.unit(nr[r], "f64", kappa, fit["L"])
        assert np.array_equal(eta.c_set[r], model.get(r, M.GET_C))
        for mdl in (model, fresh):
            assert AR.ratio(mdl.get(r, M.GET_C), fit["c_chol"], e) <= RATIO_MAX, r
            assert AR.ratio(mdl.get(r, M.GET_L), fit["L"], e) <= RATIO_MAX, r
        dC.append(2 * RATIO_MAX * e)
        Cw.append(np.abs(fresh.get(r, M.GET_C)))
        vrefs.append(VR.PatchRef(oth, Xs[r], s2))
    args = (t.root, t.LEVELS, t.RADIUS, t.DELTA)
    hp_v = pmk.partition.hyperplane_arrays(t.root)[0]

    # ---- the joint covariance: both models against the long-double reference, blocks and blend
    Ya, Va, Ca = pmk.querymixtureGP_cov(t.Xq, eta, *args, t.wth)
    Yf, Vf, Cf = pmk.querymixtureGP_cov(t.Xq, eta2, *args, t.wth)
    qa, qf = (M._cov_query(t.Xq, e_, t.root, t.RADIUS, t.DELTA, t.wth, "test") for e_ in (eta, eta2))
    assert np.array_equal(qa.fetch_cov(), Ca) and np.array_equal(qf.fetch_cov(), Cf)
    dbg = qf.debug()
    off, reg, tt = dbg["item_offsets"], dbg["item_region"], dbg["item_t"]
    assert np.array_equal(qa.debug()["item_region"], reg) and np.array_equal(qa.debug()["item_t"], tt)
    assert (np.diff(off) > 1).sum() >= 10                           # the workload exercises the blend
    S_ref, units, worst_block = {}, {}, 0.0
    for r in sorted(set(int(v) for v in reg)):
        cref = CR.RegionRef(oth, Xs[r], s2)
        for q in (qa, qf):
            idx, S = q.item_covs(r)
            out = cref.cov(t.Xq[idx])
            assert not out["clamped"].any()
            units[r] = (nr[r] + 32) * u * out["unit"]
            S_ref[r] = (idx.astype(np.int64), out["S"])
            worst_block = max(worst_block, _worst_ratio(np.abs(np.asarray(S, dtype=AR.LD) - out["S"]).astype(np.float64), units[r]))
    ref_cov, unit = CR.mix_cov_ref((off, reg), S_ref, tt, owth, units)
    worst_cov = max(_worst_ratio(np.abs(np.asarray(Cx, dtype=AR.LD) - ref_cov).astype(np.float64), unit) for Cx in (Ca, Cf))
    print("APPEND_BLEND cov", dict(blocks=worst_block, blend=worst_cov))
    assert worst_block <= RATIO_MAX and worst_cov <= RATIO_MAX, (worst_block, worst_cov)

    # ---- means and variances (single-output path) and, after the targets of all points are set again, the gradients
    Ya, Va, _ = pmk.querymixtureGP_patches(t.Xq, eta, *args, t.wth)
    Yf, Vf, _ = pmk.querymixtureGP_patches(t.Xq, eta2, *args, t.wth)
    with pytest.raises(pmk.PmkError, match="no multi-output targets"):
        model.solve_multi()
    model.set_targets_multi_global(t.yall)
    model.solve_multi()
    eta.C_set = model.weights_multi()
    pmk.fitmixtureGP_multi_(eta2, t.yall, th, s2)
    Yma, Vma, dYa, dVa = pmk.querymixtureGP_grad(t.Xq, eta, *args, th, s2, t.wth, variance=True)
    Ymf, Vmf, dYf, dVf = pmk.querymixtureGP_grad(t.Xq, eta2, *args, th, s2, t.wth, variance=True)
    q = M.DeviceQuery(fresh, t.Xq)                                  # the items of the fresh model: values for the magnitudes
    q.plan(t.RADIUS, t.DELTA)
    q.items_multi_fitted(True)
    q.items_grad()
    q.items_vgrad()
    Ui, vi = q.item_values_multi()
    Gi, plane = q.item_grads()
    GVi = q.item_vgrads()
    dbg = q.debug()
    off, reg, tt = dbg["item_offsets"], dbg["item_region"], dbg["item_t"]
    query_of = np.repeat(np.arange(len(t.Xq)), np.diff(off))
    D = 2
    du, dG, dv, dGV = np.zeros(len(reg)), np.zeros((len(reg), D)), np.zeros(len(reg)), np.zeros((len(reg), D))
    for r in range(P):
        sel = np.nonzero(reg == r)[0]
        if not len(sel):
            continue
        x = t.Xq[query_of[sel]]
        it = vrefs[r].items(x)
        assert not it["clamped"].any()
        kq, g = (np.abs(np.asarray(a, dtype=np.float64)) for a in vrefs[r].operands(x))         # n x m, n x m x D
        own = 2 * (nr[r] + 32) * u
        du[sel] = kq.sum(0) * dC[r] + own * (kq * Cw[r][:, None]).sum(0)
        dG[sel] = g.sum(0) * dC[r] + own * (g * Cw[r][:, None, None]).sum(0)
        dv[sel] = 2 * RATIO_MAX * (nr[r] + 32) * u * it["vunit"]
        dGV[sel] = 2 * RATIO_MAX * (nr[r] + 32) * u * it["unit"]
    worst = dict(Y=0.0, V=0.0, dY=0.0, dV=0.0)
    for j in range(len(t.Xq)):
        it, w, S, wn, dw, dwn = _blend_weights(off, tt, plane, hp_v, owth, j)
        rnd = 2 * 16 * len(it) * u
        bY = (wn * du[it]).sum() + rnd * (wn * np.abs(Ui[it, 0])).sum()
        bV = (wn ** 2 * dv[it]).sum() + rnd * (wn ** 2 * np.abs(vi[it])).sum()
        _, magY = GR.mix_grad_ref(it, Gi, Ui, tt, plane, hp_v, owth)
        _, magV = VR.mix_vgrad_ref(it, GVi, vi, tt, plane, hp_v, owth)
        bdY = (w[:, None] * dG[it] + (du[it] + bY)[:, None] * np.abs(dw)).sum(0) / S + rnd * np.asarray(magY[0], dtype=np.float64)
        bdV = ((wn ** 2)[:, None] * dGV[it] + 2 * (wn * dv[it])[:, None] * np.abs(dwn)).sum(0) + rnd * np.asarray(magV, dtype=np.float64)
        for key, err, bound in (("Y", [abs(Ya[j] - Yf[j]), abs(Yma[j, 0] - Ymf[j, 0])], bY),
                                ("V", [abs(Va[j] - Vf[j]), abs(Vma[j] - Vmf[j])], bV),
                                ("dY", np.abs(dYa[j, 0] - dYf[j, 0]), bdY), ("dV", np.abs(dVa[j] - dVf[j]), bdV)):
            worst[key] = max(worst[key], _worst_ratio(np.atleast_1d(np.asarray(err, dtype=np.float64)),
                                                      np.broadcast_to(bound, np.shape(np.atleast_1d(err))).astype(np.float64)))
    print("APPEND_BLEND items", worst)
    assert max(worst.values()) <= 1.0, worst
    # the *_global setters take the new N
    with pytest.raises(ValueError):
        model.set_targets_global(t.y)
    model.set_targets_global(t.yall)


def test_append_global_on_the_trees_own_leaves():
    """eps=None: the patches are the tree's leaves and a new point goes to its home leaf only"""
    rng = np.random.default_rng(31)
    th, s2 = AC.FAMILIES["spline34"][0], 1e-2
    X = rng.uniform(-3, 3, (200, 2))
    root, _, X_inds = pmk.setuppartition(X, 3)
    model = M.DeviceModel.from_tree(root, X, AC.target(X))
    model.fit(th, s2)
    off0, inds0 = (a.copy() for a in model.patch_index())
    assert all(np.array_equal(inds0[off0[r]:off0[r + 1]], X_inds[r]) for r in range(4))
    Xn = rng.uniform(-2.9, 2.9, (9, 2))
    home = np.array([O.BSP(X, 3).findpartition(x) for x in Xn])
    assert len(set(home)) >= 2
    assert model.append_global(Xn, AC.target(Xn)) == (200, 9)
    assert np.all(model.info() == 0) and model.N == 209
    off1, inds1 = model.patch_index()
    Xall, yall = np.vstack([X, Xn]), AC.target(np.vstack([X, Xn]))
    Xe, ye = [], []
    for r in range(4):
        want = np.concatenate([X_inds[r], 200 + np.nonzero(home == r)[0]])
        assert np.array_equal(inds1[off1[r]:off1[r + 1]], want), r
        assert np.array_equal(model.X[r], Xall[want]), r
        Xe.append(np.ascontiguousarray(Xall[want])); ye.append(yall[want])
    fresh = M.DeviceModel(Xe, ye)
    fresh.fit(th, s2)
    for r in range(4):
        assert np.array_equal(_packed(model, r, 0), _packed(fresh, r, 0)) and np.array_equal(_packed(model, r, 1), _packed(fresh, r, 1)), r
        fit = O.fit_patch(AC.FAMILIES["spline34"][1], Xe[r], ye[r], s2, want_K=True)
        e = AR.unit(len(ye[r]), "f64", AR.kappa_of(fit["K"] + s2 * np.eye(len(ye[r]))), fit["L"])
        for mdl in (model, fresh):
            assert AR.ratio(mdl.get(r, M.GET_C), fit["c_chol"], e) <= RATIO_MAX, r


# ------------------------------------------------------------------------------------------ failure and refusals
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_duplicate_point_without_noise_fails_its_patch_only(dtype):
    """the appended duplicate of a patch's FIRST training point at sigma2 = 0: L[0, 0] = 1 and L[j, 0] = K[j, 0] exactly,
    so V = (1, 0 ...) up to terms whose squares vanish beside 1, |V|^2 = 1 and the pivot k(0) - |V|^2 is exactly 0"""
    rng = np.random.default_rng(77)
    th = AC.FAMILIES["spline34"][0]
    Xs = [AC.rnd(rng.uniform(-10, 10, (n, 2)), dtype) for n in (20, 33, 12, 15)]
    ys = [AC.target(x) for x in Xs]
    eta = pmk.MixtureGPType(Xs, [])
    model, cs, info = M.fit_patches(Xs, ys, th, 0.0, dtype=dtype)       # fitmixtureGP_ in the precision under test
    assert np.all(info == 0)
    M._store_fit(eta, model, cs, [0.0] * 4)
    Xn = [AC.rnd(rng.uniform(-6, 6, (2, 2)), dtype), np.vstack([AC.rnd(rng.uniform(-6, 6, (1, 2)), dtype), Xs[1][:1]]),
          np.zeros((0, 2)), np.zeros((0, 2))]
    yn = [AC.target(x) for x in Xn]
    with pytest.raises(pmk.PosDefException) as ei:
        pmk.appendmixtureGP_(eta, Xn, yn)
    assert ei.value.patch == 1 and ei.value.info == 33 + 1 + 1
    assert np.array_equal(model.info(), [0, 35, 0, 0])
    assert np.array_equal(model.n, [22, 35, 12, 15]) and [len(x) for x in eta.X_parts] == [22, 35, 12, 15]
    # the patch is failed as after a failed fit: what reads info is NaN for it and for no other patch: the scores (as in
    # tests/test_gpu_patches.py) and an item stage, the covariance blocks of explicit items (as in tests/test_gpu_cov.py).
    # The plain item means never read info, after a failed fit either, and are not checked.
    logdet, quad = model.evidence()
    model.loo()
    res, var = model.loo_values()
    model.set_bsp(pmk.setuppartition(rng.uniform(-4, 4, (32, 2)), 3)[0], 0)        # any 4-leaf tree: the items name their regions
    region = np.repeat(np.arange(4, dtype=np.int32), 3)
    xq = np.vstack([x[:3] + 0.25 for x in model.X])
    q = _explicit_query(model, xq, region)
    q.items_cov()
    for r in range(4):
        idx, S = q.item_covs(r)
        assert np.array_equal(idx, np.nonzero(region == r)[0])
        assert np.all(np.isnan(S)) if r == 1 else np.all(np.isfinite(S)) and np.all(np.diag(S) > 0), (r, S)
    for r in range(4):
        nan = [np.isnan(logdet[r]), np.isnan(quad[r]), np.all(np.isnan(res[r])), np.all(np.isnan(var[r]))]
        fin = [np.isfinite(logdet[r]), np.isfinite(quad[r]), np.all(np.isfinite(res[r])), np.all(np.isfinite(var[r]))]
        assert all(nan) if r == 1 else all(fin), (r, nan, fin)
    # a failed patch takes points and stays failed
    info = model.append([np.zeros((0, 2)), AC.rnd(rng.uniform(-6, 6, (1, 2)), dtype), np.zeros((0, 2)), np.zeros((0, 2))],
                        [np.zeros(0), np.zeros(1), np.zeros(0), np.zeros(0)])
    assert np.array_equal(info, [0, 35, 0, 0]) and model.n[1] == 36
    model.fit(th, 0.05)
    assert np.all(model.info() == 0)
    fresh = M.DeviceModel(model.X, [np.concatenate([ys[0], yn[0]]), np.concatenate([ys[1], yn[1], np.zeros(1)]), ys[2], ys[3]],
                          dtype=dtype)
    fresh.fit(th, 0.05)
    for r in range(4):
        assert np.array_equal(model.get(r, M.GET_L), fresh.get(r, M.GET_L)), r
        assert np.array_equal(model.get(r, M.GET_C), fresh.get(r, M.GET_C)), r


def _raw(model, x, y, patch, diag=None, gidx=None, n_items=None):
    L = model.ctx.L
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    patch = np.ascontiguousarray(patch, dtype=np.int32)
    rc = L.pmk_model_append(model.h, len(y) if n_items is None else n_items, M._d(x), M._d(y),
                            None if diag is None else M._d(np.ascontiguousarray(diag, dtype=np.float64)),
                            patch.ctypes.data_as(C.POINTER(C.c_int32)),
                            None if gidx is None else M._i(np.ascontiguousarray(gidx, dtype=np.int64)))
    return rc, L.pmk_last_error().decode()


def test_refusals_keep_the_model_and_name_the_cause():
    rng = np.random.default_rng(5)
    th, s2 = AC.FAMILIES["spline34"][0], 1e-2
    Xs = [rng.uniform(-3, 3, (n, 2)) for n in (30, 128, 60)]
    ys = [AC.target(x) for x in Xs]
    model = M.DeviceModel(Xs, ys)
    x1, y1 = np.zeros((1, 2)), np.zeros(1)
    rc, msg = _raw(model, x1, y1, [0])
    assert rc == -1 and "the model is not fitted" in msg, (rc, msg)
    with pytest.raises(pmk.PmkError, match="no factor"):
        model.append([x1, x1[:0], x1[:0]], [y1, y1[:0], y1[:0]])
    model.fit(th, s2)
    h0 = _hash(model)
    cases = [
        (_raw(model, x1, y1, [3]), -3, "item 0 names patch 3, outside 0 .. 2"),
        (_raw(model, x1, y1, [-1]), -3, "names patch -1"),
        (_raw(model, x1, y1, [1]), -4, "patch 1 has 0 free rows (n = 128, ld = 128), 1 rows asked for"),
        (_raw(model, np.zeros((99, 2)), np.zeros(99), [0] * 99), -4, "patch 0 has 98 free rows (n = 30, ld = 128), 99 rows asked for"),
        (_raw(model, np.zeros((16385, 2)), np.zeros(16385), [0] * 16385), -5, "16385 items in one call, the limit is PMK_COV_MAX_QUERIES = 16384"),
        (_raw(model, [[np.nan, 0.0]], y1, [0]), -6, "item 0 has a non-finite coordinate, target or addend"),
        (_raw(model, x1, [np.inf], [0]), -6, "non-finite"),
        (_raw(model, x1, y1, [0], gidx=[500]), -2, "global_index must be NULL"),
        (_raw(model, x1, y1, [0], diag=[0.1]), -2, "the model holds no addends"),
    ]
    for (rc, msg), want, text in cases:
        assert rc == want and text in msg, (rc, msg, text)
    assert _hash(model) == h0
    with pytest.raises(ValueError, match="patch 1 has 0 free rows"):
        model.append([x1[:0], x1, x1[:0]], [y1[:0], y1, y1[:0]])
    # nothing to append
    assert _raw(model, x1, y1, [0], n_items=0)[0] == 0
    assert np.all(model.append([x1[:0]] * 3, [y1[:0]] * 3) == 0)
    assert _hash(model) == h0 and np.array_equal(model.n, [30, 128, 60])
    # a model of factors holds no targets
    loaded = M.DeviceModel.from_factors(Xs, [model.get(r, M.GET_C) for r in range(3)], [model.get(r, M.GET_L) for r in range(3)])
    loaded.set_kernels([th] * 3)
    rc, msg = _raw(loaded, x1, y1, [0])
    assert rc == -1 and "holds no targets" in msg, (rc, msg)
    with pytest.raises(pmk.PmkError, match="holds no targets"):
        loaded.append([x1, x1[:0], x1[:0]], [y1, y1[:0], y1[:0]])
    # a tree-built model needs the global indices
    X = rng.uniform(-3, 3, (300, 2))
    root, _, _ = pmk.setuppartition(X, 3)
    tree = M.DeviceModel.from_tree(root, X, AC.target(X), 0.2)
    tree.fit(th, s2)
    h1 = _hash(tree)
    rc, msg = _raw(tree, x1, y1, [0])
    assert rc == -2 and "global_index is required" in msg, (rc, msg)
    rc, msg = _raw(tree, x1, y1, [0], gidx=[-1])
    assert rc == -3 and "global index -1" in msg, (rc, msg)
    rc, msg = _raw(tree, x1, y1, [0], gidx=[299])
    assert rc == -3 and "has global index 299, outside N = 300" in msg, (rc, msg)
    rc, msg = _raw(tree, np.zeros((3, 2)), np.zeros(3), [0, 1, 0], gidx=[300, 300, 300])
    assert rc == -3 and "global index 300 is given twice for patch 0" in msg, (rc, msg)
    assert _hash(tree) == h1 and tree.N == 300


def test_multi_output_state_is_discarded():
    rng = np.random.default_rng(6)
    th, s2 = AC.FAMILIES["spline34"][0], 1e-2
    Xs = [rng.uniform(-3, 3, (n, 2)) for n in (30, 130)]
    Ys = [np.stack([AC.target(x), x[:, 1]], 1) for x in Xs]
    model = M.DeviceModel(Xs, [y[:, 0].copy() for y in Ys])
    model.fit(th, s2)
    model.set_targets_multi(Ys)
    model.solve_multi()
    Xn = [rng.uniform(-3, 3, (2, 2)), rng.uniform(-3, 3, (1, 2))]
    assert np.all(model.append(Xn, [AC.target(x) for x in Xn]) == 0)
    with pytest.raises(pmk.PmkError, match="no multi-output targets"):
        model.solve_multi()
    with pytest.raises(pmk.PmkError, match="loo\\(\\) has not run"):
        model.loo_values()
    Ye = [np.vstack([y, np.stack([AC.target(x), x[:, 1]], 1)]) for y, x in zip(Ys, Xn)]
    model.set_targets_multi(Ye)
    model.solve_multi()
    Cs = model.weights_multi()
    for r in range(2):
        c = model.get(r, M.GET_C)
        assert Cs[r].shape == (len(Ye[r]), 2)
        assert np.abs(Cs[r][:, 0] - c).max() <= 1e-9 * max(1.0, np.abs(c).max()), r
