"""Room to grow in a model on the GPU (pmk_model_reserve, the kernels of pmk_reserve.hip) and appends that enter the block
rows it lays out (pmk_model_append / append_border_kernel); DeviceModel.reserve, from_tree(reserve=), reservemixtureGP_.

Most checks are bit identities and carry no tolerance: a patch works on nt = ceil(n / 128) block rows whatever its stride,
so a reserved model must give the bits of an unreserved one, and a reserve must move a fitted model's content and
nothing else.  The inputs are those of tests/_reserve_cases.py; tests/test_reserve_refs.py asserts on the CPU that every
extended set is positive definite with kappa2(L') <= 10^3.

Accuracy of an append that crosses a 128-row boundary: L' and c' against the oracle on the extended set in the units of
tests/test_gpu_append.py, e = (n + m + 32) u kappa2(L') max |L'| (tests/_append_refs.py), bound 10, the fresh device fit's
own ratio printed beside it ("RESERVE_PATCH ..." with -s).

The padding state right after a crossing is checked without a refit, in fp64 (pmk_model_load takes doubles, so an fp32
factor has no bit-identical twin): L and c of the appended model are loaded into a fresh unreserved model, and the
-D^-1 blocks, the leave-one-out values, log det, the items of a planned query and its covariance blocks must have equal
bits on the two.  That is what a wrong nt, a stale -D^-1 block or a dirty padding row would change.

A reserve already satisfied must keep the device pointers: pmk_test_model_buffers (include/pmk_test.h) reports them.
"""
import ctypes as C

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import mixture as M
from oracle import oracle as O
import _append_cases as AC
import _append_refs as AR
import _reserve_cases as RC
import _cov_refs as CR
import _grad_refs as GR
import _vgrad_refs as VR
from test_gpu_append import _blend_weights, _fit, _hash, _raw, _refit, _state
from test_gpu_grad import _worst_ratio

pytestmark = pytest.mark.gpu

TH = AC.FAMILIES["spline34"][0]


def _same(a, b):
    """equal bits, NaN included"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _scores(model):
    """what a fitted model computes from its factor alone: log det, y^T c and the leave-one-out values"""
    logdet, quad = model.evidence()
    model.loo()
    res, var = model.loo_values()
    return [logdet, quad] + list(res) + list(var)


def _assert_same_model(a, b, scores=True):
    assert np.array_equal(a.info(), b.info())
    for r, ((La, ca, ia), (Lb, cb, ib)) in enumerate(zip(_state(a), _state(b))):
        assert _same(La, Lb) and _same(ca, cb) and _same(ia, ib), r
    if scores:
        for k, (x, y) in enumerate(zip(_scores(a), _scores(b))):
            assert _same(x, y), k


def _buffers(model):
    """the device addresses of the slabs, the coordinates and the weights"""
    out = [C.c_int64() for _ in range(3)]
    assert model.ctx.L.pmk_test_model_buffers(model.h, *[C.byref(v) for v in out]) == 0
    return [v.value for v in out]


def _stride_model(D, dtype, reserve):
    case = RC.stride(D, dtype)
    fams, s2 = RC.STRIDE_FAMILIES[D], RC.STRIDE_SIGMA2[dtype]
    model = M.DeviceModel(case.Xs, case.ys, dtype=dtype)
    if case.ds is not None:
        model.set_diag(case.ds)
    if reserve is not None:
        free = model.reserve(reserve)
        lds = [RC.ld_after(n, r) for n, r in zip(RC.STRIDE_SIZES, reserve)]
        assert np.array_equal(free, np.array(lds) - RC.STRIDE_SIZES), free
    _refit(model, fams, s2)
    return model


# ------------------------------------------------------------------------------------------ 1, 2: the stride
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("D", [1, 2, 4])
def test_the_stride_does_not_matter_and_a_reserve_moves_nothing_else(D, dtype):
    """patches of 1, 100, 128, 129 and 300 points, reserves of 200, 0, 1, 1 and 128 rows; D = 2 has one kernel family
    and noise per patch and addends"""
    plain = _stride_model(D, dtype, None)
    assert np.all(plain.info() == 0)
    assert np.array_equal(plain.capacity(), [128 * ((n + 127) // 128) - n for n in RC.STRIDE_SIZES])
    # ---- reserved before the fit: the fit, the scores
    reserved = _stride_model(D, dtype, RC.STRIDE_RESERVE)
    _assert_same_model(reserved, plain)
    # ---- reserve on the fitted model, no fit in between; then a second, larger one; then one already satisfied
    h0 = _hash(plain)
    plain.loo()
    free = plain.reserve(RC.STRIDE_RESERVE)
    assert np.array_equal(free, reserved.capacity())
    with pytest.raises(pmk.PmkError, match="loo\\(\\) has not run"):
        plain.loo_values()
    assert _hash(plain) == h0
    _assert_same_model(plain, reserved)
    lds = [RC.ld_after(n, r) for n, r in zip(RC.STRIDE_SIZES, RC.STRIDE_RESERVE)]
    more = [RC.ld_after(n, r, ld) for n, r, ld in zip(RC.STRIDE_SIZES, RC.STRIDE_RESERVE_MORE, lds)]
    assert np.array_equal(plain.reserve(RC.STRIDE_RESERVE_MORE), np.array(more) - RC.STRIDE_SIZES)
    assert _hash(plain) == h0
    _assert_same_model(plain, reserved)
    at = _buffers(plain)
    assert np.array_equal(plain.reserve(0), np.array(more) - RC.STRIDE_SIZES)       # satisfied: nothing moves
    assert np.array_equal(plain.reserve(RC.STRIDE_RESERVE), np.array(more) - RC.STRIDE_SIZES)
    assert _buffers(plain) == at and _hash(plain) == h0
    # ---- a fit in the larger layout is still the fit
    _refit(plain, RC.STRIDE_FAMILIES[D], RC.STRIDE_SIGMA2[dtype])
    _assert_same_model(plain, reserved, scores=False)


def test_info_of_a_failed_patch_is_kept():
    """a negative noise variance fails the first pivot of its patch (k(x, x) + sigma2 = 1 - 5); reserve keeps that info
    and the other patches' bits"""
    rng = np.random.default_rng(41)
    Xs = [rng.uniform(-6, 6, (n, 2)) for n in (40, 130, 20)]
    ys = [AC.target(x) for x in Xs]
    model = M.DeviceModel(Xs, ys)
    model.fit_patches([TH] * 3, [1e-2, -5.0, 1e-2])
    info = model.info()
    assert np.array_equal(info, [0, 1, 0]), info
    before = _state(model)
    model.reserve([10, 300, 128])
    assert np.array_equal(model.info(), info)
    after = _state(model)
    for r in (0, 2):
        assert all(_same(a, b) for a, b in zip(before[r], after[r])), r
    assert _same(before[1][0], after[1][0])              # whatever a failed factorisation left is moved as it is


# ------------------------------------------------------------------------------------------ 1, 2, 5: through a tree
def _tree_outputs(eta, t, th, s2):
    """items, blend, gradient, variance gradient and covariance of the tree case's queries, every array as it comes"""
    args = (t.root, t.LEVELS, t.RADIUS, t.DELTA)
    out = list(pmk.querymixtureGP_patches(t.Xq, eta, *args, t.wth)[:2])
    out += list(pmk.querymixtureGP_cov(t.Xq, eta, *args, t.wth))
    _refit_multi(eta, t.y)                               # the gradients run on the multi-output path
    out += list(pmk.querymixtureGP_grad(t.Xq, eta, *args, th, s2, t.wth, variance=True))
    q = M.DeviceQuery(eta._model, t.Xq)
    q.plan(t.RADIUS, t.DELTA)
    q.items_fitted()
    dbg = q.debug()
    return out + [dbg["item_region"], dbg["item_t"], dbg["item_u"], dbg["item_v"]]


def _tree_eta(t, th, s2, X, y, reserve=None):
    eta = pmk.MixtureGPType.from_tree(t.root, X, t.EPS, dtype=t.dtype, reserve=reserve)
    pmk.fitmixtureGP_(eta, y, th, s2)
    return eta


def _refit_multi(eta, y):
    model = eta._model
    model.set_targets_multi_global(y)
    model.solve_multi()
    eta.C_set = model.weights_multi()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_tree_model_of_eight_leaves_gives_the_same_bits_at_every_stride(dtype):
    t = RC.Tree8(dtype)
    th, s2 = TH, AC.SIGMA2[dtype]
    plain = _tree_eta(t, th, s2, t.X, t.y)
    assert plain._model.P == 8
    want = _tree_outputs(plain, t, th, s2)
    reserved = _tree_eta(t, th, s2, t.X, t.y, reserve=130)
    assert np.all(reserved._model.capacity() >= 130)
    for k, (a, b) in enumerate(zip(_tree_outputs(reserved, t, th, s2), want)):
        assert _same(a, b), k
    # reserve on the fitted eta: the multi-output targets go (as after an append) and are set again
    off0, inds0 = (a.copy() for a in plain._model.patch_index())
    pmk.reservemixtureGP_(plain, [0, 1, 127, 128, 129, 300, 5, 1000])
    with pytest.raises(pmk.PmkError, match="no multi-output targets"):
        plain._model.solve_multi()
    off1, inds1 = plain._model.patch_index()
    assert np.array_equal(off0, off1) and np.array_equal(inds0, inds1) and plain._model.N == len(t.X)
    for k, (a, b) in enumerate(zip(_tree_outputs(plain, t, th, s2), want)):
        assert _same(a, b), k


def test_append_global_on_a_reserved_tree_model_through_the_blend():
    """test_append_global_through_the_blend of tests/test_gpu_append.py on a from_tree(..., reserve=128) model and a point
    set (RC.TreeCross) that gives two patches more points than they could take without the reserve and takes them across
    a 128-row boundary: the same comparisons under the same bounds, by the same code where that test has it in a function.

    The appended model against a from_tree model of the extended global array, through querymixtureGP_patches,
    querymixtureGP_cov and querymixtureGP_grad(..., variance=True); each bound is the sum of the two models' unit bounds:
    covariance   every region block and the blended matrix of BOTH models within 10 units of the long-double reference of
                 tests/_cov_refs.py (units (n + 32) u kappa2(L) (k0 + |V_a| |V_b|))
    variances    an item's v within 10 (n + 32) u vunit and its gradient within 10 (n + 32) u unit_d of the truth
                 (tests/_vgrad_refs.py): twice that between the models
    means        c' of both models within 10 e of the oracle (asserted here), so the weights differ by dC <= 20 e and an
                 item's mean by sum_k |kq_k| dC, its gradient by sum_k |g_k,d| dC, plus the (n + 32) u sum_k |kq_k c_k|
                 (resp. |g_k,d c_k|) of each model's own sum
    blend        Y, V, dY, dV carry the item bounds through their weights; their own rounding is 16 m u of the sum of
                 their terms' magnitudes per model."""
    t = RC.TreeCross("f64")
    (th, oth), s2, u = AC.FAMILIES["spline34"], AC.SIGMA2["f64"], AR.U_OF["f64"]
    owth = O.kernel(O.SPLINE34, 1 / t.RADIUS)
    eta = pmk.MixtureGPType.from_tree(t.root, t.X, t.EPS, reserve=128)
    pmk.fitmixtureGP_(eta, t.y, th, s2)
    model = eta._model
    off0, inds0 = (a.copy() for a in model.patch_index())
    n0 = np.diff(off0)
    first = model.N
    ob = O.BSP(t.X, t.LEVELS)
    ooff, oinds, oloff, olists = ob.assign(t.Xnew, t.EPS)
    mult, counts = np.diff(oloff), np.diff(ooff)
    assert (mult == 1).any() and (mult == 2).any() and (mult >= 3).any(), mult
    # the reserve is what lets this append through, and it crosses a block row
    tiles = lambda v: (v + 127) // 128
    assert (counts > 128 * tiles(n0) - n0).sum() >= 2 and (tiles(n0 + counts) > tiles(n0)).sum() >= 2, (n0, counts)
    pmk.appendmixtureGP_(eta, t.Xnew, t.ynew)
    assert model.N == first + len(t.Xnew) and model.n.sum() == off0[-1] + mult.sum()
    assert np.array_equal(model.n, n0 + counts)
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
            assert AR.ratio(mdl.get(r, M.GET_C), fit["c_chol"], e) <= RC.RATIO_MAX, r
            assert AR.ratio(mdl.get(r, M.GET_L), fit["L"], e) <= RC.RATIO_MAX, r
        dC.append(2 * RC.RATIO_MAX * e)
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
    print("RESERVE_BLEND cov", dict(blocks=worst_block, blend=worst_cov))
    assert worst_block <= RC.RATIO_MAX and worst_cov <= RC.RATIO_MAX, (worst_block, worst_cov)

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
        dv[sel] = 2 * RC.RATIO_MAX * (nr[r] + 32) * u * it["vunit"]
        dGV[sel] = 2 * RC.RATIO_MAX * (nr[r] + 32) * u * it["unit"]
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
    print("RESERVE_BLEND items", worst)
    assert max(worst.values()) <= 1.0, worst
    # the *_global setters take the new N, through the chunk prefix of the new strides
    with pytest.raises(ValueError):
        model.set_targets_global(t.y)
    model.set_targets_global(t.yall)


# ------------------------------------------------------------------------------------------ 3, 4: crossing block rows
def _query_state(model, root, Xq):
    """item means, variances and covariance blocks of a planned query on `model` with the tree attached"""
    model.set_bsp(root, 0)
    q = M.DeviceQuery(model, Xq)
    q.plan(0.5, 1e-5)
    q.items_fitted()
    dbg = q.debug()
    q.items_cov()
    blocks = [q.item_covs(r)[1] for r in sorted(set(int(v) for v in dbg["item_region"]))]
    return [dbg["item_region"], dbg["item_u"], dbg["item_v"]] + blocks


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", RC.CROSSING_NAMES)
def test_appends_that_cross_block_rows(name, dtype):
    case = RC.crossing(name, dtype)
    P, s2 = case.P, [RC.SIGMA2[dtype]] * case.P
    fams = ["spline34"] * P
    model = _fit(case.Xs, case.ys, fams, s2, dtype)
    model.reserve(RC.RESERVE_ROWS)
    before = _state(model)
    root, Xq = RC.query_points(P, 40, 7) if P in (4, 8) else (None, None)
    if root is not None:                                 # a query made before the crossing: planned again below
        model.set_bsp(root, 0)
        old_q = M.DeviceQuery(model, Xq)
        old_q.plan(0.5, 1e-5)
        old_q.items_fitted()
    model.loo()                                          # the leave-one-out tasks of the old tile counts exist
    info = model.append(case.Xn, case.yn)
    assert np.all(info == 0), info
    assert np.array_equal(model.n, [n + m for n, m in case.sizes])
    assert np.array_equal(model.capacity(), [RC.ld_after(n, RC.RESERVE_ROWS) - n - m for n, m in case.sizes])
    after = _state(model)
    fresh = _fit(case.Xe, case.ye, fams, s2, dtype)
    fstate = _state(fresh)
    worst = dict(L=0.0, c=0.0)
    for r, (n, m) in enumerate(case.sizes):
        L0, L1, c1 = before[r][0], after[r][0], after[r][1]
        assert L1.shape == (n + m, n + m)
        assert _same(L1[:n, :n], L0), r
        assert np.array_equal(L1[:n, n:], np.zeros((n, m))), r
        assert np.array_equal(np.triu(L1, 1), np.zeros_like(L1)), r
        fit = O.fit_patch(AC.FAMILIES["spline34"][1], case.Xe[r], case.ye[r], s2[r], want_K=True)
        assert fit["info"] == 0
        kappa = AR.kappa_of(fit["K"] + s2[r] * np.eye(n + m))
        assert kappa <= RC.KAPPA_MAX
        e = AR.unit(n + m, dtype, kappa, fit["L"])
        got = dict(L=AR.ratio(L1, fit["L"], e), c=AR.ratio(c1, fit["c_chol"], e),
                   L_fresh=AR.ratio(fstate[r][0], fit["L"], e), c_fresh=AR.ratio(fstate[r][1], fit["c_chol"], e))
        print("RESERVE_PATCH", name, dtype, r, n, m, {k: round(v, 4) for k, v in got.items()})
        worst["L"], worst["c"] = max(worst["L"], got["L"]), max(worst["c"], got["c"])
    assert worst["L"] <= RC.RATIO_MAX and worst["c"] <= RC.RATIO_MAX, worst
    # ---- the padding state right after the crossing, no refit: a fresh unreserved model loaded with these L and c
    if dtype == "f64":
        loaded = M.DeviceModel.from_factors(case.Xe, [s[1] for s in after], [s[0] for s in after])
        loaded.set_kernels([TH] * P)
        for r, (L, c, inv) in enumerate(_state(loaded)):
            assert _same(L, after[r][0]) and _same(c, after[r][1]), r
            assert _same(inv, after[r][2]), (r, np.nonzero((inv != after[r][2]).any(axis=(1, 2)))[0])
        assert _same(model.evidence(quad=False)[0], loaded.evidence(quad=False)[0])
        model.loo(); loaded.loo()
        for k, (a, b) in enumerate(zip(*[sum(map(list, mdl.loo_values()), []) for mdl in (model, loaded)])):
            assert _same(a, b), k
        if root is not None:
            want = _query_state(loaded, root, Xq)
            for k, (a, b) in enumerate(zip(_query_state(model, root, Xq), want)):
                assert _same(a, b), k
            # the query created before the reserve's rows were entered, planned again: the bits of a new query
            old_q.plan(0.5, 1e-5)
            old_q.items_fitted()
            dbg = old_q.debug()
            assert _same(dbg["item_u"], want[1]) and _same(dbg["item_v"], want[2])
    # ---- a fit after the append is the fit of a fresh unreserved model of the extended sets, bit for bit
    _refit(model, fams, s2)
    _assert_same_model(model, fresh)


def test_a_query_made_before_the_reserve_follows_the_model():
    """the query keeps its plan across reserve(): its next launch reads the new buffers; planned again it is a new query"""
    case = RC.crossing("cross", "f64")
    s2 = [RC.SIGMA2["f64"]] * case.P
    model = _fit(case.Xs, case.ys, ["spline34"] * case.P, s2, "f64")
    root, Xq = RC.query_points(case.P, 40, 7)
    model.set_bsp(root, 0)
    q = M.DeviceQuery(model, Xq)
    q.plan(0.5, 1e-5)
    q.items_fitted()
    want = q.debug()
    model.reserve(RC.RESERVE_ROWS)
    q.items_fitted()                                     # the old plan, the new layout
    got = q.debug()
    assert _same(got["item_u"], want["item_u"]) and _same(got["item_v"], want["item_v"])
    q.plan(0.5, 1e-5)
    q.items_fitted()
    got = q.debug()
    assert _same(got["item_u"], want["item_u"]) and _same(got["item_v"], want["item_v"])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_append_remove_append_on_one_reserved_model(dtype):
    """120 -> 140 (enters a block row), 140 -> 130 (a removal inside that block row), 130 -> 150; then the fit of the
    model equals the fit of a fresh model of the points it holds"""
    rng = np.random.default_rng(52)
    pts = AC.rnd(rng.uniform(-3, 3, (160, 2)), dtype)
    y = AC.target(pts)
    s2 = RC.SIGMA2[dtype]
    model = M.DeviceModel([pts[:120]], [y[:120]], dtype=dtype)
    model.reserve(100)
    model.fit(TH, s2)
    assert np.all(model.append([pts[120:140]], [y[120:140]]) == 0)
    assert np.array_equal(model.removable(), [140 - 128 - 1])
    gone = np.array([129, 131, 132, 133, 134, 135, 136, 137, 138, 139])
    assert np.all(model.remove([gone]) == 0)
    assert np.all(model.append([pts[140:160]], [y[140:160]]) == 0)
    keep = np.concatenate([np.delete(np.arange(140), gone), np.arange(140, 160)])
    assert np.array_equal(model.X[0], pts[keep]) and model.n[0] == 150
    fit = O.fit_patch(AC.FAMILIES["spline34"][1], pts[keep], y[keep], s2, want_K=True)
    e = AR.unit(150, dtype, AR.kappa_of(fit["K"] + s2 * np.eye(150)), fit["L"])
    # three updates in a row: each within the 10 units of its own test
    assert AR.ratio(model.get(0, M.GET_L), fit["L"], e) <= 3 * RC.RATIO_MAX
    assert AR.ratio(model.get(0, M.GET_C), fit["c_chol"], e) <= 3 * RC.RATIO_MAX
    fresh = M.DeviceModel([pts[keep]], [y[keep]], dtype=dtype)
    fresh.fit(TH, s2)
    model.fit(TH, s2)
    _assert_same_model(model, fresh)


# ------------------------------------------------------------------------------------------ 6: refusals
def _reserve_raw(model, rows):
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    rc = model.ctx.L.pmk_model_reserve(model.h, rows.ctypes.data_as(C.POINTER(C.c_int64)))
    return rc, model.ctx.L.pmk_last_error().decode()


def test_refusals_leave_the_model_as_it_was():
    rng = np.random.default_rng(9)
    Xs = [rng.uniform(-3, 3, (n, 2)) for n in (30, 128, 130)]      # two tiles: the split path can be forced
    ys = [AC.target(x) for x in Xs]
    model = M.DeviceModel(Xs, ys)
    model.fit(TH, 1e-2)
    h0, free0 = _hash(model), model.capacity()

    def unchanged():
        return _hash(model) == h0 and np.array_equal(model.capacity(), free0)

    rc, msg = _reserve_raw(model, [5, -1, 5])
    assert rc == -2 and "rows[1] = -1" in msg and unchanged(), (rc, msg)
    with pytest.raises(pmk.PmkError):
        model.reserve(-3)
    rc, msg = _reserve_raw(model, [0, 0, 2 ** 24 - 129])
    assert rc == -4 and "patch 2" in msg and unchanged(), (rc, msg)
    assert model.ctx.L.pmk_model_reserve(model.h, None) == -1 and unchanged()
    # a model on the split path
    assert model.ctx.L.pmk_test_model_set_split(model.h, 1) == 0
    rc, msg = _reserve_raw(model, [5, 5, 5])
    assert rc == -3 and "split path" in msg, (rc, msg)
    assert model.ctx.L.pmk_test_model_set_split(model.h, 0) == 0
    assert unchanged()
    # a default model keeps its refusal: a full patch takes nothing
    x1, y1 = np.zeros((1, 2)), np.zeros(1)
    rc, msg = _raw(model, x1, y1, [1])
    assert rc == -4 and "patch 1 has 0 free rows (n = 128, ld = 128), 1 rows asked for" in msg and unchanged(), (rc, msg)
    # with room: 129 points for one patch in one call, and more points than the free rows
    assert np.array_equal(model.reserve([200, 10, 0]), [226, 128, 126])
    free0 = model.capacity()
    assert unchanged()
    rc, msg = _raw(model, np.zeros((129, 2)), np.zeros(129), [0] * 129)
    assert rc == -5 and "129 points for patch 0 in one call, the limit is 128 per patch" in msg and unchanged(), (rc, msg)
    rc, msg = _raw(model, np.zeros((127, 2)), np.zeros(127), [2] * 127)
    assert rc == -4 and "patch 2 has 126 free rows (n = 130, ld = 256), 127 rows asked for" in msg and unchanged(), (rc, msg)
    with pytest.raises(ValueError, match="129 points for patch 0"):
        model.append([np.zeros((129, 2)), x1[:0], x1[:0]], [np.zeros(129), y1[:0], y1[:0]])
    # the split path is not offered to a model that holds reserved rows
    assert model.ctx.L.pmk_test_model_set_split(model.h, 1) == -3
    assert unchanged()
