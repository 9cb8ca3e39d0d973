"""What runs AFTER an append (pmk_model_append): the consumers of the state an append rewrites (n on both sides, the index
list and N of a tree-built model, the leave-one-out, multi-output and trend state) and of what it leaves alone (the trend
degree, the trend columns' dirty mark, d_tinfo, the target block, every live query object), plus the calls that
tests/test_gpu_append.py does not make: calls of different shape on one model, the raw ABI with interleaved items, and the
refusal of global indices that do not ascend within a patch.

No bound is new.  Each is the bound the named test applies to a freshly fitted model, and the fresh model of the extended
points is measured on the same inputs beside the appended one:

  blended leave-one-out   tests/test_gpu_loo_blend.py: against brute-force refits (tests/_append_after_refs.py, checked on
                          the CPU by tests/test_append_after_refs.py), |dY| <= cond_2 u max|y|, |dV| <= cond_2 u (k(0) + sigma2)
  ... multi-output        tests/test_gpu_loo_blend_multi.py: the same units on R columns, long-double refits with the trend
  trend                   tests/test_gpu_trend.py: a figure within 10 x the larger of its unit kappa_2(U) u scale and what
                          fp64 scipy achieves in that unit, against tests/_trend_refs.py
  L' and c'               tests/test_gpu_append.py: 10 units e = (n + m + 32) u kappa2(L') max |L'|

Every measured ratio is printed before it is asserted ("APPEND_AFTER {json}"); a run of the whole module writes them to
profiles/append_after_accuracy.json.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
from patchmixturekriging_amd import mixture as M
from oracle import oracle as O
import _append_after_refs as AA
import _append_cases as AC
import _append_refs as AR
import _loo_blend_refs as BR
import _loo_blend_multi_refs as MR
import _trend_refs as T
import test_gpu_append as TA
from test_gpu_multi_output import kappa

pytestmark = pytest.mark.gpu

_RECORDS = []
ACCURACY_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                             "append_after_accuracy.json")
WHOLE_MODULE = {("blend", "f64"), ("blend", "f32"), ("blend_multi", "f64"), ("trend", "f64"), ("shapes", "f64"),
                ("shapes", "f32")}
TH, OTH = AC.FAMILIES["spline34"]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def _record(**kw):
    _RECORDS.append(kw)
    print("APPEND_AFTER " + json.dumps(kw, sort_keys=True))


@pytest.fixture(scope="module", autouse=True)
def _write_accuracy_file():
    """only a run of the whole module replaces the file"""
    yield
    if {(r["test"], r["dtype"]) for r in _RECORDS} >= WHOLE_MODULE:
        with open(ACCURACY_JSON, "w") as f:
            f.write("[\n" + ",\n".join(" " + json.dumps(r, sort_keys=True) for r in _RECORDS) + "\n]\n")


def _owth(radius):
    return O.kernel(O.SPLINE34, 1.0 / radius)


def _wth(radius):
    return pmk.Spline34KernelType(1.0 / radius)


def _tree_etas(t, dtype, s2):
    """(eta appended by appendmixtureGP_, eta built on the extended array): both fitted; the appended one has used its old
    index list and its old leave-one-out values, which the append makes stale"""
    eta = pmk.MixtureGPType.from_tree(t.root, t.X, t.EPS, dtype=dtype)
    pmk.fitmixtureGP_(eta, t.y, TH, s2)
    pmk.loomixtureGP_blend(eta, t.root, t.RADIUS, t.DELTA, t.wth)
    pmk.appendmixtureGP_(eta, t.Xnew, t.ynew)
    fresh = pmk.MixtureGPType.from_tree(t.root, t.Xall, t.EPS, dtype=dtype)
    pmk.fitmixtureGP_(fresh, t.yall, TH, s2)
    return eta, fresh


def _same_lists(model, o):
    off, inds = model.patch_index()
    for r, s in enumerate(o.sets):
        assert np.array_equal(inds[off[r]:off[r + 1]], s), r


# ------------------------------------------------------------------------------------------ a. blended leave-one-out
_BLEND_REF = {}


def _blend_reference(dtype):
    """brute-force refits at all 418 points, latent and noisy: computed once per precision"""
    if dtype not in _BLEND_REF:
        t, o = AA.tree_oracle(dtype)
        pts = list(range(len(t.Xall)))
        _BLEND_REF[dtype] = (o.blend_refit(_owth(t.RADIUS), t.RADIUS, pts, t.DELTA),
                             o.blend_refit_noisy(_owth(t.RADIUS), t.RADIUS, pts, t.DELTA))
    return _BLEND_REF[dtype]


def _score_bound(res, var, bY, bV):
    """what |dmu| <= bY and |dvar| <= bV move loo_log_pseudo_likelihood by, to first order and doubled for the second
    order: sum_j |dvar| / (2 var) + |res| |dmu| / var + res^2 |dvar| / (2 var^2)"""
    return 2.0 * float(np.sum(bV / (2 * var) + np.abs(res) * bY / var + res * res * bV / (2 * var * var)))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_blended_leave_one_out_after_appendmixtureGP(dtype):
    """loomixtureGP_blend of the appended model over all 418 points against brute-force refits, latent and noisy: both
    ratios of BR.ratios <= 1, the fresh from_tree model of the extended array held to the same; the item counts against the
    oracle's (a new row the bisection of patch_holds missed would be one strip item more); selectblendGP_ on both."""
    t, o = AA.tree_oracle(dtype)
    s2, u, n0, N = AC.SIGMA2[dtype], AR.U_OF[dtype], len(t.X), len(t.Xall)
    eta, fresh = _tree_etas(t, dtype, s2)
    assert eta._model.N == N and fresh._model.N == N
    for e_ in (eta, fresh):
        _same_lists(e_._model, o)
    cond, ymax, k0s2 = o.cond2(), np.abs(t.yall).max(), o.k0() + s2
    got = {}
    for noisy, (Yr, Vr) in zip((False, True), _blend_reference(dtype)):
        for name, e_ in (("appended", eta), ("fresh", fresh)):
            Y, V = pmk.loomixtureGP_blend(e_, t.root, t.RADIUS, t.DELTA, t.wth, noisy=noisy)
            got[(name, noisy)] = BR.ratios(Y, V, Yr, Vr, cond, u, ymax, k0s2)
    # ---- counts: every item whose patch holds its point is a member item
    ototal, ostrip, multi, homeless = o.counts(t.RADIUS, t.DELTA)
    assert homeless == 0 and multi >= 1 and 0 < ostrip < ototal
    home, regs, _ = o.plan(t.RADIUS, t.DELTA)
    for name, e_ in (("appended", eta), ("fresh", fresh)):
        m = e_._model
        q = pmk.DeviceQuery(m, t.Xall)
        total = q.plan(t.RADIUS, t.DELTA)
        nm, ns = q.items_loo(True)
        assert (total, ns, nm) == (ototal, ostrip, ototal - ostrip), (name, total, nm, ns, ototal, ostrip)
        dbg = q.debug()
        off, reg = dbg["item_offsets"], dbg["item_region"]
        _, var = m.loo_values()
        seen = 0
        for j in range(n0, N):                      # a new point is a member of each patch the tree assigned it to
            assert list(reg[off[j]:off[j + 1]]) == [int(r) for r in regs[j]] + [int(home[j])], j
            assert o.row_of(int(home[j]), j) >= 0, j
            for k in range(off[j], off[j + 1]):
                i = o.row_of(int(reg[k]), j)
                if i >= 0 and dtype == "f64":       # a member item's noisy variance IS the resident 1 / d_i
                    assert same_bits(dbg["item_v"][k], var[int(reg[k])][i]), (name, j, k)
                seen += i >= 0
        assert N - n0 <= seen <= int(AA.multiplicity(o, n0).sum())      # not every patch that holds a point is blended at it
    # ---- selectblendGP_ over two candidates
    cands = [(t.RADIUS, t.DELTA, t.wth), (0.9, t.DELTA, _wth(0.9))]
    sa, ba = pmk.selectblendGP_(eta, t.root, t.yall, cands)
    sf, bf = pmk.selectblendGP_(fresh, t.root, t.yall, cands)
    bounds = []
    for radius, delta, wth in cands:
        mu, var = pmk.loomixtureGP_blend(fresh, t.root, radius, delta, wth, noisy=True)
        bounds.append(2 * _score_bound(t.yall - mu, var, cond * u * ymax, cond * u * k0s2))     # the sum of two models' bounds
    _record(test="blend", dtype=dtype, cond2=cond, items=ototal, n_strip=ostrip,
            dY_latent=got[("appended", False)][0], dV_latent=got[("appended", False)][1],
            dY_noisy=got[("appended", True)][0], dV_noisy=got[("appended", True)][1],
            dY_latent_fresh=got[("fresh", False)][0], dV_latent_fresh=got[("fresh", False)][1],
            dY_noisy_fresh=got[("fresh", True)][0], dV_noisy_fresh=got[("fresh", True)][1], bound=1.0,
            select_scores=[float(v) for v in sa], select_scores_fresh=[float(v) for v in sf],
            select_score_bounds=[float(b) for b in bounds], select_best=ba, select_best_fresh=bf)
    for key, (ry, rv) in got.items():
        assert ry <= 1.0 and rv <= 1.0, (key, ry, rv)
    assert ba == bf and np.all(np.isfinite(sa)) and np.all(np.isfinite(sf))
    assert np.all(np.abs(sa - sf) <= np.array(bounds)), (sa, sf, bounds)


def test_blended_leave_one_out_multi_after_an_append():
    """loomixtureGP_blend_multi with R = 2 and a constant trend: the trend degree survives the append, the target block and
    the weights do not.  Against long-double refits with the trend at the 18 new points and 18 old ones (a refit costs 20
    ms), in the units of tests/test_gpu_loo_blend_multi.py, both ratios <= 1; the fresh model beside it."""
    dtype = "f64"
    t, _ = AA.tree_oracle(dtype)
    s2, u, n0 = AC.SIGMA2[dtype], AR.U_OF[dtype], len(t.X)
    Yall = np.asfortranarray(AA.targets2(t.Xall))
    mo = AA.MultiOracle(t.X, t.Xall, Yall, t.EPS, AA.hyper(dtype), "constant", t.LEVELS)
    eta = pmk.MixtureGPType.from_tree(t.root, t.X, t.EPS)
    pmk.fitmixtureGP_trend_(eta, np.asfortranarray(Yall[:n0]), TH, s2, "constant")
    pmk.loomixtureGP_blend_multi(eta, t.root, t.RADIUS, t.DELTA, t.wth)
    pmk.appendmixtureGP_(eta, t.Xnew, np.ascontiguousarray(Yall[n0:, 0]))
    model = eta._model
    assert eta.C_set is None and eta.beta_set is None
    with pytest.raises(pmk.PmkError, match="solve_multi has not run"):
        pmk.loomixtureGP_blend_multi(eta, t.root, t.RADIUS, t.DELTA, t.wth)
    with pytest.raises(pmk.PmkError, match="no multi-output targets"):
        model.solve_multi()
    model.set_targets_multi_global(Yall)
    model.solve_multi()
    assert np.all(model.trend_info() == 0) and model.trend()[0][0].shape == (1, 2)        # the constant trend is still set
    fresh = pmk.MixtureGPType.from_tree(t.root, t.Xall, t.EPS)
    pmk.fitmixtureGP_trend_(fresh, Yall, TH, s2, "constant")
    _same_lists(model, mo)
    pts, MUr, Vr = mo.blend(_owth(t.RADIUS), mo.items(t.RADIUS, "ref", points=AA.check_points(t)))
    cond, ymax, k0s2 = mo.cond2(), np.abs(Yall).max(), mo.k0() + s2
    ototal, oother, _, _ = mo.counts(t.RADIUS, t.DELTA)
    got = {}
    for name, e_ in (("appended", eta), ("fresh", fresh)):
        MU, V = pmk.loomixtureGP_blend_multi(e_, t.root, t.RADIUS, t.DELTA, t.wth)
        assert MU.shape == (len(t.Xall), 2)
        got[name] = MR.ratios(MU[pts], V[pts], MUr, Vr, cond, u, ymax, k0s2)
        q = pmk.DeviceQuery(e_._model, t.Xall)
        total = q.plan(t.RADIUS, t.DELTA)
        nm, no = q.items_loo_multi()
        assert (total, no, nm) == (ototal, oother, ototal - oother), (name, total, nm, no)
    _record(test="blend_multi", dtype=dtype, trend="constant", R=2, points=len(pts), cond2=cond, dY=got["appended"][0],
            dV=got["appended"][1], dY_fresh=got["fresh"][0], dV_fresh=got["fresh"][1], bound=1.0)
    for name, (ry, rv) in got.items():
        assert ry <= 1.0 and rv <= 1.0, (name, ry, rv)


# ------------------------------------------------------------------------------------------ b. unordered global indices
def _library_N(model):
    N = C.c_int64(-1)
    _lib.check(model.ctx.L.pmk_model_patch_index(model.h, C.byref(N), None, None), "pmk_model_patch_index")
    return N.value


def test_global_indices_that_do_not_ascend_are_refused():
    t, o = AA.tree_oracle("f64")
    s2, n0 = AC.SIGMA2["f64"], len(t.X)
    ooff, oinds, oloff, olists = O.BSP(t.X, t.LEVELS).assign(t.Xnew, t.EPS)
    single = np.nonzero(np.diff(oloff) == 1)[0]                 # new points that one patch holds
    patch_of = olists[oloff[single]]
    p = int(np.bincount(patch_of).argmax())
    a, b = (int(v) for v in single[patch_of == p][:2])          # two of them in one patch
    x, y = t.Xnew[[a, b]], t.ynew[[a, b]]
    model = M.DeviceModel.from_tree(t.root, t.X, t.y, t.EPS)
    model.fit(TH, s2)
    h0 = TA._hash(model)
    off0, inds0 = (v.copy() for v in model.patch_index())
    rc, msg = TA._raw(model, x, y, [p, p], gidx=[n0 + 1, n0])
    assert rc == -3, (rc, msg)
    assert ("item 1 gives patch %d the global index %d after %d: the global indices of a patch must ascend in the order given"
            % (p, n0, n0 + 1)) in msg, msg
    model._index = None
    off1, inds1 = model.patch_index()
    assert TA._hash(model) == h0 and np.array_equal(off1, off0) and np.array_equal(inds1, inds0)
    assert _library_N(model) == n0
    # equal indices are the duplicate they were before
    rc, msg = TA._raw(model, x, y, [p, p], gidx=[n0, n0])
    assert rc == -3 and "given twice" in msg, (rc, msg)
    # another patch's items between them do not matter: the order is per patch
    other = (p + 1) % model.P
    rc, msg = TA._raw(model, np.vstack([x[:1], x[:1], x[1:]]), [y[0], y[0], y[1]], [p, other, p], gidx=[n0 + 1, n0 + 2, n0])
    assert rc == -3 and "item 2 gives patch %d the global index %d after %d" % (p, n0, n0 + 1) in msg, (rc, msg)
    assert TA._hash(model) == h0 and _library_N(model) == n0
    # ---- the same two items ascending: accepted, and the blended leave-one-out counts both as members
    rc, msg = TA._raw(model, x, y, [p, p], gidx=[n0, n0 + 1])
    assert rc == 0, (rc, msg)
    model.n = model.n + np.bincount([p, p], minlength=model.P)
    Xall = np.ascontiguousarray(np.vstack([t.X, x]))
    model.N, model._index, model._X, model._X_global = n0 + 2, None, None, Xall
    model._loo_done = False
    off2, inds2 = model.patch_index()
    assert np.array_equal(inds2[off2[p]:off2[p + 1]], np.concatenate([inds0[off0[p]:off0[p + 1]], [n0, n0 + 1]]))
    assert np.all(model.info() == 0) and _library_N(model) == n0 + 2
    model.loo()
    q = pmk.DeviceQuery(model, Xall)
    total = q.plan(t.RADIUS, t.DELTA)
    nm, ns = q.items_loo(True)
    dbg = q.debug()
    off, reg = dbg["item_offsets"], dbg["item_region"]
    want = sum(int(j in set(inds2[off2[int(reg[k])]:off2[int(reg[k]) + 1]].tolist()))
               for j in range(n0 + 2) for k in range(off[j], off[j + 1]))
    assert (nm, ns) == (want, total - want), (nm, ns, want, total)
    _, var = model.loo_values()
    for k_new, j in enumerate((n0, n0 + 1)):
        ks = [k for k in range(off[j], off[j + 1]) if reg[k] == p]
        assert len(ks) == 1, (j, reg[off[j]:off[j + 1]])          # its home patch holds it
        assert same_bits(dbg["item_v"][ks[0]], var[p][int(model.n[p]) - 2 + k_new]), j


# ------------------------------------------------------------------------------------------ c. trend and multi-output state
def _packed_multi(model, r):
    """the target block of patch r, padding rows and trend columns included: ld rows of PMK_MAX_OUTPUTS"""
    L = model.ctx.L
    ld = C.c_int64()
    _lib.check(L.pmk_test_model_packed(model.h, r, 3, C.byref(ld), None), "pmk_test_model_packed")
    out = np.empty(ld.value * 16)
    _lib.check(L.pmk_test_model_packed(model.h, r, 3, C.byref(ld), M._d(out)), "pmk_test_model_packed")
    return out.reshape(ld.value, 16)


_TREND_REF = {}


def _trend_reference(case, Ye, xq, region, trend, s2):
    """per patch the long-double and the fp64 scipy figures of tests/test_gpu_trend.py, computed once per trend"""
    if trend not in _TREND_REF:
        out = []
        for r in range(case.P):
            X, Y = case.Xe[r], Ye[r]
            K, H = O.kernel_matrix(OTH, X), T.basis(X, trend)
            x = xq[region == r]
            Kq, kqq, Hq = O.cross_kernel_matrix(OTH, x, X), np.full(len(x), O.profile(OTH, 0.0)), T.basis(x, trend)
            ld, f = T.trend_reference(K, s2, Y, H), T.gls_fp64(K, s2, Y, H)
            out.append(dict(ld=ld, f64=f, pred_ld=T.predict_reference(ld, Kq, kqq, Hq), pred_f64=T.predict_fp64(f, Kq, kqq, Hq),
                            kappa=kappa(K + s2 * np.eye(len(K)))))
        _TREND_REF[trend] = out
    return _TREND_REF[trend]


def _err(dev, ref):
    return float(np.abs(np.asarray(dev, dtype=T.LD) - ref).max())


def _trend_ratios(model, case, Ye, xq, region, refs, root):
    """the figures and units of tests/test_gpu_trend.py (test_against_long_double_reference and
    test_evidence_is_the_gls_quadratic_form) for every patch -> (worst device ratio / bound per figure over the patches
    that received points, failures over all patches)"""
    u = float(np.finfo(np.float64).eps)
    Cs, (betas, _), flags = model.weights_multi(), model.trend(), model.trend_info()
    assert np.all(flags == 0), flags
    model.loo()
    RES, VAR = model.loo_values_multi()
    _, quad = model.evidence_multi()
    model.set_bsp(root, 0)
    q = TA._explicit_query(model, xq, region)
    q.items_multi_fitted(True)
    q.mix_multi(pmk.Spline34KernelType(1.0))
    MU, V = q.fetch_multi(model.R)
    worst, failures = {}, []
    for r, ref in enumerate(refs):
        ld, f, sel = ref["ld"], ref["f64"], region == r
        figures = {"beta": (betas[r], f["beta"], ld["beta"]), "weights": (Cs[r], f["C"], ld["C"]),
                   "loo_res": (RES[r], f["res"], ld["res"]), "loo_var": (VAR[r], f["var"], ld["var"]),
                   "evidence": (quad[r], f["quad"], ld["quad"]),
                   "mu": (MU[sel], ref["pred_f64"][0], ref["pred_ld"][0]), "v": (V[sel], ref["pred_f64"][1], ref["pred_ld"][1])}
        scales = {"weights": float(np.abs(ld["C_Y"]).max() + np.abs(ld["C_H"] @ ld["beta"]).max()),
                  "evidence": float(np.abs((np.asarray(Ye[r], dtype=T.LD) * ld["C_Y"]).sum(0)).max())}
        for name, (dev, f64, ref_ld) in figures.items():
            assert np.all(np.isfinite(dev)), (r, name)
            unit = ref["kappa"] * u * scales.get(name, float(np.abs(ref_ld).max()))
            d, s = _err(dev, ref_ld) / unit, _err(f64, ref_ld) / unit
            bound = 10.0 * max(1.0, s)
            if case.sizes[r][1]:                    # of the patches that received points: the others have the fresh bits
                worst[name] = max(worst.get(name, 0.0), d / bound)
            if not d <= bound:
                failures.append((r, len(case.Xe[r]), name, d, s))
    return worst, failures


def test_trend_and_multi_output_state_across_an_append():
    """D = 2, R = 2, linear trend (q = 3) on the patches of SMALL_SIZES and one of two points, which is flagged before the
    append (n <= q) and sound after it (n = 4); two more patches complete the 8 leaves that multi-output items need.
    The target block with padding rows and trend columns is the fresh model's bit for bit with the trend linear, switched
    to none (the columns an earlier solve filled are cleared) and back to constant; with a trend, both models within the
    bound of tests/test_gpu_trend.py."""
    dtype, s2 = "f64", AC.SIGMA2["f64"]
    case = AA.trend_case(dtype)
    P, R = case.P, 2
    Ys, Ye = [AA.targets2(x) for x in case.Xs], [AA.targets2(x) for x in case.Xe]
    model = M.DeviceModel(case.Xs, case.ys)
    model.fit(TH, s2)
    model.set_targets_multi(Ys)
    model.set_trend("linear")
    model.solve_multi()
    two = AA.TREND_TWO
    assert list(model.trend_info()) == [3 if r == two else 0 for r in range(P)]     # n + 1: fewer points than basis functions
    assert np.all(np.isnan(model.weights_multi()[two]))
    assert np.all(model.append(case.Xn, case.yn) == 0)
    with pytest.raises(pmk.PmkError, match="no multi-output targets"):
        model.solve_multi()
    model.set_targets_multi(Ye)
    model.solve_multi()
    fresh = M.DeviceModel(case.Xe, case.ye)
    fresh.fit(TH, s2)
    fresh.set_targets_multi(Ye)
    fresh.set_trend("linear")
    fresh.solve_multi()
    # 20 query points as explicit items (a model of lists has no tree of its own): inside each patch's data
    rng = np.random.default_rng(991)
    region = np.sort(np.arange(20) % P).astype(np.int32)
    xq = np.vstack([case.Xe[r][rng.integers(len(case.Xe[r]))] + rng.uniform(-0.3, 0.3, 2) for r in region])
    root, _, _ = pmk.setuppartition(rng.uniform(-4, 4, (64, 2)), 4)                 # any tree of 8 leaves: the items name their regions
    recorded = {}
    for trend, q in (("linear", 3), (None, 0), ("constant", 1)):
        if trend != "linear":
            for mdl in (model, fresh):
                mdl.set_trend(trend)
                mdl.solve_multi()
        for r, (n, m) in enumerate(case.sizes):
            blk = _packed_multi(model, r)
            assert np.array_equal(blk, _packed_multi(fresh, r)), (trend, r)
            assert np.array_equal(blk[:n + m, :R], Ye[r]) and np.all(blk[n + m:] == 0.0) and np.all(blk[:, R + q:] == 0.0), (trend, r)
            if q:
                assert np.array_equal(blk[:n + m, R:R + q], T.basis(case.Xe[r], trend)), (trend, r)
        if trend is None:
            assert model.trend()[0][0].shape == (0, R)
            continue
        refs = _trend_reference(case, Ye, xq, region, trend, s2)
        for name, mdl in (("appended", model), ("fresh", fresh)):
            worst, failures = _trend_ratios(mdl, case, Ye, xq, region, refs, root)
            recorded[(trend, name)] = worst
            assert not failures, (trend, name, failures)
    for trend in ("linear", "constant"):
        _record(test="trend", dtype=dtype, trend=trend, bound=1.0, kappa_U=max(r["kappa"] for r in _TREND_REF[trend]),
                appended=recorded[(trend, "appended")], fresh=recorded[(trend, "fresh")])


# ------------------------------------------------------------------------------------------ d. query objects
def _all_stages(q, model, wth):
    """every item stage and mix of one planned query -> dict of host results"""
    out = {}
    q.items_fitted()
    q.mix(wth)
    out["Y"], out["V"] = q.fetch()
    q.items_cov()
    q.mix_cov(wth)
    out["cov"] = q.fetch_cov().copy()
    q.items_multi_fitted(True)
    q.items_grad()
    q.items_vgrad()
    q.mix_multi(wth)
    q.mix_grad(wth)
    q.mix_vgrad(wth)
    out["Ym"], out["Vm"] = q.fetch_multi(model.R)
    out["dY"], out["dV"] = q.fetch_grad(), q.fetch_vgrad()
    return out


def test_a_query_made_before_the_append_serves_after_it():
    t, _ = AA.tree_oracle("f64")
    s2 = AC.SIGMA2["f64"]
    model = M.DeviceModel.from_tree(t.root, t.X, t.y, t.EPS)
    model.fit(TH, s2)
    model.set_targets_multi_global(t.y)
    model.solve_multi()
    q = M.DeviceQuery(model, t.Xq)
    total = q.plan(t.RADIUS, t.DELTA)
    before = _all_stages(q, model, t.wth)
    assert model.append_global(t.Xnew, t.ynew)[0] == len(t.X)
    assert np.all(model.info() == 0)
    model.set_targets_multi_global(t.yall)
    model.solve_multi()
    after = _all_stages(q, model, t.wth)                    # the same object, not planned again
    assert q.total == total
    q2 = M.DeviceQuery(model, t.Xq)
    assert q2.plan(t.RADIUS, t.DELTA) == total
    new = _all_stages(q2, model, t.wth)
    for key in before:
        assert same_bits(after[key], new[key]), key
        assert not same_bits(after[key], before[key]), key  # the stages ran again on the appended factor
        assert np.all(np.isfinite(after[key])), key


# ------------------------------------------------------------------------------------------ e. calls of different shape
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_calls_of_different_shape_on_one_model(dtype):
    """three calls, large then small with a changing set of receiving patches: the arena, the S blocks, the task lists and
    the iota buffer of the first call serve the later ones"""
    case = AA.shapes(dtype)
    s2 = AC.SIGMA2[dtype]
    fams, s2s = ["spline34"] * case.P, [s2] * case.P
    model = TA._fit(case.Xs, case.ys, fams, s2s, dtype)
    worst = dict(L=0.0, c=0.0, L_fresh=0.0, c_fresh=0.0, kappa=0.0)
    for k in range(len(AA.SHAPE_CALLS)):
        Xn, yn = AA.shape_call(case, k)
        assert np.all(model.append(Xn, yn) == 0), k
        Xk, yk = AA.shape_sets(case, k)
        assert np.array_equal(model.n, [len(x) for x in Xk])
        fresh = TA._fit(Xk, yk, fams, s2s, dtype)
        for r in range(case.P):
            for what in (0, 1):
                assert np.array_equal(TA._packed(model, r, what), TA._packed(fresh, r, what)), (k, r, what)
            fit = O.fit_patch(OTH, Xk[r], yk[r], s2, want_K=True)
            assert fit["info"] == 0
            kap = AR.kappa_of(fit["K"] + s2 * np.eye(len(yk[r])))
            e = AR.unit(len(yk[r]), dtype, kap, fit["L"])
            got = dict(L=AR.ratio(model.get(r, M.GET_L), fit["L"], e), c=AR.ratio(model.get(r, M.GET_C), fit["c_chol"], e),
                       L_fresh=AR.ratio(fresh.get(r, M.GET_L), fit["L"], e),
                       c_fresh=AR.ratio(fresh.get(r, M.GET_C), fit["c_chol"], e), kappa=kap)
            print("APPEND_AFTER_PATCH", dtype, k, r, len(yk[r]), {a: round(b, 4) for a, b in got.items()})
            for a, b in got.items():
                worst[a] = max(worst[a], b)
    _record(test="shapes", dtype=dtype, bound=AC.RATIO_MAX, **worst)
    assert worst["kappa"] <= AC.KAPPA_MAX
    assert worst["L"] <= AC.RATIO_MAX and worst["c"] <= AC.RATIO_MAX, worst
    # ld = 128 ceil(n / 128) of the patches as fitted: 128, 256, 256 and 640 rows
    assert np.array_equal(model.capacity(), [0, 0, 0, 640 - 516])
    h0 = TA._hash(model)
    rc, msg = TA._raw(model, np.zeros((1, 2)), np.zeros(1), [0])
    assert rc == -4 and "patch 0 has 0 free rows (n = 128, ld = 128), 1 rows asked for" in msg, (rc, msg)
    assert TA._hash(model) == h0
    TA._refit(model, fams, s2s)
    assert np.array_equal(model.info(), fresh.info())
    for r, (L, c, inv) in enumerate(TA._state(model)):
        FL, Fc, Finv = TA._state(fresh)[r]
        assert np.array_equal(L, FL) and np.array_equal(c, Fc) and np.array_equal(inv, Finv), r


# ------------------------------------------------------------------------------------------ f. raw ABI item order
def test_interleaved_items_through_the_raw_abi():
    """one call whose items arrive patch = [2, 0, 2, 1, 0, 2, ...] with m = (5, 1, 33): the regrouping of pmk_model_append
    against DeviceModel.append, which hands the items over grouped; the order within a patch is the order given"""
    s2, ns, ms = AC.SIGMA2["f64"], (30, 100, 60), (5, 1, 33)
    case = AC.Case(list(zip(ns, ms)), 2, "f64", 996)
    fams, s2s = ["spline34"] * 3, [s2] * 3
    order = [2, 0, 2, 1, 0, 2]
    left = [ms[r] - order.count(r) for r in range(3)]
    while sum(left):
        for r in (2, 2, 2, 2, 0, 2, 2, 2, 2, 2):
            if left[r]:
                order.append(r)
                left[r] -= 1
    assert [order.count(r) for r in range(3)] == list(ms) and order[:6] == [2, 0, 2, 1, 0, 2]
    nxt, x, y = [0, 0, 0], [], []
    for r in order:                                         # item i is the next new point of its patch
        x.append(case.Xn[r][nxt[r]])
        y.append(case.yn[r][nxt[r]])
        nxt[r] += 1
    grouped = TA._fit(case.Xs, case.ys, fams, s2s, "f64")
    assert np.all(grouped.append(case.Xn, case.yn) == 0)
    raw = TA._fit(case.Xs, case.ys, fams, s2s, "f64")
    rc, msg = TA._raw(raw, np.array(x), np.array(y), order)
    assert rc == 0, (rc, msg)
    raw.n = raw.n + np.array(ms)
    assert np.all(raw.info() == 0)
    assert TA._hash(raw) == TA._hash(grouped)
    for r in range(3):
        for what in (0, 1):
            assert np.array_equal(TA._packed(raw, r, what), TA._packed(grouped, r, what)), (r, what)
        ld = len(TA._packed(raw, r, 1))
        rows = TA._packed(raw, r, 0).reshape(2, ld)[:, ns[r]:ns[r] + ms[r]].T
        assert np.array_equal(rows, case.Xn[r]), r          # the order given within the patch
    # the same items with patch 2's reversed are another model: the order is not normalised away
    rev = TA._fit(case.Xs, case.ys, fams, s2s, "f64")
    idx2 = [i for i, r in enumerate(order) if r == 2]
    perm = list(range(len(order)))
    for i, j in zip(idx2, reversed(idx2)):
        perm[i] = j
    rc, msg = TA._raw(rev, np.array(x)[perm], np.array(y)[perm], order)
    assert rc == 0, (rc, msg)
    rev.n = rev.n + np.array(ms)
    assert np.array_equal(TA._packed(rev, 2, 0).reshape(2, -1)[:, ns[2]:ns[2] + ms[2]].T, case.Xn[2][::-1])
    assert np.array_equal(TA._packed(rev, 0, 0), TA._packed(grouped, 0, 0))
