"""What runs AFTER a removal (pmk_model_remove) on a TREE-BUILT model, whose index list is rebuilt by a host round trip: the
consumers of the state a removal rewrites (n on both sides, the index list, the leave-one-out, multi-output and trend
state) and of what it leaves alone (N, the tree, the trend degree, every live query object), plus the calls that
tests/test_gpu_remove.py does not make: the blended leave-one-out at the kept points and at points no patch holds any
more, the *_global setters, gradients, appends and removals mixed on one model, the refusals through the raw ABI, a model
whose patches are the tree's own leaves (eps=None), and a failed patch whose info names a row inside the rows left.

The removed set G is fixed by the rule of tests/_remove_after_refs.py (the first and the last entry of every patch's list,
the points 0 and N - 1, points of two patches, patch 0 taken exactly to the edge of its band); tests/test_remove_after_refs.py
checks the rule, the conditioning and the reference on the CPU.

No bound is new.  Each is the bound the named test applies to a freshly fitted model, and the fresh from_tree model of the
kept points under the same tree is measured on the same inputs beside the removed one:

  blended leave-one-out   tests/test_gpu_loo_blend.py: against brute-force refits of the REDUCED lists,
                          |dY| <= cond_2 u max|y|, |dV| <= cond_2 u (k(0) + sigma2)
  ... multi-output        tests/test_gpu_loo_blend_multi.py: the same units on R columns, long-double refits with the trend
  item gradients          tests/test_gpu_grad.py ((n + 32) u lip sum |C|, bound 1) and tests/test_gpu_vgrad.py (10 units e_d)
  L' and c'               tests/test_gpu_remove.py: 10 units e = (n + 32) u kappa2(L) max |L|, n the largest the patch had

Every measured ratio is printed before it is asserted ("REMOVE_AFTER {json}"); a run of the whole module writes them to
profiles/remove_after_accuracy.json.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import mixture as M
from oracle import oracle as O
import _append_cases as AC
import _loo_blend_refs as BR
import _loo_blend_multi_refs as MR
import _remove_after_refs as RA
import _remove_cases as RC
import _remove_refs as RR
import test_gpu_append as TA
import test_gpu_append_after as TAA
import test_gpu_grad as TG
import test_gpu_remove as TR
import test_gpu_vgrad as TV

pytestmark = pytest.mark.gpu

_RECORDS = []
ACCURACY_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                             "remove_after_accuracy.json")
WHOLE_MODULE = {("blend", "f64"), ("blend", "f32"), ("blend_multi", "f64"), ("items", "f64"), ("mixed", "f64"),
                ("mixed", "f32"), ("leaves", "f64")}
TH, OTH = AC.FAMILIES["spline34"]
same_bits, _owth, _same_lists, _library_N = TAA.same_bits, TAA._owth, TAA._same_lists, TAA._library_N


def _record(**kw):
    _RECORDS.append(kw)
    print("REMOVE_AFTER " + json.dumps(kw, sort_keys=True))


@pytest.fixture(scope="module", autouse=True)
def _write_accuracy_file():
    """only a run of the whole module replaces the file"""
    yield
    if {(r["test"], r["dtype"]) for r in _RECORDS} >= WHOLE_MODULE:
        with open(ACCURACY_JSON, "w") as f:
            f.write("[\n" + ",\n".join(" " + json.dumps(r, sort_keys=True) for r in _RECORDS) + "\n]\n")


def _kept(N, G):
    return np.setdiff1d(np.arange(N), G)


def _renumbered_lists(fresh, keep, sets):
    """the lists of the fresh model of X[keep] are `sets`, renumbered through keep"""
    off, inds = fresh.patch_index()
    assert len(off) == len(sets) + 1
    for r, s in enumerate(sets):
        assert np.array_equal(keep[inds[off[r]:off[r + 1]]], s), r


def _library_lists(model):
    """(offsets, inds) read back from the library, after the cached copy was found equal to them"""
    off1, inds1 = (a.copy() for a in model.patch_index())
    model._index = None
    off2, inds2 = model.patch_index()
    assert np.array_equal(off1, off2) and np.array_equal(inds1, inds2)
    return off2, inds2


def _counts_at(o, radius, delta, points):
    """(items, non-member items) of the oracle's plan over `points` only"""
    home, regs, _ = o.plan(radius, delta)
    total = strip = 0
    for j in points:
        items = [int(r) for r in regs[j]] + [int(home[j])]
        total += len(items)
        strip += sum(o.row_of(r, int(j)) < 0 for r in items)
    return total, strip


# ------------------------------------------------------------------------------------------ a. blended leave-one-out
_BLEND_REF = {}


def _blend_reference(dtype):
    """brute-force refits of the reduced lists at all 400 points, latent and noisy: computed once per precision.  At a
    point of G nothing is refitted: no patch holds it"""
    if dtype not in _BLEND_REF:
        t, _, o = RA.tree_oracle(dtype)
        pts = list(range(len(t.X)))
        _BLEND_REF[dtype] = (o.blend_refit(_owth(t.RADIUS), t.RADIUS, pts, t.DELTA),
                             o.blend_refit_noisy(_owth(t.RADIUS), t.RADIUS, pts, t.DELTA))
    return _BLEND_REF[dtype]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_blended_leave_one_out_after_removemixtureGP(dtype):
    """loomixtureGP_blend of the removed model over all 400 points against brute-force refits of the reduced lists, latent
    and noisy: both ratios of BR.ratios <= 1 at the kept points and at the points of G (which no patch holds: the plain
    blend of the fitted patches); the fresh from_tree model of the kept points held to the same.  The item counts against
    the oracle's: a removed first or last entry that the bisection of patch_holds still found would be a member item."""
    t, G, o = RA.tree_oracle(dtype)
    s2, u, N = AC.SIGMA2[dtype], RR.U_OF[dtype], len(t.X)
    keep = _kept(N, G)
    eta = pmk.MixtureGPType.from_tree(t.root, t.X, t.EPS, dtype=dtype)
    pmk.fitmixtureGP_(eta, t.y, TH, s2)
    pmk.loomixtureGP_blend(eta, t.root, t.RADIUS, t.DELTA, t.wth)           # leave-one-out state that the removal makes stale
    pmk.removemixtureGP_(eta, G)
    model = eta._model
    assert model.N == N and not model._loo_done
    fresh = pmk.MixtureGPType.from_tree(t.root, np.ascontiguousarray(t.X[keep]), t.EPS, dtype=dtype)
    pmk.fitmixtureGP_(fresh, t.y[keep], TH, s2)
    _same_lists(model, o)
    _renumbered_lists(fresh._model, keep, o.sets)
    assert np.array_equal(model.n, [len(s) for s in o.sets]) and model.n[0] == 129 and model.removable()[0] == 0
    cond, ymax, k0s2 = o.cond2(), np.abs(t.y[keep]).max(), o.k0() + s2
    got = {}
    for noisy, (Yr, Vr) in zip((False, True), _blend_reference(dtype)):
        Y, V = pmk.loomixtureGP_blend(eta, t.root, t.RADIUS, t.DELTA, t.wth, noisy=noisy)
        assert Y.shape == (N,) and np.all(np.isfinite(Y)) and np.all(np.isfinite(V))
        got[("kept", noisy)] = BR.ratios(Y[keep], V[keep], Yr[keep], Vr[keep], cond, u, ymax, k0s2)
        got[("gone", noisy)] = BR.ratios(Y[G], V[G], Yr[G], Vr[G], cond, u, ymax, k0s2)
        Yf, Vf = pmk.loomixtureGP_blend(fresh, t.root, t.RADIUS, t.DELTA, t.wth, noisy=noisy)
        assert Yf.shape == (len(keep),)
        got[("fresh", noisy)] = BR.ratios(Yf, Vf, Yr[keep], Vr[keep], cond, u, ymax, k0s2)
    # ---- counts and items
    ototal, ostrip, multi, homeless = o.counts(t.RADIUS, t.DELTA)
    assert homeless == len(G) and multi >= 1 and 0 < ostrip < ototal
    home, regs, _ = o.plan(t.RADIUS, t.DELTA)
    q0 = pmk.DeviceQuery(model, t.X)
    assert q0.plan(t.RADIUS, t.DELTA) == ototal
    q0.items_fitted()
    fitted = q0.debug()
    q = pmk.DeviceQuery(model, t.X)
    total = q.plan(t.RADIUS, t.DELTA)
    nm, ns = q.items_loo(True)
    assert (total, ns, nm) == (ototal, ostrip, ototal - ostrip), (total, nm, ns, ototal, ostrip)
    dbg = q.debug()
    off, reg = dbg["item_offsets"], dbg["item_region"]
    _, var = model.loo_values()
    for j in range(N):
        assert list(reg[off[j]:off[j + 1]]) == [int(r) for r in regs[j]] + [int(home[j])], j
    for j in G:                                     # no patch holds it: every item is the fitted patch's, plus sigma2
        for k in range(off[j], off[j + 1]):
            assert o.row_of(int(reg[k]), int(j)) < 0
            if dtype == "f64":
                assert same_bits(dbg["item_u"][k], fitted["item_u"][k]), (j, k)
                assert same_bits(dbg["item_v"][k], fitted["item_v"][k] + s2), (j, k)
    seen = 0
    for j in keep:                                  # a member item's noisy variance IS the resident 1 / d_i
        assert o.row_of(int(home[j]), int(j)) >= 0, j
        for k in range(off[j], off[j + 1]):
            i = o.row_of(int(reg[k]), int(j))
            if i >= 0 and dtype == "f64":
                assert same_bits(dbg["item_v"][k], var[int(reg[k])][i]), (j, k)
            seen += i >= 0
    assert seen == nm
    # the fresh model plans the kept points alone
    qf = pmk.DeviceQuery(fresh._model, np.ascontiguousarray(t.X[keep]))
    ftotal = qf.plan(t.RADIUS, t.DELTA)
    fm, fs = qf.items_loo(True)
    ktotal, kstrip = _counts_at(o, t.RADIUS, t.DELTA, keep)
    assert (ftotal, fs, fm) == (ktotal, kstrip, ktotal - kstrip) and fm == nm
    _record(test="blend", dtype=dtype, cond2=cond, items=ototal, n_strip=ostrip, removed=len(G), bound=1.0,
            dY_latent=got[("kept", False)][0], dV_latent=got[("kept", False)][1],
            dY_noisy=got[("kept", True)][0], dV_noisy=got[("kept", True)][1],
            dY_latent_removed_points=got[("gone", False)][0], dV_latent_removed_points=got[("gone", False)][1],
            dY_noisy_removed_points=got[("gone", True)][0], dV_noisy_removed_points=got[("gone", True)][1],
            dY_latent_fresh=got[("fresh", False)][0], dV_latent_fresh=got[("fresh", False)][1],
            dY_noisy_fresh=got[("fresh", True)][0], dV_noisy_fresh=got[("fresh", True)][1])
    for key, (ry, rv) in got.items():
        assert ry <= 1.0 and rv <= 1.0, (key, ry, rv)


# ------------------------------------------------------------------------------------------ b. multi-output with a trend
def test_blended_leave_one_out_multi_after_a_removal():
    """loomixtureGP_blend_multi with R = 2 and a constant trend: the trend degree survives the removal, the target block
    and the weights do not.  The targets are set again with NaN in the rows of G: nobody reads them.  Against long-double
    refits with the trend at 20 kept points of patch 0, 18 other kept points and 6 points of G, in the units of
    tests/test_gpu_loo_blend_multi.py, both ratios <= 1; the fresh model beside it."""
    dtype = "f64"
    t, G, _ = RA.tree_oracle(dtype)
    s2, u, N = AC.SIGMA2[dtype], RR.U_OF[dtype], len(t.X)
    keep = _kept(N, G)
    Y = np.asfortranarray(RA.targets2(t.X))
    mo = RA.MultiOracle(t.X, t.X, Y, t.EPS, RA.hyper(dtype), "constant", t.LEVELS, G)
    eta = pmk.MixtureGPType.from_tree(t.root, t.X, t.EPS)
    pmk.fitmixtureGP_trend_(eta, Y, TH, s2, "constant")
    pmk.loomixtureGP_blend_multi(eta, t.root, t.RADIUS, t.DELTA, t.wth)
    pmk.removemixtureGP_(eta, G)
    model = eta._model
    assert eta.C_set is None and eta.beta_set is None
    with pytest.raises(pmk.PmkError, match="solve_multi has not run"):
        pmk.loomixtureGP_blend_multi(eta, t.root, t.RADIUS, t.DELTA, t.wth)
    with pytest.raises(pmk.PmkError, match="no multi-output targets"):
        model.solve_multi()
    Yn = Y.copy(order="F")
    Yn[G] = np.nan                                  # a removed point's value is read by nobody
    model.set_targets_multi_global(Yn)
    model.solve_multi()
    assert np.all(model.trend_info() == 0) and model.trend()[0][0].shape == (1, 2)        # the constant trend is still set
    assert all(np.all(np.isfinite(c)) for c in model.weights_multi()) and all(np.all(np.isfinite(b)) for b in model.trend()[0])
    for r in range(model.P):
        assert np.all(np.isfinite(TAA._packed_multi(model, r))), r
    fresh = pmk.MixtureGPType.from_tree(t.root, np.ascontiguousarray(t.X[keep]), t.EPS)
    pmk.fitmixtureGP_trend_(fresh, np.asfortranarray(Y[keep]), TH, s2, "constant")
    _same_lists(model, mo)
    _renumbered_lists(fresh._model, keep, mo.sets)
    mine, other, gone = RA.multi_points(mo, G)
    pts, MUr, Vr = mo.blend(_owth(t.RADIUS), mo.items(t.RADIUS, "ref", points=mine + other + gone))
    pts = np.array(pts)
    is_kept = ~np.isin(pts, G)
    assert is_kept.sum() == 38 and (~is_kept).sum() == 6
    cond, ymax, k0s2 = mo.cond2(), np.abs(Y[keep]).max(), mo.k0() + s2
    ototal, oother, _, homeless = mo.counts(t.RADIUS, t.DELTA)
    assert homeless == len(G)
    MU, V = pmk.loomixtureGP_blend_multi(eta, t.root, t.RADIUS, t.DELTA, t.wth)
    assert MU.shape == (N, 2) and np.all(np.isfinite(MU)) and np.all(np.isfinite(V))
    q = pmk.DeviceQuery(model, t.X)
    total = q.plan(t.RADIUS, t.DELTA)
    nm, no = q.items_loo_multi()
    assert (total, no, nm) == (ototal, oother, ototal - oother), (total, nm, no)
    MUf, Vf = pmk.loomixtureGP_blend_multi(fresh, t.root, t.RADIUS, t.DELTA, t.wth)
    at = np.searchsorted(keep, pts[is_kept])
    assert MUf.shape == (len(keep), 2) and np.array_equal(keep[at], pts[is_kept])
    got = dict(kept=MR.ratios(MU[pts[is_kept]], V[pts[is_kept]], MUr[is_kept], Vr[is_kept], cond, u, ymax, k0s2),
               gone=MR.ratios(MU[pts[~is_kept]], V[pts[~is_kept]], MUr[~is_kept], Vr[~is_kept], cond, u, ymax, k0s2),
               fresh=MR.ratios(MUf[at], Vf[at], MUr[is_kept], Vr[is_kept], cond, u, ymax, k0s2))
    _record(test="blend_multi", dtype=dtype, trend="constant", R=2, points=len(pts), cond2=cond, bound=1.0,
            dY=got["kept"][0], dV=got["kept"][1], dY_removed_points=got["gone"][0], dV_removed_points=got["gone"][1],
            dY_fresh=got["fresh"][0], dV_fresh=got["fresh"][1])
    for name, (ry, rv) in got.items():
        assert ry <= 1.0 and rv <= 1.0, (name, ry, rv)


# ------------------------------------------------------------------------------------------ c. the *_global setters
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_global_setters_after_a_removal_read_no_removed_value(dtype):
    """set_targets_global, set_diag_global and set_targets_multi_global gather through the rebuilt index list with n from
    the device descriptor: N values each with NaN at G, against the fresh model of the kept points given the kept values.
    Every packed buffer, padding included, and then the fit, bit for bit."""
    t, G, o = RA.tree_oracle(dtype)
    s2, N = AC.SIGMA2[dtype], len(t.X)
    keep = _kept(N, G)
    rng = np.random.default_rng(2020)
    y2 = 0.5 * np.cos(0.6 * t.X[:, 0]) - 0.3 * np.sin(0.5 * t.X[:, 1]) + 0.05 * t.X[:, 1]
    d = rng.uniform(0.0, 0.05, N)
    Y2 = np.asfortranarray(np.stack([y2, RA.targets2(t.X)[:, 1], np.sin(0.3 * t.X[:, 0] * t.X[:, 1])], 1))
    for a in (y2, d, Y2):
        a[G] = np.nan
    model = M.DeviceModel.from_tree(t.root, t.X, t.y, t.EPS, dtype=dtype)
    model.fit(TH, s2)
    assert model.remove_global(G) == int(RA.multiplicity(RA.tree_lists(t, t.X), N)[G].sum())
    _same_lists(model, o)
    model.set_targets_global(y2)
    model.set_diag_global(d)
    model.set_targets_multi_global(Y2)
    fresh = M.DeviceModel.from_tree(t.root, np.ascontiguousarray(t.X[keep]), np.ascontiguousarray(y2[keep]), t.EPS, dtype=dtype)
    fresh.set_diag_global(np.ascontiguousarray(d[keep]))
    fresh.set_targets_multi_global(np.asfortranarray(Y2[keep]))
    _renumbered_lists(fresh, keep, o.sets)
    for r in range(model.P):
        n = len(o.sets[r])
        for what in (0, 1, 2):
            a, b = TA._packed(model, r, what), TA._packed(fresh, r, what)
            assert a.shape == b.shape and not np.isnan(a).any() and np.array_equal(a, b), (r, what)
        blk = TAA._packed_multi(model, r)
        assert np.all(np.isfinite(blk)) and np.array_equal(blk, TAA._packed_multi(fresh, r)), r
        assert np.all(blk[n:] == 0.0) and np.all(blk[:, 3:] == 0.0) and np.all(TA._packed(model, r, 1)[n:] == 0.0), r
        if dtype == "f64":
            assert np.array_equal(TA._packed(model, r, 1)[:n], y2[o.sets[r]]) and np.array_equal(blk[:n, :3], Y2[o.sets[r]]), r
    for mdl in (model, fresh):
        mdl.fit(TH, s2)
    assert np.all(model.info() == 0) and np.array_equal(model.info(), fresh.info())
    for r, ((L, c, inv), (FL, Fc, Finv)) in enumerate(zip(TA._state(model), TA._state(fresh))):
        assert np.all(np.isfinite(L)) and np.all(np.isfinite(c)), r
        assert np.array_equal(L, FL) and np.array_equal(c, Fc) and np.array_equal(inv, Finv), r


# ------------------------------------------------------------------------------------------ d. query objects, gradients
def test_a_query_made_before_the_removal_serves_after_it():
    t, G, _ = RA.tree_oracle("f64")
    s2 = AC.SIGMA2["f64"]
    model = M.DeviceModel.from_tree(t.root, t.X, t.y, t.EPS)
    model.fit(TH, s2)
    model.set_targets_multi_global(t.y)
    model.solve_multi()
    q = M.DeviceQuery(model, t.Xq)
    total = q.plan(t.RADIUS, t.DELTA)
    before = TAA._all_stages(q, model, t.wth)
    assert model.remove_global(G) > len(G)
    assert np.all(model.info() == 0)
    model.set_targets_multi_global(t.y)
    model.solve_multi()
    after = TAA._all_stages(q, model, t.wth)                # the same object, not planned again
    assert q.total == total
    q2 = M.DeviceQuery(model, t.Xq)
    assert q2.plan(t.RADIUS, t.DELTA) == total
    new = TAA._all_stages(q2, model, t.wth)
    for key in before:
        assert same_bits(after[key], new[key]), key
        assert not same_bits(after[key], before[key]), key  # the stages ran again on the reduced factor
        assert np.all(np.isfinite(after[key])), key


def test_item_gradients_after_a_removal():
    """items_grad and items_vgrad with explicit items on the `consumers` case of tests/_remove_cases.py, with the queries
    per patch of test_consumers_of_the_padding_agree_with_a_fresh_model (at the rows that took the place of removed ones,
    at the last rows, and near them): L, c, the coordinates and their padding as the removal left them.  Against
    _grad_refs.item_grad_ref with the device's own weights and _vgrad_refs.PatchRef, the units and bounds of
    tests/test_gpu_grad.py and tests/test_gpu_vgrad.py, the removed model and the fresh one."""
    dtype, u = "f64", RR.U_OF["f64"]
    case, fams, s2 = {n: (c, f, s) for n, c, f, s in RC.all_cases(dtype)}["consumers"]
    P = case.P
    assert s2[0] == TV.SIGMA2[dtype]                         # TV._item_ratios builds its factor with it
    model = TA._fit(case.Xs, case.ys, fams, s2, dtype)
    assert np.all(model.remove(case.rows) == 0)
    fresh = TA._fit(case.Xr, case.yr, fams, s2, dtype)
    rng = np.random.default_rng(1990)
    root, _, _ = pmk.setuppartition(rng.uniform(-4, 4, (64, 2)), 4)                 # any tree of 8 leaves: the items name their regions
    xq = []
    for r in range(P):
        n1 = len(case.Xr[r])
        at = np.unique(np.clip(np.concatenate([case.rows[r][:3], [n1 - 1, n1 - 2, 0]]), 0, n1 - 1))
        near = case.Xr[r][rng.integers(n1, size=8 - len(at))] + rng.uniform(-0.2, 0.2, (8 - len(at), 2))
        xq.append(np.vstack([case.Xr[r][at], near]))
    xq = np.ascontiguousarray(np.vstack(xq))
    region = np.repeat(np.arange(P), 8).astype(np.int32)
    Yr = [np.stack([RC.target(x), 0.5 * x[:, 1] - 0.2 * x[:, 0] ** 2], 1) for x in case.Xr]
    got = {}
    for name, mdl in (("removed", model), ("fresh", fresh)):
        mdl.set_targets_multi(Yr)
        mdl.solve_multi()
        mdl.set_bsp(root, 0)
        q = TA._explicit_query(mdl, xq, region)
        q.items_multi_fitted(True)
        q.items_grad()
        q.items_vgrad()
        Gm, plane = q.item_grads()
        GV = q.item_vgrads()
        assert Gm.shape == (len(xq), 2, 2) and GV.shape == (len(xq), 2) and np.all(plane == -1)
        rg = TG._item_ratios(Gm, xq, region, case.Xr, mdl.weights_multi(), [OTH] * P, [None] * P, np.zeros(P), u)
        rv, kappa = TV._item_ratios(GV, xq, region, case.Xr, [OTH] * P, dtype, None, np.zeros(P, dtype=bool))
        got[name] = dict(grad=rg, vgrad=rv, kappa=kappa)
    _record(test="items", dtype=dtype, grad=got["removed"]["grad"], vgrad=got["removed"]["vgrad"],
            grad_fresh=got["fresh"]["grad"], vgrad_fresh=got["fresh"]["vgrad"], kappa=got["removed"]["kappa"],
            grad_bound=1.0, vgrad_bound=TV.RATIO_MAX)
    for name, g in got.items():
        assert g["kappa"] <= RC.KAPPA_MAX, (name, g)
        assert g["grad"] <= 1.0 and g["vgrad"] <= TV.RATIO_MAX, (name, g)


# ------------------------------------------------------------------------------------------ e. appends and removals mixed
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_appends_and_removals_mixed_on_one_tree_model(dtype):
    """remove_global, append_global, remove_global (old points and just-appended ones, one of two patches), append_global:
    two host routines rebuild the index list in turn.  After every step the lists (cached and read back), N, n, capacity
    and removable; at the end the packed buffers and a fit against the fresh from_tree model of the surviving points, and
    L and c within 10 units of the oracle."""
    t, steps = RA.mixed_steps(dtype)
    s2, n0 = AC.SIGMA2[dtype], len(t.X)
    model = M.DeviceModel.from_tree(t.root, t.X, t.y, t.EPS, dtype=dtype)
    model.fit(TH, s2)
    ld = np.array([RA.ld_of(int(n)) for n in model.n])
    assert np.array_equal(ld, model.n + model.capacity())
    nmax, N = model.n.copy(), n0
    for k, st in enumerate(steps):
        if st.kind == "remove":
            off, inds = model.patch_index()
            assert model.remove_global(st.points) == int(np.isin(inds, st.points).sum())
        else:
            first, items = model.append_global(*st.points)
            assert first == N and items == sum(len(s) for s in st.sets) - int(model.n.sum() - items)
        N = st.N
        assert np.all(model.info() == 0), k
        off, inds = _library_lists(model)
        for r, s in enumerate(st.sets):
            assert np.array_equal(inds[off[r]:off[r + 1]], s), (k, r)
        n = np.array([len(s) for s in st.sets])
        assert model.N == N and _library_N(model) == N
        assert np.array_equal(model.n, n) and np.array_equal(model.capacity(), ld - n), k
        assert np.array_equal(model.removable(), n - 128 * (ld // 128 - 1) - 1), k
        nmax = np.maximum(nmax, n)
        if k == 0:
            # a removed index is not given again: an append under one is refused, nothing changes
            j = int(st.points[0])
            h0 = TA._hash(model)
            rc, msg = TA._raw(model, t.X[j:j + 1], t.y[j:j + 1], [int(np.argmax([j in s for s in RA.tree_lists(t, t.X)]))], gidx=[j])
            assert rc == -3 and "item 0 has global index %d, outside N = %d" % (j, n0) in msg, (rc, msg)
            off2, inds2 = _library_lists(model)
            assert TA._hash(model) == h0 and np.array_equal(off2, off) and np.array_equal(inds2, inds)
            assert _library_N(model) == n0 and np.array_equal(model.capacity(), ld - n)
    last = steps[-1]
    surv = _kept(last.N, last.removed)
    fresh = M.DeviceModel.from_tree(t.root, np.ascontiguousarray(last.X[surv]), np.ascontiguousarray(last.y[surv]), t.EPS,
                                    dtype=dtype)
    fresh.fit(TH, s2)
    _renumbered_lists(fresh, surv, last.sets)
    worst = dict(L=0.0, c=0.0, L_fresh=0.0, c_fresh=0.0, kappa=0.0)
    for r, s in enumerate(last.sets):
        for what in (0, 1):
            assert np.array_equal(TA._packed(model, r, what), TA._packed(fresh, r, what)), (r, what)
        fit = O.fit_patch(OTH, last.X[s], last.y[s], s2, want_K=True)
        assert fit["info"] == 0
        kap = RR.kappa_of(fit["K"] + s2 * np.eye(len(s)))
        e = RR.unit(int(nmax[r]), dtype, kap, fit["L"])
        got = dict(L=RR.ratio(model.get(r, M.GET_L), fit["L"], e), c=RR.ratio(model.get(r, M.GET_C), fit["c_chol"], e),
                   L_fresh=RR.ratio(fresh.get(r, M.GET_L), fit["L"], e), c_fresh=RR.ratio(fresh.get(r, M.GET_C), fit["c_chol"], e),
                   kappa=kap)
        print("REMOVE_AFTER_PATCH", dtype, r, len(s), int(nmax[r]), {a: round(b, 4) for a, b in got.items()})
        for a, b in got.items():
            worst[a] = max(worst[a], b)
    _record(test="mixed", dtype=dtype, bound=RC.RATIO_MAX, **worst)
    assert worst["kappa"] <= RC.KAPPA_MAX
    assert worst["L"] <= RC.RATIO_MAX and worst["c"] <= RC.RATIO_MAX, worst
    model.fit(TH, s2)
    assert np.array_equal(model.info(), fresh.info())
    for r, ((L, c, inv), (FL, Fc, Finv)) in enumerate(zip(TA._state(model), TA._state(fresh))):
        assert np.array_equal(L, FL) and np.array_equal(c, Fc) and np.array_equal(inv, Finv), r


# ------------------------------------------------------------------------------------------ f. refusals on a tree model
def test_refusals_on_a_tree_model_keep_the_factor_and_the_index_list():
    t, G, _ = RA.tree_oracle("f64")
    s2 = AC.SIGMA2["f64"]
    model = M.DeviceModel.from_tree(t.root, t.X, t.y, t.EPS)
    model.fit(TH, s2)
    assert list(model.n[:2]) == [149, 122] and list(model.removable()[:2]) == [20, 121]
    h0 = TA._hash(model)
    off0, inds0 = (a.copy() for a in _library_lists(model))
    for (patch, rows), want, text in ((([0] * 21, np.arange(21)), -4, "patch 0 has 20 removable rows"),
                                      (([1] * 33, np.arange(33)), -5, "33 rows of patch 1 in one call")):
        rc, msg = TR._raw(model, patch, rows)
        assert rc == want and text in msg, (rc, msg)
        off, inds = _library_lists(model)
        assert TA._hash(model) == h0 and np.array_equal(off, off0) and np.array_equal(inds, inds0)
        assert _library_N(model) == len(t.X)
    # a valid call follows: the first entry of patch 0's list leaves every patch that holds it
    j = int(inds0[off0[0]])
    held = int((inds0 == j).sum())
    assert model.remove_global([j]) == held and np.all(model.info() == 0)
    off, inds = _library_lists(model)
    assert j not in inds and off[-1] == off0[-1] - held and TA._hash(model) != h0


# ------------------------------------------------------------------------------------------ the tree's own leaves
def test_remove_global_on_the_trees_own_leaves():
    """eps=None: the patches are the tree's leaves and a point is a row of its home leaf only.  The ends of every leaf's
    list leave; the lists, the packed buffers against a model of the reduced lists, and the blended leave-one-out at all
    200 points against refits of the reduced leaves (a removed point is predicted by leaves that never held it), the
    from_tree model of the kept points at eps = 0 beside it."""
    X, y, G, o = RA.leaves_case("f64")
    s2, u, radius, delta = AC.SIGMA2["f64"], RR.U_OF["f64"], 0.6, BR.DELTA
    keep = _kept(len(X), G)
    root, _, X_inds = pmk.setuppartition(X, RA.LEAF_LEVELS)
    eta = pmk.MixtureGPType.from_tree(root, X)
    pmk.fitmixtureGP_(eta, y, TH, s2)
    model = eta._model
    wth = pmk.Spline34KernelType(1 / radius)
    pmk.loomixtureGP_blend(eta, root, radius, delta, wth)
    pmk.removemixtureGP_(eta, G)
    assert model.N == len(X) and np.array_equal(model.n, [len(s) - 2 for s in X_inds])
    off, inds = _library_lists(model)
    for r, s in enumerate(o.sets):
        assert np.array_equal(inds[off[r]:off[r + 1]], s) and np.array_equal(s, np.setdiff1d(X_inds[r], G)), r
    fresh = M.DeviceModel([np.ascontiguousarray(X[s]) for s in o.sets], [y[s] for s in o.sets])
    fresh.fit(TH, s2)
    for r in range(model.P):
        for what in (0, 1):
            assert np.array_equal(TA._packed(model, r, what), TA._packed(fresh, r, what)), (r, what)
    Yr, Vr = o.blend_refit(_owth(radius), radius, None, delta)
    Y, V = pmk.loomixtureGP_blend(eta, root, radius, delta, wth)
    cond, ymax, k0s2 = o.cond2(), np.abs(y[keep]).max(), o.k0() + s2
    # beside it the tree model of the kept points: at eps = 0 the eps-sets of the kept points are the reduced leaves
    eta0 = pmk.MixtureGPType.from_tree(root, np.ascontiguousarray(X[keep]), 0.0)
    pmk.fitmixtureGP_(eta0, y[keep], TH, s2)
    _renumbered_lists(eta0._model, keep, o.sets)
    Yf, Vf = pmk.loomixtureGP_blend(eta0, root, radius, delta, wth)
    got = dict(kept=BR.ratios(Y[keep], V[keep], Yr[keep], Vr[keep], cond, u, ymax, k0s2),
               gone=BR.ratios(Y[G], V[G], Yr[G], Vr[G], cond, u, ymax, k0s2),
               fresh=BR.ratios(Yf, Vf, Yr[keep], Vr[keep], cond, u, ymax, k0s2))
    q = pmk.DeviceQuery(model, X)
    total = q.plan(radius, delta)
    nm, ns = q.items_loo(False)
    ototal, ostrip, _, homeless = o.counts(radius, delta)
    assert homeless == len(G) and (total, ns, nm) == (ototal, ostrip, len(keep)), (total, nm, ns)
    _record(test="leaves", dtype="f64", cond2=cond, removed=len(G), bound=1.0, dY=got["kept"][0], dV=got["kept"][1],
            dY_removed_points=got["gone"][0], dV_removed_points=got["gone"][1], dY_fresh=got["fresh"][0],
            dV_fresh=got["fresh"][1])
    for name, (ry, rv) in got.items():
        assert ry <= 1.0 and rv <= 1.0, (name, ry, rv)


# ------------------------------------------------------------------------------------------ g. a failed patch
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_info_of_a_failed_patch_that_names_a_row_left_is_kept(dtype):
    """the duplicate-point construction of tests/test_gpu_remove.py with the duplicate FIRST among the appended rows: patch 1
    fails at its row 34 of 35.  One row less leaves info = 34 = n' as it is (it names a leading minor that still exists), one
    more lowers it to n' = 33; the other patches keep every bit in both calls."""
    rng = np.random.default_rng(77)
    th = RC.FAMILIES["spline34"][0]
    Xs = [RC.rnd(rng.uniform(-10, 10, (n, 2)), dtype) for n in (20, 33, 12, 15)]
    ys = [RC.target(x) for x in Xs]
    model, _, info = M.fit_patches(Xs, ys, th, 0.0, dtype=dtype)
    assert np.all(info == 0)
    Xn = [np.zeros((0, 2)), np.vstack([Xs[1][:1], RC.rnd(rng.uniform(-6, 6, (1, 2)), dtype)]), np.zeros((0, 2)), np.zeros((0, 2))]
    info = model.append(Xn, [RC.target(x) for x in Xn])
    assert np.array_equal(info, [0, 34, 0, 0]) and model.n[1] == 35
    others = [[a.copy() for a in s] for s in TA._state(model)]
    X1 = np.vstack([Xs[1], Xn[1]])
    for rows, n1, want in (([3], 34, 34), ([0], 33, 33)):
        info = model.remove([[], rows, [], []])
        assert np.array_equal(info, [0, want, 0, 0]) and np.array_equal(model.n, [20, n1, 12, 15]), (rows, info)
        X1 = np.delete(X1, rows, axis=0)
        assert np.array_equal(model.X[1], X1)
        logdet, _ = model.evidence()
        assert np.isnan(logdet[1]) and np.all(np.isfinite(np.delete(logdet, 1)))
        state = TA._state(model)
        for r in (0, 2, 3):
            assert all(np.array_equal(a, b) for a, b in zip(state[r], others[r])), (rows, r)
