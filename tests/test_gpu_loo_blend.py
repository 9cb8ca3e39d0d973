"""Blended leave-one-out on the GPU: pmk_query_items_loo, pmk_predict_mixture_loo and the front-end functions over them.

The reference of the accuracy tests is the oracle's BRUTE FORCE (tests/_loo_blend_refs.py): every patch that holds point j
refitted without it, then the mixture queried at x_j.  Bounds: the solve's forward error, the convention of
tests/test_gpu_model_selection.py: |dY| <= cond_2 u max|y| and |dV| <= cond_2 u (k(0) + sigma2), cond_2 of the oracle's
U = K + sigma2 I maximised over the patches, u = 2^-53 for fp64 models and 2^-24 for fp32 models.  Item counts are
recomputed with the oracle, never written down.  The bit claims are fp64 only and have no tolerance.

Every measured ratio is printed before it is asserted ("measured {json}"); with PMK_WRITE_PROFILES=1 in the environment
the module also writes them to profiles/loo_blend_accuracy.json (the committed file is one such run on an MI355X).
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

import _loo_blend_refs as BR

pytestmark = pytest.mark.gpu

TH = pmk.Spline34KernelType(BR.A)
SIGMA2, DELTA, N = BR.SIGMA2, BR.DELTA, BR.N
UNIFORM = [(("s34", BR.A), SIGMA2)]
# four distinct (theta_r, sigma2_r), two families (test 4)
HYPER4 = [(("s34", 0.5), 1e-3), (("s34", 0.7), 2e-3), (("rq", 4.0), 5e-3), (("rq", 6.0), 1e-2)]
U = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "loo_blend_accuracy.json")
_MEASURED = []


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def _record(**kw):
    print("measured " + json.dumps(kw))
    _MEASURED.append(kw)


def _theta(h):
    return {"s34": pmk.Spline34KernelType, "rq": pmk.RationalQuadraticKernelType}[h[0]](h[1])


def _wth(radius, oracle=False):
    return O.kernel(O.SPLINE34, 1.0 / radius) if oracle else pmk.Spline34KernelType(1.0 / radius)


@pytest.fixture(scope="module")
def W():
    """the base workload, its tree, and lazily one oracle and one fitted device model per (eps, dtype)"""
    X, y = BR.workload()
    root, _, _ = pmk.setuppartition(X, BR.LEVELS)
    w = dict(X=X, y=y, root=root, oracle={}, model={})

    def oracle(eps, hyper=None):
        key = (eps, "uniform" if hyper is None else "hyper4")
        if key not in w["oracle"]:
            w["oracle"][key] = BR.Oracle(X, y, eps, UNIFORM if hyper is None else hyper)
        return w["oracle"][key]

    def model(eps, dtype="f64"):
        if (eps, dtype) not in w["model"]:
            m = pmk.DeviceModel.from_tree(root, X, y, eps=eps, dtype=dtype)
            m.fit(TH, SIGMA2)
            assert np.all(m.info() == 0)
            m.loo()
            off, inds = m.patch_index()
            for r, s in enumerate(oracle(eps).sets):       # the device's index lists are the oracle's
                assert np.array_equal(inds[off[r]:off[r + 1]], s), r
            w["model"][(eps, dtype)] = m
        return w["model"][(eps, dtype)]

    w["get_oracle"], w["get_model"] = oracle, model
    yield w
    if os.environ.get("PMK_WRITE_PROFILES") == "1":
        with open(PROFILE, "w") as f:
            json.dump(_MEASURED, f, indent=1)
            f.write("\n")


def _staged(m, X, radius, noisy=False, delta=DELTA):
    q = pmk.DeviceQuery(m, X)
    total = q.plan(radius, delta)
    nm, ns = q.items_loo(noisy)
    q.mix(_wth(radius))
    Y, V = q.fetch()
    return q, total, nm, ns, Y, V


def _check_counts(o, radius, total, nm, ns, eps):
    ototal, ostrip, multi, homeless = o.counts(radius)
    assert homeless == 0 and multi >= 1
    assert (total, ns) == (ototal, ostrip), (total, ns, ototal, ostrip)
    assert nm + ns == total
    if eps is not None and radius <= eps:
        assert ns == 0
    else:
        assert 0 < ns < total
    return multi


def _against_refits(W, eps, radius, dtype, test):
    o, m = W["get_oracle"](eps), W["get_model"](eps, dtype)
    _, total, nm, ns, Y, V = _staged(m, W["X"], radius)
    multi = _check_counts(o, radius, total, nm, ns, eps)
    Yr, Vr = o.blend_refit(_wth(radius, True), radius)
    cond = o.cond2()
    ry, rv = BR.ratios(Y, V, Yr, Vr, cond, U[dtype], np.abs(W["y"]).max(), o.k0() + SIGMA2)
    _record(test=test, eps=eps, radius=radius, dtype=dtype, items=total, n_member=nm, n_strip=ns, points_2_neighbours=multi,
            cond2=cond, dY_ratio_to_cond_u_maxy=ry, dV_ratio_to_cond_u_k0s2=rv, max_dY=float(np.abs(Y - Yr).max()),
            max_dV=float(np.abs(V - Vr).max()))
    assert ry <= 1.0, (eps, radius, dtype, ry)
    assert rv <= 1.0, (eps, radius, dtype, rv)
    return nm, ns, total


# ------------------------------------------------------------------------------------ 1. against refits, fp64
@pytest.mark.parametrize("eps, radius", BR.CASES)
def test_against_refits(W, eps, radius):
    """Yq and Vq of all 620 points against the brute force, both ratios <= 1.
    Measured on an MI355X (profiles/loo_blend_accuracy.json): Y at 0.013 .. 0.018 of its bound (max |dY| 3.4e-14), V at
    0.0017 .. 0.0029; the closed form on the CPU sits at 0.010 .. 0.012 and 0.0014 .. 0.0023."""
    _against_refits(W, eps, radius, "f64", "against_refits")


# ------------------------------------------------------------------------------------ 2. bits, fp64
def _row_lookup(m):
    """(offsets, inds, row_of): row_of(r, j) is the row of global point j in patch r, or -1"""
    off, inds = m.patch_index()

    def row_of(r, j):
        s = inds[off[r]:off[r + 1]]
        i = int(np.searchsorted(s, j))
        return i if i < len(s) and s[i] == j else -1
    return off, inds, row_of


def _expected_items(m, dbg, dbg_fitted, y, sigma2s, noisy):
    """per item in reference order: (member?, patch row, u, v) from numpy on pmk_model_get_loo for members and from
    pmk_query_items_fitted (+ sigma2 with noisy, one add) for the rest"""
    res, var = m.loo_values()
    _, _, row_of = _row_lookup(m)
    off, reg = dbg["item_offsets"], dbg["item_region"]
    T = len(reg)
    member, rows, u, v = np.zeros(T, bool), np.full(T, -1), np.empty(T), np.empty(T)
    for j in range(len(off) - 1):
        for k in range(off[j], off[j + 1]):
            r = int(reg[k])
            i = row_of(r, j)
            member[k], rows[k] = i >= 0, i
            if i >= 0:
                u[k] = y[j] - res[r][i]
                v[k] = var[r][i] if noisy else np.maximum(var[r][i] - sigma2s[r], 1e-12)
            else:
                u[k] = dbg_fitted["item_u"][k]
                v[k] = dbg_fitted["item_v"][k] + sigma2s[r] if noisy else dbg_fitted["item_v"][k]
    return member, rows, u, v


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("eps, radius", BR.CASES)
def test_item_bits_through_the_debug_view(W, eps, radius, noisy):
    m, X, y = W["get_model"](eps), W["X"], W["y"]
    q, total, nm, ns, Y, V = _staged(m, X, radius, noisy)
    dbg = q.debug()
    q2 = pmk.DeviceQuery(m, X)
    assert q2.plan(radius, DELTA) == total
    q2.items_fitted()
    dbg2 = q2.debug()
    assert np.array_equal(dbg["item_region"], dbg2["item_region"]) and np.array_equal(dbg["item_offsets"], dbg2["item_offsets"])
    member, rows, u, v = _expected_items(m, dbg, dbg2, y, [SIGMA2] * m.P, noisy)
    assert int(member.sum()) == nm and int((~member).sum()) == ns
    assert same_bits(dbg["item_u"][member], u[member]) and same_bits(dbg["item_v"][member], v[member])
    assert same_bits(dbg["item_u"][~member], u[~member]) and same_bits(dbg["item_v"][~member], v[~member])
    # a point with only its home item: weight 1, Yq and Vq are the item's
    off = dbg["item_offsets"]
    alone = np.nonzero(np.diff(off) == 1)[0]
    assert len(alone) > 0
    assert same_bits(Y[alone], dbg["item_u"][off[alone]]) and same_bits(V[alone], dbg["item_v"][off[alone]])
    # the edges, by name.  Items are (point, region); a patch row is an item only if the region is the point's home or
    # one of its neighbours, so for the eps-sets (eps > 0) not every row of every patch has one
    reg, item_point = dbg["item_region"], np.repeat(np.arange(N), np.diff(off))
    poff, pinds, _ = _row_lookup(m)
    seen = {}
    for r in range(m.P):
        n = int(m.n[r])
        for name, i in (("row 0", 0), ("row 127", 127), ("row 128", 128), ("row n-1", n - 1)):
            k = np.nonzero((reg == r) & (item_point == pinds[poff[r] + i]))[0]
            if len(k):
                assert member[k[0]] and rows[k[0]] == i
                assert same_bits(dbg["item_u"][k], u[k]) and same_bits(dbg["item_v"][k], v[k]), (r, name)
                seen.setdefault(name, []).append(r)
    print("edge rows with an item, per patch:", seen)
    if eps == 0.0:          # eps = 0: the sets are the leaves, every row is its point's home item
        assert all(len(seen.get(name, [])) == m.P for name in ("row 0", "row 127", "row 128", "row n-1")), seen
    else:                   # first / last entry of an index list, rows 127 / 128: each at least once
        assert all(name in seen for name in ("row 0", "row 127", "row 128", "row n-1")), seen
    for j in (0, N - 1):    # global points 0 and N - 1
        ks = np.arange(off[j], off[j + 1])
        assert member[ks[-1]]                          # the home item comes last, and the home set holds the point
        assert same_bits(dbg["item_u"][ks], u[ks]) and same_bits(dbg["item_v"][ks], v[ks]), j


# ------------------------------------------------------------------------------------ 3. the tree's own leaf lists
def test_leaf_lists_every_neighbour_item_goes_through_the_strips(W):
    """eps=None: every point is a member of exactly one patch (its home leaf), so n_member == N and every neighbour item
    is a strip item; accuracy against refits as in test 1"""
    nm, ns, total = _against_refits(W, None, 0.4, "f64", "leaf_lists")
    assert nm == N and ns == total - N and ns > 0


# ------------------------------------------------------------------------------------ 4. per-patch hyperparameters
def test_per_patch_hyperparameters(W):
    X, y, root = W["X"], W["y"], W["root"]
    eps, radius = 0.3, 0.6
    o = W["get_oracle"](eps, HYPER4)
    s2s = [h[1] for h in HYPER4]

    def run(sigma2s):
        m = pmk.DeviceModel.from_tree(root, X, y, eps=eps)
        m.fit_patches([_theta(h[0]) for h in HYPER4], sigma2s)
        assert np.all(m.info() == 0)
        m.loo()
        q, total, nm, ns, Y, V = _staged(m, X, radius)
        return m, q, total, nm, ns, Y, V

    m, q, total, nm, ns, Y, V = run(s2s)
    _check_counts(o, radius, total, nm, ns, eps)
    rng = np.random.default_rng(44)
    home, regs, _ = o.plan(radius)
    with_nb = [j for j in range(N) if len(regs[j]) >= 1]
    pts = sorted(set(rng.choice(N, 25, replace=False).tolist()) | set(with_nb[:15]))
    Yr, Vr = o.blend_refit(_wth(radius, True), radius, pts)
    cond = o.cond2()
    ry, rv = BR.ratios(Y[pts], V[pts], Yr, Vr, cond, U["f64"], np.abs(y).max(), o.k0() + max(s2s))
    _record(test="per_patch_hyper", eps=eps, radius=radius, dtype="f64", points=len(pts), cond2=cond,
            dY_ratio_to_cond_u_maxy=ry, dV_ratio_to_cond_u_k0s2=rv)
    assert ry <= 1.0 and rv <= 1.0, (ry, rv)
    # member v uses sigma2 of the item's OWN patch: numpy on pmk_model_get_loo with sigma2s[region]
    dbg = q.debug()
    q2 = pmk.DeviceQuery(m, X)
    q2.plan(radius, DELTA)
    q2.items_fitted()
    member, _, u, v = _expected_items(m, dbg, q2.debug(), y, s2s, False)
    assert same_bits(dbg["item_u"], u) and same_bits(dbg["item_v"], v)
    # ... and flipping one sigma2_r moves the items of patch r only
    flip = 2
    s2f = list(s2s)
    s2f[flip] = 7e-3
    _, qf, totalf, _, _, _, _ = run(s2f)
    dbf = qf.debug()
    assert totalf == total and np.array_equal(dbf["item_region"], dbg["item_region"])
    other = dbg["item_region"] != flip
    assert same_bits(dbf["item_u"][other], dbg["item_u"][other]) and same_bits(dbf["item_v"][other], dbg["item_v"][other])
    moved = dbf["item_v"][~other] != dbg["item_v"][~other]
    assert (~other).sum() > 0 and moved.all()


# ------------------------------------------------------------------------------------ 5. a failed patch
def test_a_failed_patch_gives_nan_to_its_points_only(W):
    X, y, root = W["X"], W["y"], W["root"]
    eps, radius, bad = 0.3, 0.6, 1
    good = W["get_model"](eps)
    qg, total, _, _, Yg, Vg = _staged(good, X, radius)
    off, inds = good.patch_index()
    count = np.bincount(inds, minlength=N)
    mine = inds[off[bad]:off[bad + 1]]
    only = mine[count[mine] == 1]                      # points that no other patch holds
    dg = np.zeros(N)
    dg[only[len(only) // 2]] = -3.0                    # pivot <= -2 there, in any precision (tests/test_gpu_breakdown.py)
    m = pmk.DeviceModel.from_tree(root, X, y, eps=eps)
    m.set_diag_global(dg)
    m.fit(TH, SIGMA2)
    info = m.info()
    assert info[bad] != 0 and np.all(np.delete(info, bad) == 0), info
    m.loo()
    q, totalb, nm, ns, Y, V = _staged(m, X, radius)
    dbg = q.debug()
    assert totalb == total
    o, reg = dbg["item_offsets"], dbg["item_region"]
    hit = np.array([bad in reg[o[j]:o[j + 1]] for j in range(N)])
    _, _, row_of = _row_lookup(m)
    strip_hit = sum(row_of(bad, j) < 0 for j in np.nonzero(hit)[0])      # points that reach the failed patch as non-members
    assert hit.any() and (~hit).any() and strip_hit > 0       # both routes into the failed patch are exercised
    assert np.isnan(Y[hit]).all() and np.isnan(V[hit]).all()
    assert same_bits(Y[~hit], Yg[~hit]) and same_bits(V[~hit], Vg[~hit])
    # the context stays usable
    _, _, _, _, Y2, V2 = _staged(good, X, radius)
    assert same_bits(Y2, Yg) and same_bits(V2, Vg)


# ------------------------------------------------------------------------------------ 6. refusals on the device
def test_refusals_return_their_status_and_a_good_call_follows(W):
    X, y, root = W["X"], W["y"], W["root"]
    L = pmk.lib()
    eps, radius = 0.3, 0.6
    good = W["get_model"](eps)

    def planned(m, Xq):
        q = pmk.DeviceQuery(m, Xq)
        q.plan(radius, DELTA)
        return q

    def refused(q, text, status=-3):
        assert L.pmk_query_items_loo(q.h, 0, None, None) == status
        assert text in L.pmk_last_error().decode(), L.pmk_last_error().decode()
        nm, ns = C.c_int64(), C.c_int64()
        qg = planned(good, X)                           # a good call succeeds
        assert L.pmk_query_items_loo(qg.h, 0, C.byref(nm), C.byref(ns)) == 0
        assert nm.value + ns.value == qg.total and ns.value > 0

    # not planned
    assert L.pmk_query_items_loo(pmk.DeviceQuery(good, X).h, 0, None, None) == -1
    # a list-route model
    sets = pmk.organizetrainingsets(root, BR.LEVELS, X, eps)[1]
    lists = pmk.DeviceModel([X[s] for s in sets], [y[s] for s in sets])
    lists.set_bsp(root, 0)
    lists.fit(TH, SIGMA2)
    lists.loo()
    refused(planned(lists, X), "pmk_model_create_from_bsp")
    # Nq = N - 1
    refused(planned(good, X[:-1].copy()), "%d points" % (N - 1))
    # a shard
    shard = pmk.DeviceModel.from_tree(root, X, y, eps=eps, leaf_base=2, P=2)
    shard.fit(TH, SIGMA2)
    shard.loo()
    refused(planned(shard, X), "2 of 4 leaves")
    # before pmk_model_loo, and after a new fit without it
    fresh = pmk.DeviceModel.from_tree(root, X, y, eps=eps)
    fresh.fit(TH, SIGMA2)
    qf = planned(fresh, X)
    refused(qf, "pmk_model_loo has not run")
    fresh.loo()
    assert L.pmk_query_items_loo(qf.h, 0, None, None) == 0
    fresh.fit(TH, SIGMA2)
    refused(qf, "pmk_model_loo has not run")
    Y = np.empty(N)
    wd = _wth(radius).desc()
    assert L.pmk_predict_mixture_loo(fresh.h, C.byref(wd), X.ctypes.data_as(C.POINTER(C.c_double)), radius, DELTA, 0,
                                     Y.ctypes.data_as(C.POINTER(C.c_double)), None) == -3
    # the front end refuses the same states without reaching the library
    with pytest.raises(_lib.PmkError):
        qf.items_loo()


# ------------------------------------------------------------------------------------ 7. reuse
def test_one_query_replanned_gives_the_bits_of_fresh_queries(W):
    """0.6 -> 0.25 -> 0.6 on one query object: the inner query is created, skipped (empty compaction) and reused"""
    m, X = W["get_model"](0.3), W["X"]
    fresh = {r: _staged(m, X, r) for r in (0.6, 0.25)}
    q = pmk.DeviceQuery(m, X)
    for r in (0.6, 0.25, 0.6):
        total = q.plan(r, DELTA)
        nm, ns = q.items_loo()
        q.mix(_wth(r))
        Y, V = q.fetch()
        _, ftotal, fnm, fns, FY, FV = fresh[r]
        assert (total, nm, ns) == (ftotal, fnm, fns)
        assert (ns == 0) == (r == 0.25)
        assert same_bits(Y, FY) and same_bits(V, FV), r
        assert same_bits(q.debug()["item_u"], fresh[r][0].debug()["item_u"])


# ------------------------------------------------------------------------------------ 8. inputs and helpers
def test_device_inputs_the_one_shot_and_the_module_functions(W):
    import torch
    X, y, root = W["X"], W["y"], W["root"]
    eps, radius = 0.3, 0.6
    m = W["get_model"](eps)
    _, _, _, _, Yh, Vh = _staged(m, X, radius)
    Xd = torch.from_numpy(X).cuda()
    buf = torch.full((2, N + 8), -12345.678, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    q = pmk.DeviceQuery(m, Xd)
    assert q.Xq is None and q.Nq == N
    q.plan(radius, DELTA)
    q.items_loo()
    q.mix(_wth(radius))
    q.fetch_into(buf[0, :N], buf[1, :N])
    m.ctx.synchronize()
    got = buf.cpu().numpy()
    assert same_bits(got[0, :N], Yh) and same_bits(got[1, :N], Vh) and np.all(got[:, N:] == -12345.678)
    # the one-shot call
    Y1, V1 = np.empty(N), np.empty(N)
    wd = _wth(radius).desc()
    dp = C.POINTER(C.c_double)
    _lib.check(pmk.lib().pmk_predict_mixture_loo(m.h, C.byref(wd), X.ctypes.data_as(dp), radius, DELTA, 0,
                                                 Y1.ctypes.data_as(dp), V1.ctypes.data_as(dp)), "pmk_predict_mixture_loo")
    assert same_bits(Y1, Yh) and same_bits(V1, Vh)
    # the module functions on an eta built from the tree
    eta = pmk.MixtureGPType.from_tree(root, X, eps=eps)
    pmk.fitmixtureGP_(eta, y, TH, SIGMA2)
    mu, var = pmk.loomixtureGP_blend(eta, root, radius, DELTA, _wth(radius))          # runs loo() itself, X from the model
    assert same_bits(mu, Yh) and same_bits(var, Vh)
    cands = [(0.25, DELTA, _wth(0.25)), (0.6, DELTA, _wth(0.6)), (0.6, DELTA, pmk.Spline34KernelType(3.0)), (0.9, DELTA, _wth(0.9))]
    scores, best = pmk.selectblendGP_(eta, root, y, cands)
    want = []
    for r, d, w in cands:
        qs = pmk.DeviceQuery(eta._model, X)
        qs.plan(r, d)
        qs.items_loo(True)
        qs.mix(w)
        mu, var = qs.fetch()
        want.append(M.loo_log_pseudo_likelihood(y - mu, var))
    print("selectblendGP_ scores:", scores, "best", best)
    assert same_bits(scores, np.array(want)) and best == int(np.argmax(want)) and np.all(np.isfinite(scores))


# ------------------------------------------------------------------------------------ 9. fp32
@pytest.mark.parametrize("eps, radius", BR.CASES)
def test_against_refits_fp32(W, eps, radius):
    """test 1 on an fp32 model with u = 2^-24; no bit claims.  Measured on an MI355X: Y at 0.034 .. 0.055 of its bound, V
    at 0.0034 .. 0.0066."""
    _against_refits(W, eps, radius, "f32", "against_refits_fp32")
