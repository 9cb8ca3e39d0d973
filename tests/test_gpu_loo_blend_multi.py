"""Blended leave-one-out of the multi-output path on the GPU: pmk_query_items_loo_multi, pmk_predict_mixture_loo_multi,
pmk_query_get_items_multi and the front-end functions over them, for R target columns with and without a trend.

The reference of the accuracy tests is BRUTE FORCE (tests/_loo_blend_multi_refs.py): every patch that holds point j fitted
again without it, the GLS drift included, then the blended predictor at x_j; long double where there is a trend, the oracle
otherwise.  Bounds: the solve's forward error, the convention of tests/test_gpu_loo_blend.py: |dY| <= cond_2 u max|Y| and
|dV| <= cond_2 u (k(0) + sigma2), cond_2 of the oracle's U = K + sigma2 I maximised over the patches, u = 2^-53 for fp64
models and 2^-24 for fp32 models; fp32 with a trend has tests/test_gpu_trend.py's margin for summation order, 10 x the
larger of that unit and what the fp64 scipy closed form achieves in it.  Item counts are recomputed with the oracle, never
written down.  The bit claims are fp64 only and have no tolerance.

Every measured ratio is printed before it is asserted ("measured {json}"); with PMK_WRITE_PROFILES=1 in the environment
the module also writes them to profiles/loo_blend_multi_accuracy.json (the committed file is one such run on an MI355X:
fp64 at most 0.0046 of the bound of the means and 0.0047 of that of the variances, fp32 0.013 and 0.0068, with a trend as
without one).
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
import _loo_blend_multi_refs as MR

pytestmark = pytest.mark.gpu

TH = pmk.Spline34KernelType(BR.A)
SIGMA2, DELTA, N = BR.SIGMA2, BR.DELTA, BR.N
UNIFORM = [(("s34", BR.A), SIGMA2)]
# four distinct (theta_r, sigma2_r), two families (tests/test_gpu_loo_blend.py)
HYPER4 = [(("s34", 0.5), 1e-3), (("s34", 0.7), 2e-3), (("rq", 4.0), 5e-3), (("rq", 6.0), 1e-2)]
U = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "loo_blend_multi_accuracy.json")
_MEASURED = []
_dp = C.POINTER(C.c_double)


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


def _build(root, X, Y, eps, trend, dtype="f64", hyper=None, diag=None, ctx=None):
    """tree model -> fit -> R target columns -> trend -> solve -> loo"""
    m = pmk.DeviceModel.from_tree(root, X, np.ascontiguousarray(Y[:, 0]), eps=eps, dtype=dtype, ctx=ctx)
    if diag is not None:
        m.set_diag_global(diag)
    if hyper is None:
        m.fit(TH, SIGMA2)
    else:
        m.fit_patches([_theta(h[0]) for h in hyper], [h[1] for h in hyper])
    m.set_targets_multi_global(np.asfortranarray(Y))
    m.set_trend(trend)
    m.solve_multi()
    m.loo()
    return m


@pytest.fixture(scope="module")
def W():
    """the workload with 3 target columns, its tree, and lazily one oracle and one device model per setting"""
    X, Y = MR.targets(3)
    root, _, _ = pmk.setuppartition(X, BR.LEVELS)
    w = dict(X=X, Y=Y, root=root, oracle={}, model={}, ref={})

    def oracle(eps, trend, hyper=None):
        key = (eps, trend, "uniform" if hyper is None else "hyper4")
        if key not in w["oracle"]:
            w["oracle"][key] = MR.MultiOracle(X, Y, eps, UNIFORM if hyper is None else hyper, trend)
        return w["oracle"][key]

    def model(eps, trend, dtype="f64"):
        if (eps, trend, dtype) not in w["model"]:
            m = _build(root, X, Y, eps, trend, dtype)
            assert np.all(m.info() == 0) and np.all(m.trend_info() == 0)
            off, inds = m.patch_index()
            for r, s in enumerate(oracle(eps, trend).sets):    # the device's index lists are the oracle's
                assert np.array_equal(inds[off[r]:off[r + 1]], s), r
            w["model"][(eps, trend, dtype)] = m
        return w["model"][(eps, trend, dtype)]

    def reference(eps, trend, radius):
        """(MU, V, MU of the fp64 closed form, V of it) at all points, computed once"""
        if (eps, trend, radius) not in w["ref"]:
            o = oracle(eps, trend)
            _, MUr, Vr = o.blend(_wth(radius, True), o.items(radius, "ref"))
            _, MUc, Vc = o.blend(_wth(radius, True), o.items(radius, "closed64"))
            w["ref"][(eps, trend, radius)] = (MUr, Vr, MUc, Vc)
        return w["ref"][(eps, trend, radius)]

    w["get_oracle"], w["get_model"], w["get_reference"] = oracle, model, reference
    yield w
    if os.environ.get("PMK_WRITE_PROFILES") == "1":
        with open(PROFILE, "w") as f:
            json.dump(_MEASURED, f, indent=1)
            f.write("\n")


def _staged(m, X, radius, noisy=False, variance=True, delta=DELTA):
    q = pmk.DeviceQuery(m, X)
    total = q.plan(radius, delta)
    nm, no = q.items_loo_multi(noisy, variance)
    q.mix_multi(_wth(radius))
    MU, V = q.fetch_multi(m.R)
    return q, total, nm, no, MU, V


def _check_counts(o, radius, total, nm, no, eps):
    ototal, oother, multi, homeless = o.counts(radius)
    assert homeless == 0 and multi >= 1
    assert (total, no) == (ototal, oother), (total, no, ototal, oother)
    assert nm + no == total
    if eps is not None and radius <= eps:
        assert no == 0
    else:
        assert 0 < no < total
    return multi


# ------------------------------------------------------------------------------------ 1. against refits
def _against_refits(W, eps, radius, trend, dtype, test):
    o, m = W["get_oracle"](eps, trend), W["get_model"](eps, trend, dtype)
    _, total, nm, no, MU, V = _staged(m, W["X"], radius)
    multi = _check_counts(o, radius, total, nm, no, eps)
    MUr, Vr, MUc, Vc = W["get_reference"](eps, trend, radius)
    cond, ymax, k0s2 = o.cond2(), np.abs(W["Y"]).max(), o.k0() + SIGMA2
    ry, rv = MR.ratios(MU, V, MUr, Vr, cond, U[dtype], ymax, k0s2)
    cy, cv = MR.ratios(MUc, Vc, MUr, Vr, cond, U[dtype], ymax, k0s2)
    by = bv = 1.0
    if dtype == "f32" and trend is not None:        # the margin of tests/test_gpu_trend.py for summation order
        by, bv = 10.0 * max(1.0, cy), 10.0 * max(1.0, cv)
    _record(test=test, eps=eps, radius=radius, trend=trend, dtype=dtype, items=total, n_member=nm, n_other=no,
            points_2_neighbours=multi, cond2=cond, dY_ratio_to_cond_u_maxY=ry, dV_ratio_to_cond_u_k0s2=rv,
            fp64_closed_form_dY_ratio=cy, fp64_closed_form_dV_ratio=cv, bound_dY=by, bound_dV=bv,
            max_dY=float(np.abs(MU - MUr).max()), max_dV=float(np.abs(V - Vr).max()))
    assert ry <= by, (eps, radius, trend, dtype, ry)
    assert rv <= bv, (eps, radius, trend, dtype, rv)


@pytest.mark.parametrize("trend", MR.TRENDS)
@pytest.mark.parametrize("eps, radius", BR.CASES)
def test_against_refits(W, eps, radius, trend):
    """MU (3 columns) and V of all 620 points against the brute force, both ratios <= 1.
    Measured on an MI355X (profiles/loo_blend_multi_accuracy.json): at most 0.0046 and 0.0047; the closed form on the CPU sits at 0.003 .. 0.006
    of the bound of the means and 0.002 .. 0.0025 of that of the variances."""
    _against_refits(W, eps, radius, trend, "f64", "against_refits")


@pytest.mark.parametrize("trend", MR.TRENDS)
@pytest.mark.parametrize("eps, radius", BR.CASES)
def test_against_refits_fp32(W, eps, radius, trend):
    """the same on fp32 models with u = 2^-24: <= 1 without a trend; with a trend <= 10 x max(1, the fp64 scipy closed
    form's ratio in the same unit) (the closed form is far below 1 in this unit, so the bound is 10).  No bit claims.
    Measured on an MI355X: at most 0.013 and 0.0066 without a trend, 0.013 and 0.0068 with one."""
    _against_refits(W, eps, radius, trend, "f32", "against_refits_fp32")


# ------------------------------------------------------------------------------------ 2. bits, fp64
def _row_lookup(m):
    off, inds = m.patch_index()

    def row_of(r, j):
        s = inds[off[r]:off[r + 1]]
        i = int(np.searchsorted(s, j))
        return i if i < len(s) and s[i] == j else -1
    return row_of


def _expected_items(m, dbg, fitted, Y, sigma2s, noisy, variance=True):
    """per item in reference order: member?, U [T, R] and v [T] from numpy on pmk_model_get_loo_multi for the members and
    from pmk_query_items_multi_fitted's download (+ sigma2 with noisy, one add) for the rest"""
    RES, var = m.loo_values_multi()
    row_of = _row_lookup(m)
    off, reg = dbg["item_offsets"], dbg["item_region"]
    T = len(reg)
    member, Ue, ve = np.zeros(T, bool), np.empty((T, m.R)), np.empty(T)
    for j in range(len(off) - 1):
        for k in range(off[j], off[j + 1]):
            r = int(reg[k])
            i = row_of(r, j)
            member[k] = i >= 0
            if i >= 0:
                Ue[k] = Y[j] - RES[r][i]
                ve[k] = var[r][i] if noisy else np.maximum(var[r][i] - sigma2s[r], 1e-12)
            else:
                Ue[k] = fitted[0][k]
                if variance:
                    ve[k] = fitted[1][k] + sigma2s[r] if noisy else fitted[1][k]
    return member, Ue, ve


def _fitted_items(m, X, radius, total, variance=True):
    q2 = pmk.DeviceQuery(m, X)
    assert q2.plan(radius, DELTA) == total
    q2.items_multi_fitted(variance)
    return q2, q2.item_values_multi()


def _check_item_bits(m, X, Y, radius, noisy, sigma2s):
    q, total, nm, no, MU, V = _staged(m, X, radius, noisy)
    dbg = q.debug()
    q2, fitted = _fitted_items(m, X, radius, total)
    dbg2 = q2.debug()
    assert np.array_equal(dbg["item_region"], dbg2["item_region"]) and np.array_equal(dbg["item_offsets"], dbg2["item_offsets"])
    member, Ue, ve = _expected_items(m, dbg, fitted, Y, sigma2s, noisy)
    Ug, vg = q.item_values_multi()
    assert Ug.shape == (total, m.R) and vg.shape == (total,)
    assert int(member.sum()) == nm and int((~member).sum()) == no
    assert same_bits(Ug[member], Ue[member]) and same_bits(vg[member], ve[member])
    assert same_bits(Ug[~member], Ue[~member]) and same_bits(vg[~member], ve[~member])
    # a point with only its home item: weight 1, its row of MU and its V are the item's
    off = dbg["item_offsets"]
    alone = np.nonzero(np.diff(off) == 1)[0]
    assert len(alone) > 0
    assert same_bits(MU[alone], Ug[off[alone]]) and same_bits(V[alone], vg[off[alone]])
    return nm, no


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("trend", [None, "linear"])
@pytest.mark.parametrize("eps, radius", BR.CASES)
def test_item_bits_through_get_items_multi(W, eps, radius, trend, noisy):
    m = W["get_model"](eps, trend)
    nm, no = _check_item_bits(m, W["X"], W["Y"], radius, noisy, [SIGMA2] * m.P)
    assert (no == 0) == (radius <= eps)


@pytest.mark.parametrize("noisy", [False, True])
def test_item_bits_with_per_patch_hyperparameters(W, noisy):
    """member v uses sigma2 of the item's OWN patch, and so does the noisy add of a non-member"""
    m = _build(W["root"], W["X"], W["Y"], 0.3, "linear", hyper=HYPER4)
    assert np.all(m.info() == 0) and np.all(m.trend_info() == 0)
    nm, no = _check_item_bits(m, W["X"], W["Y"], 0.6, noisy, [h[1] for h in HYPER4])
    assert nm > 0 and no > 0


# ------------------------------------------------------------------------------------ 3. R and column isolation
@pytest.mark.parametrize("R, trend", [(1, None), (16, None), (1, "linear"), (13, "linear")])
def test_other_numbers_of_columns(W, R, trend):
    """R = 1 and R = 16 - q (R = 3 is test 1) against the fp64 scipy closed form at every 7th point: that form sits at
    0.006 / 0.0025 of the bounds against refits (tests/test_loo_blend_multi_abi.py), so the bound of test 1 stays 1."""
    eps, radius = 0.3, 0.6
    X, Y = MR.targets(R)
    o = MR.MultiOracle(X, Y, eps, UNIFORM, trend)
    m = _build(W["root"], X, Y, eps, trend)
    assert np.all(m.info() == 0) and np.all(m.trend_info() == 0)
    _, total, nm, no, MU, V = _staged(m, X, radius)
    _check_counts(o, radius, total, nm, no, eps)
    assert MU.shape == (N, R)
    pts, MUc, Vc = o.blend(_wth(radius, True), o.items(radius, "closed64", points=list(range(0, N, 7))))
    ry, rv = MR.ratios(MU[pts], V[pts], MUc, Vc, o.cond2(), U["f64"], np.abs(Y).max(), o.k0() + SIGMA2)
    _record(test="columns", R=R, trend=trend, eps=eps, radius=radius, points=len(pts), dY_ratio_to_cond_u_maxY=ry,
            dV_ratio_to_cond_u_k0s2=rv)
    assert ry <= 1.0 and rv <= 1.0, (R, trend, ry, rv)


@pytest.mark.parametrize("trend", [None, "linear"])
def test_changing_one_column_leaves_the_others_bits(W, trend):
    eps, radius = 0.3, 0.6
    X, Y = W["X"], W["Y"]
    m = _build(W["root"], X, Y, eps, trend)
    _, _, _, _, MU0, V0 = _staged(m, X, radius)
    Y2 = np.asfortranarray(Y.copy())
    Y2[:, 1] = np.cos(0.9 * X[:, 0]) - 0.3 * X[:, 1]
    m.set_targets_multi_global(Y2)
    m.solve_multi()
    _, _, _, _, MU1, V1 = _staged(m, X, radius)
    assert same_bits(MU1[:, 0], MU0[:, 0]) and same_bits(MU1[:, 2], MU0[:, 2]) and same_bits(V1, V0)
    assert np.abs(MU1[:, 1] - MU0[:, 1]).max() > 0.1


def test_one_column_without_a_trend_agrees_with_the_single_output_path(W):
    """the two solves differ in operation order: no bit claim, the bound of test 1 (both sit far below it)"""
    eps, radius = 0.3, 0.6
    X, Y = W["X"], W["Y"]
    y = np.ascontiguousarray(Y[:, 0])
    m = _build(W["root"], X, y[:, None], eps, None)
    _, _, _, _, MU, V = _staged(m, X, radius)
    q = pmk.DeviceQuery(m, X)
    q.plan(radius, DELTA)
    q.items_loo()
    q.mix(_wth(radius))
    Ys, Vs = q.fetch()
    o = W["get_oracle"](eps, None)
    ry, rv = MR.ratios(MU[:, 0], V, Ys, Vs, o.cond2(), U["f64"], np.abs(y).max(), o.k0() + SIGMA2)
    _record(test="single_output_agreement", eps=eps, radius=radius, dY_ratio_to_cond_u_maxY=ry, dV_ratio_to_cond_u_k0s2=rv)
    assert ry <= 1.0 and rv <= 1.0, (ry, rv)


# ------------------------------------------------------------------------------------ 4. mean-only
def _stage_recorded(ctx, stage):
    try:
        ctx.timer_ms(stage)
        return True
    except pmk.PmkError:
        return False


@pytest.mark.parametrize("trend", [None, "linear"])
def test_mean_only(W, trend):
    """on a context of its own, so that the stage timers show what ran.  The stage "items" is recorded by
    pmk_query_items and pmk_query_items_fitted only: on this path the strip kernel, when it runs, runs inside the stage
    "items_multi", so the absence of "items" holds with the variance as well (asserted below) and does not by itself show
    that a mean-only run launched no strip kernel.  That rests on the library's code (the strips are launched only under
    want_var); what is observable here is that the means have the bits of the run with the variance, that no variance
    can be fetched, and which stages were entered."""
    X, Y = W["X"], W["Y"]
    eps = 0.3
    ctx = pmk.Context(0)
    ctx.enable_timers(True)
    m = _build(W["root"], X, Y, eps, trend, ctx=ctx)
    # radius <= eps: every item is a lookup, with or without the variance
    for variance in (True, False):
        q, total, nm, no, MU, V = _staged(m, X, 0.25, variance=variance)
        assert no == 0 and nm == total and (V is None) == (not variance)
    assert _stage_recorded(ctx, "loo_items_multi")
    for stage in ("items", "items_multi", "trend_items"):
        assert not _stage_recorded(ctx, stage), stage
    # radius > eps, mean-only: the non-members cost the means kernel; no strip kernel runs
    _, total, nm, no, MU0, V0 = _staged(m, X, 0.6, variance=False)
    assert no > 0 and V0 is None
    assert _stage_recorded(ctx, "items_multi") and not _stage_recorded(ctx, "items")
    assert _stage_recorded(ctx, "trend_items") == (trend is not None)
    q, _, _, _, MU1, V1 = _staged(m, X, 0.6, variance=True)
    assert same_bits(MU0, MU1) and V1 is not None and np.all(np.isfinite(V1))
    assert not _stage_recorded(ctx, "items")              # with the strips too: this stage cannot tell the two runs apart
    # after a mean-only run the library refuses Vq and the per-item v
    qm, _, _, _, _, _ = _staged(m, X, 0.6, variance=False)
    L = pmk.lib()
    Yq, Vq = np.empty((N, 3), order="F"), np.empty(N)
    assert L.pmk_query_fetch_multi(qm.h, Yq.ctypes.data_as(_dp), N, Vq.ctypes.data_as(_dp)) == -3
    assert "Vq was not computed" in L.pmk_last_error().decode()
    Ui = np.empty((qm.total, 3))
    assert L.pmk_query_get_items_multi(qm.h, Ui.ctypes.data_as(_dp), 3, Vq.ctypes.data_as(_dp)) == -3
    Um, vm = qm.item_values_multi()
    assert vm is None and same_bits(Um, q.item_values_multi()[0])
    ctx.synchronize()


# ------------------------------------------------------------------------------------ 5. failed and flagged patches
def test_a_failed_patch_gives_nan_to_its_points_only(W):
    X, Y, root = W["X"], W["Y"], W["root"]
    eps, radius, bad, trend = 0.3, 0.6, 1, "linear"
    good = W["get_model"](eps, trend)
    _, total, _, _, MUg, Vg = _staged(good, X, radius)
    off, inds = good.patch_index()
    count = np.bincount(inds, minlength=N)
    mine = inds[off[bad]:off[bad + 1]]
    only = mine[count[mine] == 1]                      # points that no other patch holds
    dg = np.zeros(N)
    dg[only[len(only) // 2]] = -3.0                    # pivot <= -2 there, in any precision (tests/test_gpu_breakdown.py)
    m = _build(root, X, Y, eps, trend, diag=dg)
    info = m.info()
    assert info[bad] != 0 and np.all(np.delete(info, bad) == 0), info
    assert np.all(m.trend_info() == 0)
    q, totalb, nm, no, MU, V = _staged(m, X, radius)
    dbg = q.debug()
    assert totalb == total
    o, reg = dbg["item_offsets"], dbg["item_region"]
    hit = np.array([bad in reg[o[j]:o[j + 1]] for j in range(N)])
    row_of = _row_lookup(m)
    other_hit = sum(row_of(bad, j) < 0 for j in np.nonzero(hit)[0])      # points that reach the failed patch as non-members
    assert hit.any() and (~hit).any() and other_hit > 0 and other_hit < hit.sum()       # both routes are exercised
    assert np.isnan(MU[hit]).all() and np.isnan(V[hit]).all()
    assert same_bits(MU[~hit], MUg[~hit]) and same_bits(V[~hit], Vg[~hit])
    # the mean-only run as well
    _, _, _, _, MUm, _ = _staged(m, X, radius, variance=False)
    assert np.isnan(MUm[hit]).all() and same_bits(MUm[~hit], MUg[~hit])


def test_a_flagged_patch_gives_nan_to_its_points_only(W):
    """tinfo != 0: on the tree's own leaf lists (eps=None keeps the index lists whatever the coordinates are) the second
    coordinate of every point of one leaf is set to 0, so column 3 of that patch's H, and pivot 3 of its G, are exactly
    zero under the linear trend.  No model exists in which this patch is good and the others see the same numbers (the
    constant trend changes every patch), so the other queries are held to their own items' bits, as in test 2."""
    Y, root = W["Y"], W["root"]
    radius, bad = 0.4, 2
    X = W["X"].copy()
    probe = pmk.DeviceModel.from_tree(root, X, np.ascontiguousarray(Y[:, 0]), eps=None)
    off, inds = probe.patch_index()
    X[inds[off[bad]:off[bad + 1]], 1] = 0.0
    m = _build(root, X, Y, None, "linear")
    assert np.all(m.info() == 0)
    flags = m.trend_info()
    assert flags[bad] == 3 and np.all(np.delete(flags, bad) == 0), flags
    for noisy in (False, True):
        q, total, nm, no, MU, V = _staged(m, X, radius, noisy)
        dbg = q.debug()
        o, reg = dbg["item_offsets"], dbg["item_region"]
        hit = np.array([bad in reg[o[j]:o[j + 1]] for j in range(N)])
        row_of = _row_lookup(m)
        other_hit = sum(row_of(bad, j) < 0 for j in np.nonzero(hit)[0])
        assert hit.any() and (~hit).any() and 0 < other_hit < hit.sum()
        assert np.isnan(MU[hit]).all() and np.isnan(V[hit]).all()
        assert np.isfinite(MU[~hit]).all() and np.isfinite(V[~hit]).all()
        # every item outside the flagged patch keeps its bits; every item inside it is NaN
        _, fitted = _fitted_items(m, X, radius, total)
        member, Ue, ve = _expected_items(m, dbg, fitted, Y, [SIGMA2] * m.P, noisy)
        Ug, vg = q.item_values_multi()
        inside = reg == bad
        assert np.isnan(Ug[inside]).all() and np.isnan(vg[inside]).all()
        assert same_bits(Ug[~inside], Ue[~inside]) and same_bits(vg[~inside], ve[~inside])
        alone = np.nonzero((np.diff(o) == 1) & ~hit)[0]
        assert len(alone) > 0
        assert same_bits(MU[alone], Ug[o[alone]]) and same_bits(V[alone], vg[o[alone]])


# ------------------------------------------------------------------------------------ 6. state
def test_stale_states_are_refused_with_their_messages(W):
    X, Y, root = W["X"], W["Y"], W["root"]
    L = pmk.lib()
    eps, radius = 0.3, 0.6
    m = _build(root, X, Y, eps, None)
    q = pmk.DeviceQuery(m, X)
    q.plan(radius, DELTA)
    # the single-output call before any multi call
    q1 = pmk.DeviceQuery(m, X)
    q1.plan(radius, DELTA)
    q1.items_loo()
    before = q1.debug()

    def refused(text, status=-3):
        assert L.pmk_query_items_loo_multi(q.h, 0, 1, None, None) == status
        assert text in L.pmk_last_error().decode(), L.pmk_last_error().decode()
        wd = _wth(radius).desc()
        Yq = np.empty((N, 3), order="F")
        assert L.pmk_predict_mixture_loo_multi(m.h, C.byref(wd), X.ctypes.data_as(_dp), radius, DELTA, 0,
                                               Yq.ctypes.data_as(_dp), N, None) == status
        assert text in L.pmk_last_error().decode(), L.pmk_last_error().decode()
        with pytest.raises(_lib.PmkError):                  # the front end refuses the same state
            q.items_loo_multi()

    def accepted():
        nm, no = C.c_int64(), C.c_int64()
        assert L.pmk_query_items_loo_multi(q.h, 0, 1, C.byref(nm), C.byref(no)) == 0
        assert nm.value + no.value == q.total and no.value > 0

    accepted()
    assert L.pmk_query_items_loo_multi(pmk.DeviceQuery(m, X).h, 0, 1, None, None) == -1         # not planned
    m.fit(TH, SIGMA2)                                       # a new fit: d and the weights are stale
    refused("pmk_model_loo has not run")
    m.loo()
    refused("pmk_model_solve_multi has not run")
    m.solve_multi()
    accepted()
    m.set_trend("linear")
    refused("pmk_model_solve_multi has not run")
    m.solve_multi()
    accepted()
    m.set_targets_multi_global(np.asfortranarray(Y))
    refused("pmk_model_solve_multi has not run")
    m.set_trend(None)
    m.solve_multi()
    accepted()
    # the single-output call after all of this: the bits it returned before, trend or not
    for trend in (None, "linear"):
        m.set_trend(trend)
        m.solve_multi()
        accepted()
        q1.plan(radius, DELTA)
        q1.items_loo()
        after = q1.debug()
        assert same_bits(after["item_u"], before["item_u"]) and same_bits(after["item_v"], before["item_v"])
    # a model fitted but never solved
    fresh = pmk.DeviceModel.from_tree(root, X, np.ascontiguousarray(Y[:, 0]), eps=eps)
    fresh.fit(TH, SIGMA2)
    fresh.loo()
    qf = pmk.DeviceQuery(fresh, X)
    qf.plan(radius, DELTA)
    assert L.pmk_query_items_loo_multi(qf.h, 0, 1, None, None) == -3
    assert "pmk_model_solve_multi has not run" in L.pmk_last_error().decode()
    assert L.pmk_query_get_items_multi(qf.h, None, 0, None) == -2


@pytest.mark.parametrize("trend", [None, "linear"])
def test_the_one_shot_and_the_module_functions(W, trend):
    X, Y, root = W["X"], W["Y"], W["root"]
    eps, radius = 0.3, 0.6
    m = W["get_model"](eps, trend)
    _, _, _, _, MUh, Vh = _staged(m, X, radius)
    L = pmk.lib()
    wd = _wth(radius).desc()
    MU1, V1 = np.full((N + 5, 3), -7.0, order="F"), np.empty(N)
    _lib.check(L.pmk_predict_mixture_loo_multi(m.h, C.byref(wd), X.ctypes.data_as(_dp), radius, DELTA, 0,
                                               MU1.ctypes.data_as(_dp), N + 5, V1.ctypes.data_as(_dp)),
               "pmk_predict_mixture_loo_multi")
    assert same_bits(MU1[:N], MUh) and same_bits(V1, Vh) and np.all(MU1[N:] == -7.0)
    MU2 = np.empty((N, 3), order="F")
    _lib.check(L.pmk_predict_mixture_loo_multi(m.h, C.byref(wd), X.ctypes.data_as(_dp), radius, DELTA, 0,
                                               MU2.ctypes.data_as(_dp), N, None), "pmk_predict_mixture_loo_multi")
    assert same_bits(MU2, MUh)
    # the module functions on an eta built from the tree
    eta = pmk.MixtureGPType.from_tree(root, X, eps=eps)
    if trend is None:
        pmk.fitmixtureGP_multi_(eta, np.asfortranarray(Y), TH, SIGMA2)
    else:
        pmk.fitmixtureGP_trend_(eta, np.asfortranarray(Y), TH, SIGMA2, trend)
    mu, var = pmk.loomixtureGP_blend_multi(eta, root, radius, DELTA, _wth(radius))     # runs loo() itself, X from the model
    assert same_bits(mu, MUh) and same_bits(var, Vh)
    mu0, var0 = pmk.loomixtureGP_blend_multi(eta, root, radius, DELTA, _wth(radius), variance=False)
    assert same_bits(mu0, MUh) and var0 is None
    cands = [(0.25, DELTA, _wth(0.25)), (0.6, DELTA, _wth(0.6)), (0.9, DELTA, pmk.Spline34KernelType(3.0))]
    scores, best = pmk.selectblendGP_multi_(eta, root, Y, cands)
    want = np.empty((3, 3))
    for g, (r, d, w) in enumerate(cands):
        mu, var = pmk.loomixtureGP_blend_multi(eta, root, r, d, w, noisy=True)
        want[g] = [M.loo_log_pseudo_likelihood(Y[:, c] - mu[:, c], var) for c in range(3)]
    print("selectblendGP_multi_ scores:", scores, "best", best)
    assert same_bits(scores, want) and best == int(np.argmax(want.sum(axis=1))) and np.all(np.isfinite(scores))
