"""Kriging with a trend on the GPU (pmk_model_set_trend / _get_trend / _trend_info, and the multi-output calls with a trend
set): one generalised-least-squares drift per patch from the resident factor.

References: tests/_trend_refs.py -- GLS, prediction and trend-aware leave-one-out in numpy.longdouble from the oracle's
kernel matrices -- and the same quantities in plain fp64 scipy (LAPACK), which is the yardstick of every bound: a figure
of the device may be 10 x the larger of (the unit of the figure) and (what fp64 scipy achieves on the same inputs); the
margin is for summation order.  Units: n u for the KKT residuals, kappa_2(U) u scale for forward errors, u = eps of the
model's element type.  Every measured figure is printed before it is asserted ("TREND {json}") and a run of the whole
module writes them all to profiles/trend_accuracy.json.

Workload: the ragged SIZES of tests/test_gpu_multi_output.py, uniform(-4, 4), Spline34 a = 1/3, sigma2 = 1e-3
(kappa(U) <= 3.4e4).  The fp32 cases assert kappa(U) eps32 <= 1e-3 as the fp32 multi-output tests do, which a = 1/3,
sigma2 = 1e-3 cannot meet (3.4e4 eps32 = 4e-3): they run at those tests' own fp32 setting, a = 1, sigma2 = 0.05.

Per-item (mu, v): the library has no per-item download of the R-column results, so the items are explicit (point, region)
items (pmk_query_create_items), one per query, and the mixture of one home item with weight 1 returns the item itself.
Explicit items need a tree whose leaf count equals the patch count: the batch there is the ragged seven plus one small
patch, under an 8-leaf tree.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import mixture as M
from oracle import oracle as O
import _trend_refs as T
from test_gpu_multi_output import SIZES, _mixgp_case, _targets, kappa

pytestmark = pytest.mark.gpu

A = 1 / 3.0
SIGMA2 = 1e-3
EPS = {"f64": float(np.finfo(np.float64).eps), "f32": float(np.finfo(np.float32).eps)}
SETTING = {"f64": (A, SIGMA2), "f32": (1.0, 0.05)}
NONE, CONSTANT, LINEAR = -1, 0, 1
Q_OF = {"constant": lambda D: 1, "linear": lambda D: 1 + D}


_RECORDS = []
ACCURACY_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "trend_accuracy.json")


def _record(**kw):
    _RECORDS.append(kw)
    print("TREND " + json.dumps(kw, sort_keys=True))


@pytest.fixture(scope="module", autouse=True)
def _write_accuracy_file():
    """after the module's last test: every figure recorded by this run -> profiles/trend_accuracy.json.  Only a run of
    the whole module replaces the file: a selection of tests would leave it with part of the figures."""
    yield
    if {r["test"] for r in _RECORDS} == {"kkt", "reference", "mixture", "evidence"}:
        with open(ACCURACY_JSON, "w") as f:
            f.write("[\n" + ",\n".join(" " + json.dumps(r, sort_keys=True) for r in _RECORDS) + "\n]\n")


def _ragged(seed, D, sizes=SIZES):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-4, 4, (n, D)) for n in sizes]


def _model(Xs, Ys, dtype="f64", trend=None, diag=None, split=None):
    a, sigma2 = SETTING[dtype]
    model = M.DeviceModel(Xs, [np.ascontiguousarray(y[:, 0]) for y in Ys], dtype=dtype)
    if split is not None:
        assert pmk.default_context().L.pmk_test_model_set_split(model.h, split) == 0
    if diag is not None:
        model.set_diag(diag)
    model.fit(pmk.Spline34KernelType(a), sigma2)
    model.set_targets_multi(Ys)
    model.set_trend(trend)
    model.solve_multi()
    return model


_K = {}


def _kernel_matrices(seed, D, dtype, sizes=SIZES):
    """oracle K of every ragged patch and kappa(U), computed once per (seed, D, setting)"""
    key = (seed, D, SETTING[dtype], tuple(sizes))
    if key not in _K:
        a, sigma2 = SETTING[dtype]
        Xs = _ragged(seed, D, sizes)
        Ks = [O.kernel_matrix(O.kernel(O.SPLINE34, a), X) for X in Xs]
        _K[key] = (Xs, Ks, [kappa(K + sigma2 * np.eye(len(K))) for K in Ks])
    return _K[key]


def _bound(yardstick):
    """10 x the larger of the unit and what fp64 scipy achieves (both already in the unit)"""
    return 10.0 * max(1.0, yardstick)


# ------------------------------------------------------------------------------------------ 1. KKT residuals
KKT_CASES = [(D, R, trend, "f64") for D in (1, 2, 4) for R in (1, 3) for trend in ("constant", "linear")] + \
            [(2, 13, "linear", "f64"), (2, 3, "constant", "f32"), (2, 3, "linear", "f32")]


@pytest.mark.parametrize("D,R,trend,dtype", KKT_CASES)
def test_kkt_residuals(D, R, trend, dtype):
    Xs, Ks, kappas = _kernel_matrices(50 + D, D, dtype)
    sigma2, u, q = SETTING[dtype][1], EPS[dtype], Q_OF[trend](D)
    Ys = [_targets(X, R) for X in Xs]
    model = _model(Xs, Ys, dtype, trend)
    Cs, (betas, Gs), flags = model.weights_multi(), model.trend(), model.trend_info()
    failures = []
    for r, (X, K, Y) in enumerate(zip(Xs, Ks, Ys)):
        n = len(X)
        if n < q:
            assert flags[r] == n + 1 and np.all(np.isnan(Cs[r])) and np.all(np.isnan(betas[r]))
            continue
        assert flags[r] == 0 and betas[r].shape == (q, R) and Gs[r].shape == (q, q)
        if dtype == "f32":
            assert kappas[r] * EPS["f32"] <= 1e-3, kappas[r]
        H = T.basis(X, trend)
        U = K + sigma2 * np.eye(n)
        f = T.gls_fp64(K, sigma2, Y, H)
        dev = T.kkt_ratios(U, H, Y, Cs[r], betas[r], u, f["C_Y"], f["C_H"])
        ref = T.kkt_ratios(U, H, Y, f["C"], f["beta"], u, f["C_Y"], f["C_H"])
        _record(test="kkt", D=D, R=R, trend=trend, dtype=dtype, n=n, primal=dev[0], constraint=dev[1], scipy_primal=ref[0],
                scipy_constraint=ref[1])
        for name, d, s in (("primal", dev[0], ref[0]), ("constraint", dev[1], ref[1])):
            if not d <= _bound(s):
                failures.append((r, n, name, d, s))
    assert not failures, failures


# ------------------------------------------------------------------------------------------ 2. the long-double reference
_REF = {}
ITEM_SIZES = SIZES + [5]          # the eighth patch completes the 8-leaf tree that explicit items need


def _item_batch(dtype, trend, R=3, D=2):
    """patches, targets, long-double and fp64 references, query points per patch: computed once and shared"""
    key = (dtype, trend)
    if key not in _REF:
        a, sigma2 = SETTING[dtype]
        Xs, Ks, kappas = _kernel_matrices(61, D, dtype, ITEM_SIZES)
        oth = O.kernel(O.SPLINE34, a)
        Ys = [_targets(X, R) for X in Xs]
        rng = np.random.default_rng(62)
        out = []
        for X, K, Y, k in zip(Xs, Ks, Ys, kappas):
            if len(X) < Q_OF[trend](D):
                out.append(None)
                continue
            H = T.basis(X, trend)
            # queries: inside the data, on its edge, and two far outside every kernel support
            xq = np.vstack([rng.uniform(-4, 4, (12, D)), rng.uniform(3.5, 5.5, (4, D)), [[40.0, -25.0], [-300.0, 7.0]]])
            Kq, kqq, Hq = O.cross_kernel_matrix(oth, xq, X), np.full(len(xq), O.profile(oth, 0.0)), T.basis(xq, trend)
            ld, f = T.trend_reference(K, sigma2, Y, H), T.gls_fp64(K, sigma2, Y, H)
            out.append(dict(ld=ld, f64=f, xq=xq, pred_ld=T.predict_reference(ld, Kq, kqq, Hq),
                            pred_f64=T.predict_fp64(f, Kq, kqq, Hq), kappa=k))
        _REF[key] = (Xs, Ys, out)
    return _REF[key]


def _explicit_items(model, xq, region):
    """(mu [m, R], v [m]) of explicit (point, region) items through items_multi -> mix_multi -> fetch_multi"""
    tree_pts = np.random.default_rng(5).uniform(-4, 4, (64, xq.shape[1]))
    root, _, _ = pmk.setuppartition(tree_pts, 4)                       # any 8-leaf tree: the items name their regions
    model.set_bsp(root, 0)
    xq = np.ascontiguousarray(xq, dtype=np.float64)
    region = np.ascontiguousarray(region, dtype=np.int32)
    q = M.DeviceQuery.from_items(model, len(xq), xq.ctypes.data_as(C.c_void_p), region.ctypes.data_as(C.c_void_p))
    q.items_multi(pmk.Spline34KernelType(SETTING[model.dtype][0]), True)
    q.mix_multi(pmk.Spline34KernelType(1.0))
    return q.fetch_multi(model.R)


def _err(dev, ref):
    return float(np.abs(np.asarray(dev, dtype=T.LD) - ref).max())


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("trend", ["constant", "linear"])
def test_against_long_double_reference(trend, dtype):
    Xs, Ys, refs = _item_batch(dtype, trend)
    u = EPS[dtype]
    model = _model(Xs, Ys, dtype, trend)
    Cs, (betas, Gs), flags = model.weights_multi(), model.trend(), model.trend_info()
    model.loo()
    RES, VAR = model.loo_values_multi()
    live = [r for r, ref in enumerate(refs) if ref is not None]
    xq = np.vstack([refs[r]["xq"] for r in live])
    region = np.concatenate([np.full(len(refs[r]["xq"]), r) for r in live])
    MU, V = _explicit_items(model, xq, region)
    failures, at = [], 0
    for r, ref in enumerate(refs):
        if ref is None:
            assert flags[r] == len(Xs[r]) + 1
            continue
        assert flags[r] == 0
        if dtype == "f32":
            assert ref["kappa"] * EPS["f32"] <= 1e-3, ref["kappa"]
        ld, f = ref["ld"], ref["f64"]
        m = len(ref["xq"])
        mu, v = MU[at:at + m], V[at:at + m]
        at += m
        mu_ld, v_ld = ref["pred_ld"]
        mu_f, v_f = ref["pred_f64"]
        figures = {
            "beta": (betas[r], f["beta"], ld["beta"]), "G": (Gs[r], f["G"], ld["G"]), "weights": (Cs[r], f["C"], ld["C"]),
            "loo_res": (RES[r], f["res"], ld["res"]), "loo_var": (VAR[r], f["var"], ld["var"]),
            # the two far queries apart: with a linear trend their |mu| and v are hundreds of times the interior's, and
            # one scale for all would hold the interior queries to almost nothing
            "mu_near": (mu[:-2], mu_f[:-2], mu_ld[:-2]), "mu_far": (mu[-2:], mu_f[-2:], mu_ld[-2:]),
            "v_near": (v[:-2], v_f[:-2], v_ld[:-2]), "v_far": (v[-2:], v_f[-2:], v_ld[-2:]),
        }
        # C = C_Y - C_H beta cancels (to exactly zero for one point and a constant trend): the scale of its error is that
        # of its terms.  Leaving one of n <= q points out leaves fewer points than basis functions: no such prediction,
        # and the library says so with NaN.
        scales = {"weights": float(np.abs(ld["C_Y"]).max() + np.abs(ld["C_H"] @ ld["beta"]).max())}
        if len(Xs[r]) <= Q_OF[trend](Xs[r].shape[1]):
            del figures["loo_res"], figures["loo_var"]
            assert np.isnan(RES[r]).all() and np.isnan(VAR[r]).all(), (r, RES[r], VAR[r])
        for name, (dev, f64, ref_ld) in figures.items():
            unit = ref["kappa"] * u * scales.get(name, float(np.abs(ref_ld).max()))
            d, s = _err(dev, ref_ld) / unit, _err(f64, ref_ld) / unit
            _record(test="reference", trend=trend, dtype=dtype, n=len(Xs[r]), what=name, device=d, scipy=s)
            if not d <= _bound(s):
                failures.append((r, len(Xs[r]), name, d, s))
    assert not failures, failures


# ------------------------------------------------------------------------------------------ 3. fails without the feature
def test_exact_plane_is_recovered_and_extrapolated():
    Xs = _ragged(70, 2)[1:]                              # every patch has n >= q = 3
    Ys = [(2 + 3 * X[:, 0] - X[:, 1])[:, None] for X in Xs]
    far = np.array([[60.0, 45.0], [-200.0, 3.0], [17.0, -90.0]])     # outside every kernel support (radius 3)
    plain = _model(Xs + Xs[:2], Ys + Ys[:2])             # eight patches for the 8-leaf tree
    trended = _model(Xs + Xs[:2], Ys + Ys[:2], trend="linear")
    assert np.all(trended.trend_info() == 0)
    betas, _ = trended.trend()
    for r, (b, Cw, C0) in enumerate(zip(betas, trended.weights_multi(), plain.weights_multi())):
        assert np.abs(b[:, 0] - [2, 3, -1]).max() <= 1e-9, (r, b[:, 0])
        assert np.abs(Cw).max() <= 1e-9 * np.abs(C0).max(), r          # the plane explains everything
    for model, want in ((plain, np.zeros(3)), (trended, 2 + 3 * far[:, 0] - far[:, 1])):
        for r in (0, 5):
            mu, v = _explicit_items(model, far, np.full(3, r))
            assert np.abs(mu[:, 0] - want).max() <= 1e-7 * max(1.0, np.abs(want).max()), (r, mu[:, 0], want)
    assert np.abs(_explicit_items(plain, far, np.zeros(3))[1] - 1.0).max() <= 1e-12     # simple kriging: the prior variance


# ------------------------------------------------------------------------------------------ 4. mixture end to end
def _blend(mu_items, v_items, home_mu, home_v, off, ts, owth):
    """querymixtureGP's blend (neighbours phi_w(|t|) in hyperplane order, home weight 1 last, normalised) in Python"""
    Nq = len(home_v)
    Yq, Vq = np.zeros((Nq, home_mu.shape[1])), np.zeros(Nq)
    for j in range(Nq):
        w = np.array([O.profile(owth, abs(t)) for t in ts[off[j]:off[j + 1]]] + [1.0])
        w = w / w.sum()
        mu = np.vstack([mu_items[off[j]:off[j + 1]], home_mu[j:j + 1]])
        v = np.concatenate([v_items[off[j]:off[j + 1]], home_v[j:j + 1]])
        Yq[j], Vq[j] = w @ mu, (w * w) @ v
    return Yq, Vq


@pytest.mark.parametrize("trend", ["constant", "linear"])
def test_mixture_end_to_end(trend):
    levels, eps, a, radius, delta, R = 4, 0.6, 1 / 4.0, 0.5, 1e-5, 2
    X, Xq, root, X_set, X_set_inds = _mixgp_case(1500, levels, eps, radius, 700, 25)
    Yall = _targets(X, R) + 3.0 + 0.5 * X[:, :1]
    th, wth = pmk.Spline34KernelType(a), pmk.Spline34KernelType(1 / radius)
    oth, owth = O.kernel(O.SPLINE34, a), O.kernel(O.SPLINE34, 1 / radius)
    Ys = [Yall[i] for i in X_set_inds]
    # reference: long-double per-item values, blended with the oracle's neighbour lists and weights
    fits = [O.fit_patch(oth, xs, y[:, 0], SIGMA2) for xs, y in zip(X_set, Ys)]
    _, _, home, off, reg, ts = O.query_mixture(O.BSP(X, levels), oth, owth, X_set, [f["c_lu"] for f in fits],
                                               [f["L"] for f in fits], Xq, radius, delta, debug=True, nthreads=8)
    refs = [T.trend_reference(O.kernel_matrix(oth, xs), SIGMA2, y, T.basis(xs, trend)) for xs, y in zip(X_set, Ys)]
    item_q = np.repeat(np.arange(len(Xq)), np.diff(off))

    def per_item(points, regions):
        mu, v = np.zeros((len(points), R)), np.zeros(len(points))
        for r in np.unique(regions):
            sel = np.nonzero(regions == r)[0]
            xs = X_set[r]
            m, vv = T.predict_reference(refs[r], O.cross_kernel_matrix(oth, points[sel], xs),
                                        np.full(len(sel), O.profile(oth, 0.0)), T.basis(points[sel], trend))
            mu[sel], v[sel] = np.asarray(m, dtype=np.float64), np.asarray(vv, dtype=np.float64)
        return mu, v

    mu_nb, v_nb = per_item(Xq[item_q], reg)
    mu_home, v_home = per_item(Xq, home)
    wantY, wantV = _blend(mu_nb, v_nb, mu_home, v_home, off, ts, owth)

    eta = pmk.MixtureGPType(X_set, pmk.fetchhyperplanes(root))
    pmk.fitmixtureGP_trend_(eta, Ys, th, SIGMA2, trend=trend)
    assert eta.beta_set[0].shape == (T.basis(X[:1], trend).shape[1], R) and eta.C_set[0].shape == (len(X_set[0]), R)
    Yq, Vq = pmk.querymixtureGP_multi(Xq, eta, root, levels, radius, delta, th, SIGMA2, wth)
    Ym, Vm = pmk.querymixtureGP_multi(Xq, eta, root, levels, radius, delta, th, SIGMA2, wth, variance=False)
    # the same through per-patch kernels: fit_patches + items_multi_fitted
    etap = pmk.MixtureGPType(X_set, pmk.fetchhyperplanes(root))
    pmk.fitmixtureGP_patches_(etap, [y[:, 0].copy() for y in Ys], [th] * len(X_set), [SIGMA2] * len(X_set))
    etap._model.set_targets_multi(Ys)
    etap._model.set_trend(trend)
    etap._model.solve_multi()
    Yp, Vp = pmk.querymixtureGP_multi_patches(Xq, etap, root, levels, radius, delta, wth)
    _record(test="mixture", trend=trend, dY=float(np.abs(Yq - wantY).max()), dV=float(np.abs(Vq - wantV).max()),
            dY_patches=float(np.abs(Yp - wantY).max()), dV_patches=float(np.abs(Vp - wantV).max()))
    assert Vm is None
    assert np.array_equal(Ym, Yq)                       # the epilogue's means do not depend on the variance pass
    for Yd, Vd in ((Yq, Vq), (Yp, Vp)):
        assert np.all(np.abs(Yd - wantY) <= 1e-7 * np.maximum(1, np.abs(wantY))), np.abs(Yd - wantY).max()
        assert np.all(np.abs(Vd - wantV) <= 1e-9 + 1e-5 * wantV), np.abs(Vd - wantV).max()
    # a refit without a trend behaves as it always did
    pmk.fitmixtureGP_multi_(eta, Ys, th, SIGMA2)
    fresh = pmk.MixtureGPType(X_set, pmk.fetchhyperplanes(root))
    pmk.fitmixtureGP_multi_(fresh, Ys, th, SIGMA2)
    assert all(np.array_equal(c1, c2) for c1, c2 in zip(eta.C_set, fresh.C_set))


def test_tree_route_and_trend_free_refit():
    """fitmixtureGP_trend_ on an eta built by from_tree (global targets, the resident model refitted) equals the list
    route bit for bit; fitmixtureGP_multi_ afterwards clears the trend of the resident model"""
    levels, eps, R = 4, 0.6, 2
    X, Xq, root, X_set, X_set_inds = _mixgp_case(1500, levels, eps, 0.5, 100, 29)
    Yall = np.asfortranarray(_targets(X, R) + 3.0 + 0.5 * X[:, :1])
    th, wth = pmk.Spline34KernelType(A), pmk.Spline34KernelType(2.0)
    hps = pmk.fetchhyperplanes(root)
    lst = pmk.MixtureGPType(X_set, hps)
    pmk.fitmixtureGP_trend_(lst, [Yall[i] for i in X_set_inds], th, SIGMA2, trend="linear")
    eta = pmk.MixtureGPType.from_tree(root, X, eps=eps, hps=hps)
    pmk.fitmixtureGP_trend_(eta, Yall, th, SIGMA2, trend="linear")
    assert len(eta.C_set) == len(lst.C_set)
    for r in range(len(lst.C_set)):
        assert np.array_equal(eta.C_set[r], lst.C_set[r]) and np.array_equal(eta.beta_set[r], lst.beta_set[r]), r
    Yt, Vt = pmk.querymixtureGP_multi(Xq, eta, root, levels, 0.5, 1e-5, th, SIGMA2, wth)
    Yl, Vl = pmk.querymixtureGP_multi(Xq, lst, root, levels, 0.5, 1e-5, th, SIGMA2, wth)
    assert np.array_equal(Yt, Yl) and np.array_equal(Vt, Vl)
    # the same resident model, refitted without a trend: as if it never had one
    pmk.fitmixtureGP_multi_(eta, Yall, th, SIGMA2)
    assert eta.beta_set is None
    assert np.all(eta._model.trend_info() == 0) and eta._model.trend()[0][0].shape == (0, R)
    fresh = pmk.MixtureGPType.from_tree(root, X, eps=eps, hps=hps)
    pmk.fitmixtureGP_multi_(fresh, Yall, th, SIGMA2)
    assert all(np.array_equal(c1, c2) for c1, c2 in zip(eta.C_set, fresh.C_set))
    assert not any(np.array_equal(c1, c2) for c1, c2 in zip(eta.C_set, lst.C_set))
    Y0, V0 = pmk.querymixtureGP_multi(Xq, eta, root, levels, 0.5, 1e-5, th, SIGMA2, wth)
    Y1, V1 = pmk.querymixtureGP_multi(Xq, fresh, root, levels, 0.5, 1e-5, th, SIGMA2, wth)
    assert np.array_equal(Y0, Y1) and np.array_equal(V0, V1)


# ------------------------------------------------------------------------------------------ 5. bit identity
def _everything(model, root, Xq, th, wth):
    model.set_bsp(root, 0)
    q = M.DeviceQuery(model, Xq)
    q.plan(0.5, 1e-5)
    q.items_multi(th, True)
    q.mix_multi(wth)
    Yq, Vq = q.fetch_multi(model.R)
    q.items(th)
    q.mix(wth)
    y1, v1 = q.fetch()
    model.loo()
    return dict(C=model.weights_multi(), ev=model.evidence_multi(), loo=model.loo_values_multi(), Yq=Yq, Vq=Vq, y1=y1, v1=v1,
                c=model.weights(), ev1=model.evidence(), loo1=model.loo_values())


def _same(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


def test_bit_identity_without_a_trend():
    levels, R = 4, 3
    X, Xq, root, X_set, X_set_inds = _mixgp_case(1500, levels, 0.6, 0.5, 300, 27)
    Ys = [_targets(X, R)[i] for i in X_set_inds]
    th, wth = pmk.Spline34KernelType(A), pmk.Spline34KernelType(2.0)
    fresh = _everything(_model(X_set, Ys), root, Xq, th, wth)
    model = _model(X_set, Ys, trend="linear")
    with_trend = _everything(model, root, Xq, th, wth)
    model.set_trend(None)
    model.solve_multi()
    again = _everything(model, root, Xq, th, wth)
    for key in fresh:
        assert _same(fresh[key], again[key]), key
    # the single-output results never see the trend
    for key in ("y1", "v1", "c", "ev1", "loo1"):
        assert _same(fresh[key], with_trend[key]), key
    assert not _same(fresh["C"], with_trend["C"])
    assert np.all(with_trend["Vq"] - fresh["Vq"] >= 0)          # the drift's uncertainty only adds


# ------------------------------------------------------------------------------------------ 6. flags
def test_flags():
    Xs = _ragged(80, 2)
    Xs[3] = Xs[3].copy()
    Xs[3][:, 1] = 0.0                                    # x_2 == 0 exactly: column 3 of H, and row 3 of G, are exactly zero
    Ys = [_targets(X, 2) for X in Xs]
    lin = _model(Xs, Ys, trend="linear")
    flags = lin.trend_info()
    assert list(flags) == [2, 0, 0, 3, 0, 0, 0], flags   # n = 1 < q = 3 -> n + 1; the degenerate patch -> pivot 3
    assert pmk.lib().pmk_model_trend_info(lin.h, flags.ctypes.data_as(C.POINTER(C.c_int32))) == 1
    betas, Gs = lin.trend()
    Cl = lin.weights_multi()
    assert np.all(Gs[3][2] == 0.0) and np.all(Gs[3][:, 2] == 0.0)
    for r in (0, 3):
        assert np.all(np.isnan(betas[r])) and np.all(np.isnan(Cl[r]))
    # the constant trend is fine on both, and on one point beta = y
    con = _model(Xs, Ys, trend="constant")
    assert np.all(con.trend_info() == 0)
    assert np.abs(con.trend()[0][0][0] - Ys[0][0]).max() <= 4 * EPS["f64"] * np.abs(Ys[0]).max()
    # the other patches do not see their neighbours' flags: the same batch with a healthy patch 3
    Xh = list(Xs)
    Xh[3] = _ragged(80, 2)[3]
    healthy = _model(Xh, Ys, trend="linear")
    assert list(healthy.trend_info()) == [2, 0, 0, 0, 0, 0, 0]
    for r in (1, 2, 4, 5, 6):
        assert np.array_equal(healthy.weights_multi()[r], Cl[r]), r
        assert np.array_equal(healthy.trend()[0][r], betas[r]), r
    # a patch whose factorisation failed (one diagonal addend of -3, as in test_gpu_breakdown.py): NaN there only
    dg = [np.zeros(len(X)) for X in Xs]
    sound = _model(Xs, Ys, trend="constant", diag=dg)
    dg[4][17] = -3.0
    broken = _model(Xs, Ys, trend="constant", diag=dg)
    assert broken.info()[4] == 18 and np.all(np.delete(broken.info(), 4) == 0)
    assert np.all(broken.trend_info() == 0)              # the failure is pmk_model_info's to report
    Cb, (bb, _) = broken.weights_multi(), broken.trend()
    assert np.all(np.isnan(Cb[4])) and np.all(np.isnan(bb[4]))
    broken.loo()
    assert np.all(np.isnan(broken.loo_values_multi()[0][4]))
    Cs, (bs, _) = sound.weights_multi(), sound.trend()
    for r in (0, 1, 2, 3, 5, 6):
        assert np.array_equal(Cb[r], Cs[r]) and np.array_equal(bb[r], bs[r]), r


# ------------------------------------------------------------------------------------------ 7. evidence
@pytest.mark.parametrize("trend", ["constant", "linear"])
def test_evidence_is_the_gls_quadratic_form(trend):
    Xs, Ys, refs = _item_batch("f64", trend)
    model = _model(Xs, Ys, "f64", trend)
    _, quad = model.evidence_multi()
    failures = []
    for r, ref in enumerate(refs):
        if ref is None:
            assert np.all(np.isnan(quad[r]))
            continue
        # quad = Y^T C_Y - B^T G^-1 B cancels (to zero for one point and a constant trend): the scale is that of its terms
        unit = ref["kappa"] * EPS["f64"] * float(np.abs((np.asarray(Ys[r], dtype=T.LD) * ref["ld"]["C_Y"]).sum(0)).max())
        d, s = _err(quad[r], ref["ld"]["quad"]) / unit, _err(ref["f64"]["quad"], ref["ld"]["quad"]) / unit
        _record(test="evidence", trend=trend, n=len(Xs[r]), device=d, scipy=s)
        if not d <= _bound(s):
            failures.append((r, d, s))
    assert not failures, failures


# ------------------------------------------------------------------------------------------ 8. errors
def test_errors():
    L = pmk.lib()
    Xs = _ragged(90, 2)[1:4]
    model = M.DeviceModel(Xs, [X[:, 0].copy() for X in Xs])
    model.fit(pmk.Spline34KernelType(A), SIGMA2)
    for bad in (-2, 2, 7):
        assert L.pmk_model_set_trend(model.h, bad) == -2
        assert b"degree" in L.pmk_last_error()
    model.set_targets_multi([_targets(X, 14) for X in Xs])
    q = C.c_int(-1)
    assert L.pmk_model_get_trend(model.h, C.byref(q), None, None) == -3           # before any solve
    flags = np.zeros(3, dtype=np.int32)
    assert L.pmk_model_trend_info(model.h, flags.ctypes.data_as(C.POINTER(C.c_int32))) == -3
    assert L.pmk_model_set_trend(model.h, LINEAR) == 0
    assert L.pmk_model_solve_multi(model.h) == -3                                  # 14 + 3 > 16
    msg = L.pmk_last_error()
    assert b"R=14" in msg and b"q=3" in msg
    assert L.pmk_model_get_trend(model.h, C.byref(q), None, None) == -3
    assert L.pmk_model_set_trend(model.h, CONSTANT) == 0
    assert L.pmk_model_solve_multi(model.h) == 0                                   # 14 + 1 fits
    assert L.pmk_model_get_trend(model.h, C.byref(q), None, None) == 0 and q.value == 1
    assert L.pmk_model_set_trend(model.h, NONE) == 0
    assert L.pmk_model_get_trend(model.h, C.byref(q), None, None) == -3           # set_trend made the weights stale
    assert L.pmk_model_solve_multi(model.h) == 0
    assert L.pmk_model_get_trend(model.h, C.byref(q), None, None) == 0 and q.value == 0


# ------------------------------------------------------------------------------------------ 9. other routes
def test_split_mode_and_loaded_model():
    Xs = _ragged(95, 2)[4:]                              # 129, 257, 700: two tiles and more, so that the split path exists
    Ys = [_targets(X, 3) for X in Xs]
    regular = _model(Xs, Ys, trend="linear")
    Cr, (br, _) = regular.weights_multi(), regular.trend()
    split = _model(Xs, Ys, trend="linear", split=1)
    assert np.all(split.info() == 0) and np.all(split.trend_info() == 0)
    loaded = M.DeviceModel.from_factors(Xs, regular.weights(), [regular.get(r, M.GET_L) for r in range(len(Xs))])
    loaded.set_targets_multi(Ys)
    loaded.set_trend("linear")
    loaded.solve_multi()
    assert np.all(loaded.trend_info() == 0)
    # loaded: two solves from the same factor bits, the tolerance of tests/test_gpu_multi_output.py for that comparison;
    # split: another summation order in the factor itself, held to that file's tolerance against a reference solve
    for other, tol in ((loaded, 1e-12), (split, 1e-6)):
        Co, (bo, _) = other.weights_multi(), other.trend()
        for r in range(len(Xs)):
            assert np.linalg.norm(Co[r] - Cr[r]) <= tol * np.linalg.norm(Cr[r]), (tol, r)
            assert np.linalg.norm(bo[r] - br[r]) <= tol * np.linalg.norm(br[r]), (tol, r)
