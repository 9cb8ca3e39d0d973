"""Gradient of the blended mean on the GPU (pmk_query_items_grad / _mix_grad / _fetch_grad / _get_items_grad,
pmk_predict_mixture_grad_fitted; item_grads_kernel and mix_grad_kernel of pmk_grad.hip).

Reference: tests/_grad_refs.py, the numpy.longdouble restatement that tests/test_grad_refs.py pins to the oracle.

Per-item gradients.  The reference is evaluated with the device's OWN weights (weights_multi, and trend() for beta) and, in
fp32, with the points and queries rounded to float32 first, so that only the new kernel is judged.  Bound, per column c:
    |err| <= (n + 32) u lip(theta) sum_k |C[k, c]|,   u = 2^-53 (fp64) or 2^-24 (fp32),
lip = max |phi'|: every one of the n products psi (x_d - z_d) C is at most lip |C| in magnitude, any summation order of n
such products stays inside n u, and the 32 covers the evaluation of psi and of the distance.
Shapes: explicit (point, region) items (pmk_query_create_items) under an 8-leaf tree, patches of 1, 7, 8, 9, 127, 128, 129
and 40 points (the 8-point unroll and the 128-row slab edge), regions with 0, 1, 15, 16, 17 and 33 items (the 16-item
chunk), D = 1..4, R = 1, 3, 16, R = 12 with a linear trend at D = 3 (R + q = 16).

Blend.  fetch_grad against mix_grad_ref fed with the device's own items (debug(), item_values_multi(), item_grads()):
    |err| <= 16 m 2^-53 sum_i (|w_i G_i| + |(u_i - Y) dw_i|) / S   for a query of m items,
and, end to end, against central differences of pmk_predict_mixture_multi_fitted under the rule of tests/test_grad_refs.py.

Every measured ratio err / bound is printed ("GRAD {json}", run with -s) and a run of the whole module writes them to
profiles/grad_accuracy.json.
"""
import ctypes as C
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
from patchmixturekriging_amd import mixture as M
from patchmixturekriging_amd.partition import hyperplane_arrays
from oracle import oracle as O
import _grad_refs as GR

pytestmark = pytest.mark.gpu

U_OF = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
SIGMA2 = {"f64": 1e-2, "f32": 0.05}
FAMILIES = {
    "spline34": (pmk.Spline34KernelType(1 / 3.0), O.kernel(O.SPLINE34, 1 / 3.0)),
    "spline12": (pmk.Spline12KernelType(1 / 3.0), O.kernel(O.SPLINE12, 1 / 3.0)),
    "spline32": (pmk.Spline32KernelType(1 / 3.0), O.kernel(O.SPLINE32, 1 / 3.0)),
    "gaussian": (pmk.GaussianKernel1DType(2.0), O.kernel(O.GAUSSIAN, 2.0)),
    "rq": (pmk.RationalQuadraticKernelType(2.0), O.kernel(O.RQ, 2.0)),
    "trq": (pmk.TunableRationalQuadraticKernelType(2.0, 0.7), O.kernel(O.TRQ, 2.0, 0.7)),
    "modsqexp": (pmk.ModulatedSqExpKernelType(2.0, 1.3), O.kernel(O.MODSQEXP, 2.0, 1.3)),
}
SIZES = [1, 7, 8, 9, 127, 128, 129, 40]
COUNTS = [17, 1, 15, 16, 33, 0, 3, 5]           # items per region; rotated per case so that every patch size meets several

_RECORDS = []
ACCURACY_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "grad_accuracy.json")


def _record(**kw):
    _RECORDS.append(kw)
    print("GRAD " + json.dumps(kw, sort_keys=True))


@pytest.fixture(scope="module", autouse=True)
def _write_accuracy_file():
    """only a run of the whole module replaces the file"""
    yield
    if {r["test"] for r in _RECORDS} >= {"items", "items_mixed", "blend", "blend_fd"}:
        with open(ACCURACY_JSON, "w") as f:
            f.write("[\n" + ",\n".join(" " + json.dumps(r, sort_keys=True) for r in _RECORDS) + "\n]\n")


def _targets(X, R):
    cols = [np.sin((0.5 + 0.3 * j) * X[:, 0] + 0.2 * j) * np.cos((0.2 + 0.1 * j) * X[:, -1]) + 0.1 * j + 0.3 * X[:, 0]
            for j in range(R)]
    return np.stack(cols, 1)


def _round(a, dtype):
    return a.astype(np.float32).astype(np.float64) if dtype == "f32" else a


_TREE8 = {}


def _tree8(D):
    """any 8-leaf tree: explicit items name their regions"""
    if D not in _TREE8:
        _TREE8[D] = pmk.setuppartition(np.random.default_rng(5).uniform(-4, 4, (64, D)), 4)[0]
    return _TREE8[D]


def _patches(seed, D, dtype):
    rng = np.random.default_rng(seed)
    return [_round(rng.uniform(-2, 2, (n, D)), dtype) for n in SIZES]


def _model(Xs, Ys, theta, dtype="f64", trend=None, diag=None):
    """theta: one kernel (pmk_model_fit) or a list, one per patch (pmk_model_fit_patches)"""
    model = M.DeviceModel(Xs, [np.ascontiguousarray(y[:, 0]) for y in Ys], dtype=dtype)
    if diag is not None:
        model.set_diag(diag)
    if isinstance(theta, list):
        model.fit_patches(theta, [SIGMA2[dtype]] * len(Xs))
    else:
        model.fit(theta, SIGMA2[dtype])
    model.set_targets_multi(Ys)
    model.set_trend(trend)
    model.solve_multi()
    model.set_bsp(_tree8(Xs[0].shape[1]), 0)
    return model


def _items(seed, Xs, counts, dtype):
    """(xq [m, D], region [m]): per region random points around the patch; the first item of a region coincides with a
    training point"""
    rng = np.random.default_rng(seed)
    D = Xs[0].shape[1]
    xq, region = [], []
    for r, cnt in enumerate(counts):
        if cnt == 0:
            continue
        pts = rng.uniform(-2.5, 2.5, (cnt, D))
        pts[0] = Xs[r][len(Xs[r]) // 2]
        xq.append(pts)
        region += [r] * cnt
    return _round(np.vstack(xq), dtype), np.array(region, dtype=np.int32)


def _explicit_query(model, xq, region):
    xq = np.ascontiguousarray(xq, dtype=np.float64)
    region = np.ascontiguousarray(region, dtype=np.int32)
    q = M.DeviceQuery.from_items(model, len(xq), xq.ctypes.data_as(C.c_void_p), region.ctypes.data_as(C.c_void_p))
    q._keep = (xq, region)
    return q


def _worst_ratio(err, bound):
    """max err / bound; a zero bound (all-zero weights) admits only a zero error"""
    zero = bound == 0
    if np.any(err[zero] > 0):
        return float("inf")
    return float((err[~zero] / bound[~zero]).max()) if np.any(~zero) else 0.0


def _item_ratios(G, xq, region, Xs, Cs, oths, betas, tinfo, u):
    """worst err / bound over the items; NaN exactly where the patch is flagged"""
    worst, lips = 0.0, {}
    for i, (x, r) in enumerate(zip(xq, region)):
        if tinfo[r] != 0:
            assert np.all(np.isnan(G[i])), (i, r)
            continue
        oth = oths[r]
        key = (oth.family, oth.p[0], oth.p[1])
        if key not in lips:
            lips[key] = GR.lip(oth)
        ref = np.asarray(GR.item_grad_ref(oth, Xs[r], Cs[r], x, betas[r])).T                 # R x D
        bound = (len(Xs[r]) + 32) * u * lips[key] * np.abs(Cs[r]).sum(0)                       # R
        assert np.all(np.isfinite(G[i])), (i, r)
        err = np.abs(np.asarray(G[i], dtype=GR.LD) - ref).astype(np.float64)
        worst = max(worst, _worst_ratio(err, np.broadcast_to(bound[:, None], err.shape)))
    return worst


ITEM_CASES = [(D, R, "spline34", "f64", None) for D in (1, 2, 3, 4) for R in (1, 3, 16)] + \
             [(2, 3, fam, "f64", None) for fam in ("spline12", "spline32", "gaussian", "rq", "trq")] + \
             [(1, 3, "modsqexp", "f64", None), (2, 3, "spline34", "f32", None), (3, 1, "rq", "f32", None),
              (3, 12, "spline34", "f64", "linear"), (2, 3, "spline32", "f32", "linear"), (2, 3, "gaussian", "f64", "constant"),
              (4, 2, "rq", "f64", "linear"), (1, 3, "spline12", "f64", "linear")]


@pytest.mark.parametrize("D,R,family,dtype,trend", ITEM_CASES)
def test_item_gradients(D, R, family, dtype, trend):
    case = ITEM_CASES.index((D, R, family, dtype, trend))
    th, oth = FAMILIES[family]
    Xs = _patches(100 + case, D, dtype)
    Ys = [_targets(X, R) for X in Xs]
    model = _model(Xs, Ys, th, dtype, trend)
    assert np.all(model.info() == 0)
    counts = list(np.roll(COUNTS, case))
    xq, region = _items(200 + case, Xs, counts, dtype)
    q = _explicit_query(model, xq, region)
    q.items_multi(th, False)
    U0, _ = q.item_values_multi()
    q.items_grad(th)
    G, plane = q.item_grads()
    assert G.shape == (len(xq), R, D) and np.all(plane == -1)
    assert np.array_equal(q.item_values_multi()[0], U0, equal_nan=True)          # the means keep their bits
    Cs = model.weights_multi()
    tinfo = model.trend_info() if trend else np.zeros(len(Xs), dtype=np.int32)
    betas = model.trend()[0] if trend == "linear" else [None] * len(Xs)
    if trend == "linear":
        assert [int(f != 0) for f in tinfo] == [int(n < 1 + D) for n in SIZES]       # a patch of n < q points is flagged: NaN
    worst = _item_ratios(G, xq, region, Xs, Cs, [oth] * len(Xs), betas, tinfo, U_OF[dtype])
    _record(test="items", D=D, R=R, family=family, dtype=dtype, trend=trend, ratio=worst)
    assert worst <= 1.0, worst
    # one home item per query with weight 1: the blend returns the item's gradient bit for bit
    w = pmk.Spline34KernelType(1.0)
    q.mix_multi(w)
    q.mix_grad(w)
    assert np.array_equal(q.fetch_grad(), G, equal_nan=True)


def test_mixed_families_per_patch_and_the_models_own_kernels():
    D, R = 2, 3
    names = ["spline34", "gaussian", "rq", "spline12", "trq", "spline32", "spline34", "rq"]
    thetas, oths = [FAMILIES[n][0] for n in names], [FAMILIES[n][1] for n in names]
    for dtype in ("f64", "f32"):
        Xs = _patches(301, D, dtype)
        Ys = [_targets(X, R) for X in Xs]
        model = _model(Xs, Ys, thetas, dtype)
        assert np.all(model.info() == 0)
        xq, region = _items(302, Xs, COUNTS, dtype)
        q = _explicit_query(model, xq, region)
        q.items_multi_fitted(False)
        q.items_grad()                                               # theta = None: the model's own per-patch kernels
        G, _ = q.item_grads()
        worst = _item_ratios(G, xq, region, Xs, model.weights_multi(), oths, [None] * 8, np.zeros(8), U_OF[dtype])
        _record(test="items_mixed", dtype=dtype, ratio=worst)
        assert worst <= 1.0, worst
    # every patch Spline34 through fit_patches: the per-patch Spline34 instantiation equals the uniform one bit for bit
    Xs = _patches(303, D, "f64")
    Ys = [_targets(X, R) for X in Xs]
    th = FAMILIES["spline34"][0]
    xq, region = _items(304, Xs, COUNTS, "f64")
    out = []
    for theta, own in ((th, False), ([th] * 8, True)):
        q = _explicit_query(_model(Xs, Ys, theta), xq, region)
        q.items_multi(th, False)
        q.items_grad(None if own else th)
        out.append(q.item_grads()[0])
    assert np.array_equal(out[0], out[1])


@pytest.mark.parametrize("family", ["spline34", "spline12", "spline32"])
def test_coincident_point_and_outside_every_support(family):
    D, R = 3, 2
    th, oth = FAMILIES[family]
    Xs = _patches(400, D, "f64")
    Ys = [_targets(X, R) for X in Xs]
    far = np.array([[50.0, -40.0, 9.0], [-7.0, 300.0, 0.0]])
    for trend in (None, "linear"):
        model = _model(Xs, Ys, th, "f64", trend)
        Cs = model.weights_multi()
        betas = model.trend()[0] if trend else [None] * 8
        for r in (4, 6):
            x0 = Xs[r][5]
            q = _explicit_query(model, np.vstack([x0[None, :], far]), np.full(3, r))
            q.items_multi(th, False)
            q.items_grad(th)
            G, _ = q.item_grads()
            # the coinciding training point contributes 0: the reference without it is the reference
            keep = np.arange(len(Xs[r])) != 5
            ref = np.asarray(GR.item_grad_ref(oth, Xs[r][keep], Cs[r][keep], x0, betas[r])).T
            bound = (len(Xs[r]) + 32) * U_OF["f64"] * GR.lip(oth) * np.abs(Cs[r]).sum(0)
            assert np.all(np.isfinite(G[0]))
            assert np.all(np.abs(np.asarray(G[0], dtype=GR.LD) - ref).astype(np.float64) <= bound[:, None])
            # outside the support a spline's psi is exactly 0: G is exactly 0, or exactly the slope of the linear trend
            want = np.zeros((R, D)) if trend is None else betas[r][1:].T
            assert np.array_equal(G[1], want) and np.array_equal(G[2], want), (family, trend, r)


# ------------------------------------------------------------------------------------------ the blend
class Blend:
    """a tree, its eps-sets as patches, a fitted multi-output model and planned queries"""

    def __init__(self, D, R, family, trend, dtype="f64", diag_patch=None, radius=0.8, seed=7, N=480, nq=160):
        rng = np.random.default_rng(seed + D)
        self.D, self.R, self.radius, self.delta, self.levels = D, R, radius, 1e-5, 4
        self.X = _round(rng.uniform(-4, 4, (N, D)), dtype)
        self.Xq = rng.uniform(-3.9, 3.9, (nq, D))
        self.root, _, _ = pmk.setuppartition(self.X, self.levels)
        self.Xs, self.inds, _, _ = pmk.organizetrainingsets(self.root, self.levels, self.X, 0.3)
        self.th, self.oth = FAMILIES[family]
        self.wth, self.owth = pmk.Spline34KernelType(1 / radius), O.kernel(O.SPLINE34, 1 / radius)
        Ys = [_targets(x, R) for x in self.Xs]
        diag = None
        if diag_patch is not None:
            diag = [np.zeros(len(x)) for x in self.Xs]
            diag[diag_patch][3] = -3.0                      # the factorisation of this patch fails (tests/test_gpu_breakdown.py)
        self.model = M.DeviceModel(self.Xs, [np.ascontiguousarray(y[:, 0]) for y in Ys], dtype=dtype)
        if diag is not None:
            self.model.set_diag(diag)
        self.model.fit(self.th, SIGMA2[dtype])
        self.model.set_targets_multi(Ys)
        self.model.set_trend(trend)
        self.model.solve_multi()
        self.model.set_bsp(self.root, 0)
        self.hp_v, self.hp_c = hyperplane_arrays(self.root)

    def staged(self, Xq=None, radius=None):
        q = M.DeviceQuery(self.model, self.Xq if Xq is None else Xq)
        q.plan(self.radius if radius is None else radius, self.delta)
        q.items_multi(self.th, False)
        q.items_grad(self.th)
        q.mix_multi(self.wth)
        q.mix_grad(self.wth)
        return q


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _plane_t(v, c, x, dot_mode):
    """c - v . x as plan_kernel forms it: the dot product sequentially (mode 0) or as an fma chain (mode 1), then -s + c"""
    s = np.float64(v[0]) * np.float64(x[0])
    for d in range(1, len(x)):
        s = np.float64(_fma(v[d], x[d], s)) if dot_mode else s + np.float64(v[d]) * np.float64(x[d])
    return -s + np.float64(c)


BLEND_CASES = [(2, 3, "spline34", None, "f64"), (2, 2, "gaussian", "linear", "f64"), (3, 1, "rq", "constant", "f64"),
               (3, 16, "spline32", None, "f32"), (1, 3, "modsqexp", "linear", "f64")]


@pytest.mark.parametrize("D,R,family,trend,dtype", BLEND_CASES)
def test_blend_against_the_reference_fed_with_the_devices_items(D, R, family, trend, dtype):
    b = Blend(D, R, family, trend, dtype)
    q = M.DeviceQuery(b.model, b.Xq)
    q.plan(b.radius, b.delta)
    q.items_multi(b.th, False)
    q.mix_multi(b.wth)
    Y0, _ = q.fetch_multi(R)
    U0, _ = q.item_values_multi()
    q.items_grad(b.th)
    q.mix_grad(b.wth)
    dY = q.fetch_grad()
    assert dY.shape == (len(b.Xq), R, D)
    # the means keep their bits through the gradient calls
    assert np.array_equal(q.fetch_multi(R)[0], Y0) and np.array_equal(q.item_values_multi()[0], U0)
    dbg = q.debug()
    G, plane = q.item_grads()
    off, t, reg = dbg["item_offsets"], dbg["item_t"], dbg["item_region"]
    assert np.all(np.isfinite(dY))
    # plane is -1 exactly for the home items (the last of every query); a neighbour's t is c - v . x of its plane, bit for bit
    home_items = off[1:] - 1
    is_home = np.zeros(len(t), dtype=bool)
    is_home[home_items] = True
    assert np.array_equal(plane == -1, is_home)
    assert np.array_equal(reg[home_items], dbg["home"])
    dot_mode = pmk.lib().pmk_bsp_dot_mode(M._native(b.root).h)
    n_nb = 0
    for j in range(len(b.Xq)):
        for it in range(off[j], off[j + 1] - 1):
            assert 0 <= plane[it] < len(b.hp_c)
            assert _plane_t(b.hp_v[plane[it]], b.hp_c[plane[it]], b.Xq[j], dot_mode) == t[it], (j, it)
            n_nb += 1
    assert n_nb >= 20                                           # the workload exercises the blend
    worst = 0.0
    for j in range(len(b.Xq)):
        items = range(off[j], off[j + 1])
        ref, mag = GR.mix_grad_ref(items, G, U0, t, plane, b.hp_v, b.owth)
        bound = 16 * len(items) * 2.0 ** -53 * mag.astype(np.float64)
        err = np.abs(np.asarray(dY[j], dtype=GR.LD) - ref).astype(np.float64)
        worst = max(worst, _worst_ratio(err, bound))
        assert np.all(err <= bound), (j, err, bound)
    _record(test="blend", D=D, R=R, family=family, trend=trend, dtype=dtype, ratio=worst, neighbour_items=n_nb)


def test_radius_zero_is_the_home_items_gradient():
    b = Blend(2, 3, "spline34", "linear")
    q = b.staged(radius=0.0)
    assert q.total == len(b.Xq)
    G, plane = q.item_grads()
    assert np.all(plane == -1)
    assert np.array_equal(q.fetch_grad(), G)


def _predict_fitted(b, Xq):
    Xq = np.ascontiguousarray(Xq)
    Y = np.empty((len(Xq), b.R), order="F")
    w = b.wth.desc()
    _lib.check(pmk.lib().pmk_predict_mixture_multi_fitted(b.model.h, C.byref(w), len(Xq), M._d(Xq), b.radius, b.delta, M._d(Y),
                                                          len(Xq), None), "pmk_predict_mixture_multi_fitted")
    return Y


def _fd_ratio(b, trend, Xc, stencil, sigs, dY, h, oths, Xs, u=2.0 ** -53, check=True):
    """the central-difference rule: fd_h = (f(x + h e_d) - f(x - h e_d)) / 2h of pmk_predict_mixture_multi_fitted against
    dY [len(Xc), R, D], tolerance |fd_2h - fd_h| + 2 eps_f / h per component, asserted unless check is False ->
    (worst err / tol, median over the queries of the largest tol / the largest |dY|).  b: .model, .wth, .radius, .delta,
    .R; stencil(x): the points x +- h e_d, x +- 2h e_d per d; sigs: (home, neighbour regions) per query; oths, Xs: the
    oracle kernel and the points of every patch; u: the unit roundoff of the model's items"""
    D, R = Xc.shape[1], b.R
    Yfd = _predict_fitted(b, np.vstack([p for x in Xc for p in stencil(x)])).reshape(len(Xc), D, 4, R)
    # eps_f of one device prediction: the blend is a convex combination of items, each n products and sums
    Cs = b.model.weights_multi()
    betas = b.model.trend()[0] if trend else [None] * len(Cs)
    worst, rel = 0.0, []
    for k, x in enumerate(Xc):
        home, reg = sigs[k]
        mag = np.zeros(R)
        for r in list(reg) + [home]:
            a = np.abs(O.cross_kernel_matrix(oths[r], x[None, :], Xs[r])[0]) @ np.abs(Cs[r])
            n = len(Xs[r])
            if betas[r] is not None and len(betas[r]):
                hb = np.concatenate([[1.0], x])[:len(betas[r])]
                a, n = a + np.abs(hb) @ np.abs(betas[r]), n + len(hb)
            mag = np.maximum(mag, (n + len(reg) + 9) * a)
        eps_f = u * mag
        tols = []
        for d in range(D):
            fp, fm, fp2, fm2 = Yfd[k, d]
            fd_h, fd_2h = (fp - fm) / (2 * h), (fp2 - fm2) / (4 * h)
            tol = np.abs(fd_2h - fd_h) + 2 * eps_f / h
            err = np.abs(fd_h - dY[k, :, d])
            worst = max(worst, float((err / tol).max()))
            tols.append(float(tol.max()))
            assert not check or np.all(err <= tol), (k, d, err, tol)
        rel.append(max(tols) / max(float(np.abs(dY[k]).max()), 1e-300))
    return worst, float(np.median(rel))


@pytest.mark.parametrize("D,R,family,trend", [(2, 2, "spline34", None), (2, 2, "rq", "linear"), (3, 1, "gaussian", "constant")])
def test_device_gradient_equals_central_differences_of_the_device_predictor(D, R, family, trend):
    b = Blend(D, R, family, trend)
    ob = O.BSP(b.X, b.levels)
    h = 8.0 * 2.0 ** -17                                        # 2^-17 of the domain width

    def signature(x):
        home = ob.findpartition(x)
        reg, _, _, keep = ob.neighbours(x, b.radius, b.delta, home)
        return home, tuple(int(r) for r in reg), tuple(np.nonzero(keep)[0])

    def stencil(x):
        return [x + s * h * np.eye(D)[d] for d in range(D) for s in (1, -1, 2, -2)]

    kept = [j for j, x in enumerate(b.Xq) if all(signature(p) == signature(x) for p in stencil(x))]
    with_nb = [j for j in kept if signature(b.Xq[j])[1]]
    pick = (with_nb[:8] + [j for j in kept if j not in with_nb[:8]])[:16]
    assert len(pick) == 16 and len(with_nb) >= 2
    Xc = b.Xq[pick]
    q = b.staged(Xc)
    worst, _ = _fd_ratio(b, trend, Xc, stencil, [signature(x)[:2] for x in Xc], q.fetch_grad(), h, [b.oth] * len(b.Xs), b.Xs)
    _record(test="blend_fd", D=D, R=R, family=family, trend=trend, ratio=worst, with_neighbours=len([j for j in pick if j in with_nb]))


def test_one_shot_equals_the_staged_calls():
    for trend in (None, "linear"):
        b = Blend(2, 3, "spline34", trend)
        q = M.DeviceQuery(b.model, b.Xq)
        q.plan(b.radius, b.delta)
        q.items_multi_fitted(False)
        q.items_grad()
        q.mix_multi(b.wth)
        q.mix_grad(b.wth)
        Ys, dYs = q.fetch_multi(b.R)[0], q.fetch_grad()
        Nq = len(b.Xq)
        Y1, buf = np.empty((Nq, b.R), order="F"), np.empty((b.R, b.D, Nq + 3))
        w = b.wth.desc()
        Xc = np.ascontiguousarray(b.Xq)
        _lib.check(pmk.lib().pmk_predict_mixture_grad_fitted(b.model.h, C.byref(w), Nq, M._d(Xc), b.radius, b.delta, M._d(Y1), Nq,
                                                             M._d(buf), Nq + 3), "pmk_predict_mixture_grad_fitted")
        assert np.array_equal(Y1, Ys)
        assert np.array_equal(buf[:, :, :Nq].transpose(2, 0, 1), dYs)
        # and the model's own kernels equal the same theta passed explicitly
        assert np.array_equal(b.staged().fetch_grad(), dYs)
    # the front end
    X, Xq = b.X, b.Xq[:40]
    eta = pmk.MixtureGPType(b.Xs, pmk.fetchhyperplanes(b.root))
    Yall = _targets(X, 2)
    pmk.fitmixtureGP_trend_(eta, [Yall[i] for i in b.inds], b.th, 1e-2, trend="linear")
    Yq, dYq = pmk.querymixtureGP_grad(Xq, eta, b.root, b.levels, b.radius, b.delta, b.th, 1e-2, b.wth)
    assert Yq.shape == (40, 2) and dYq.shape == (40, 2, 2) and np.all(np.isfinite(dYq))
    Ym, _ = pmk.querymixtureGP_multi(Xq, eta, b.root, b.levels, b.radius, b.delta, b.th, 1e-2, b.wth, variance=False)
    assert np.array_equal(Yq, Ym)


def test_failed_patch_gives_nan_and_the_rest_keep_their_bits():
    sound, broken = Blend(2, 3, "spline34", "constant"), Blend(2, 3, "spline34", "constant", diag_patch=2)
    assert broken.model.info()[2] != 0 and np.all(np.delete(broken.model.info(), 2) == 0)
    qs, qb = sound.staged(), broken.staged()
    Gs, _ = qs.item_grads()
    Gb, _ = qb.item_grads()
    dbg = qb.debug()
    reg, off = dbg["item_region"], dbg["item_offsets"]
    bad_item = reg == 2
    assert bad_item.any() and not bad_item.all()
    assert np.all(np.isnan(Gb[bad_item])) and np.array_equal(Gb[~bad_item], Gs[~bad_item])
    bad_q = np.array([bad_item[off[j]:off[j + 1]].any() for j in range(len(sound.Xq))])
    dYs, dYb = qs.fetch_grad(), qb.fetch_grad()
    assert bad_q.any() and not bad_q.all()
    assert np.all(np.isnan(dYb[bad_q])) and np.array_equal(dYb[~bad_q], dYs[~bad_q])


# ------------------------------------------------------------------------------------------ refusals
def test_refusals():
    L = pmk.lib()
    b = Blend(2, 2, "spline34", None, N=240, nq=40)
    d, w = b.th.desc(), b.wth.desc()
    bb = pmk.BrownianBridge10(1.0).desc()
    q = M.DeviceQuery(b.model, b.Xq)
    assert L.pmk_query_items_grad(q.h, C.byref(d)) == -1                     # before the plan
    q.plan(b.radius, b.delta)
    assert L.pmk_query_items_grad(q.h, C.byref(d)) == -2                     # before items_multi
    assert L.pmk_query_get_items_grad(q.h, None, 0, None) == 0               # the planes alone need only the plan
    q.items_multi(b.th, False)
    assert L.pmk_query_mix_grad(q.h, C.byref(w), 0, q.Nq) == -2              # mix_grad before items_grad
    assert L.pmk_query_items_grad(q.h, C.byref(bb)) == -2                    # a Brownian-bridge theta ...
    assert b"PMK_BB10" in L.pmk_last_error()
    msq = pmk.ModulatedSqExpKernelType(2.0, 1.3).desc()
    assert L.pmk_query_items_grad(q.h, C.byref(msq)) == -2                   # ModSqExp at D = 2
    assert L.pmk_query_items_grad(q.h, C.byref(d)) == 0
    assert L.pmk_query_mix_grad(q.h, C.byref(bb), 0, q.Nq) == -2             # ... and a Brownian-bridge weight kernel
    assert b"PMK_BB10" in L.pmk_last_error()
    buf = np.empty((b.R, b.D, q.Nq))
    assert L.pmk_query_fetch_grad(q.h, M._d(buf), q.Nq) == -2                # fetch before mix_grad
    assert L.pmk_query_mix_grad(q.h, C.byref(w), 0, q.Nq) == 0
    assert L.pmk_query_fetch_grad(q.h, M._d(buf), q.Nq - 1) == -4
    assert L.pmk_query_fetch_grad(q.h, M._d(buf), q.Nq) == 0
    # a new plan discards the gradients, as it does the items
    q.plan(b.radius, b.delta)
    assert L.pmk_query_mix_grad(q.h, C.byref(w), 0, q.Nq) == -2
    assert L.pmk_query_fetch_grad(q.h, M._d(buf), q.Nq) == -2
    # stale weights: set_trend, and a new fit
    q.items_multi(b.th, False)
    b.model.set_trend("constant")
    assert L.pmk_query_items_grad(q.h, C.byref(d)) == -3
    b.model.solve_multi()
    q.items_multi(b.th, False)
    assert L.pmk_query_items_grad(q.h, C.byref(d)) == 0
    b.model.fit(b.th, 2e-2)
    assert L.pmk_query_items_grad(q.h, C.byref(d)) == -3
    # a model built from factors holds no kernels: th == NULL is refused, an explicit theta serves
    src = Blend(2, 2, "spline34", None, N=240, nq=40)
    loaded = M.DeviceModel.from_factors(src.Xs, src.model.weights(), [src.model.get(r, M.GET_L) for r in range(len(src.Xs))])
    loaded.set_targets_multi([_targets(x, 2) for x in src.Xs])
    loaded.solve_multi()
    loaded.set_bsp(src.root, 0)
    ql = M.DeviceQuery(loaded, src.Xq)
    ql.plan(src.radius, src.delta)
    ql.items_multi(src.th, False)
    assert L.pmk_query_items_grad(ql.h, None) == -3
    with pytest.raises(_lib.PmkError, match="holds no kernels"):
        ql.items_grad()
    assert L.pmk_query_items_grad(ql.h, C.byref(d)) == 0
    ql.mix_multi(src.wth)
    ql.mix_grad(src.wth)
    assert np.array_equal(ql.fetch_grad(), src.staged().fetch_grad())        # the same factor bits, the same gradient


def test_refused_after_the_blended_leave_one_out():
    L = pmk.lib()
    rng = np.random.default_rng(3)
    X = rng.uniform(-4, 4, (240, 2))
    root, _, _ = pmk.setuppartition(X, 3)
    th, wth = pmk.Spline34KernelType(1 / 3.0), pmk.Spline34KernelType(1 / 0.8)
    eta = pmk.MixtureGPType.from_tree(root, X, eps=0.3, hps=pmk.fetchhyperplanes(root))
    pmk.fitmixtureGP_multi_(eta, np.asfortranarray(_targets(X, 2)), th, 1e-2)
    model = eta._model
    model.loo()
    q = M.DeviceQuery(model, X)
    q.plan(0.8, 1e-5)
    q.items_loo_multi(False, False)
    d = th.desc()
    assert L.pmk_query_items_grad(q.h, C.byref(d)) == -2                     # a member item is a lookup, not a function of x
    assert b"lookup" in L.pmk_last_error()
    q.items_multi_fitted(False)
    q.items_grad()
    q.mix_multi(wth)
    q.mix_grad(wth)
    assert np.all(np.isfinite(q.fetch_grad()))
    # the device-to-device fetch
    import torch
    dev = torch.empty((2, 2, len(X)), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    q.fetch_grad_into(dev)
    model.ctx.synchronize()
    assert np.array_equal(dev.cpu().numpy().transpose(2, 0, 1), q.fetch_grad())
