"""Gradient of the blended variance on the GPU (pmk_query_items_vgrad / _mix_vgrad / _fetch_vgrad / _get_items_vgrad,
pmk_predict_mixture_vgrad_fitted; the kernels of pmk_vgrad.hip).

Reference: tests/_vgrad_refs.py, the numpy.longdouble restatement that tests/test_vgrad_refs.py pins to the oracle.

Per-item gradients against PatchRef (its own Cholesky of the points the device sees; in fp32 the points and queries are
rounded to float32 first).  The error unit is that of _vgrad_refs.py,
    e_d = (n + 32) u [ kappa2(L) |V|_2 |W_d|_2 + t_d ],   u = 2^-53 (fp64) or 2^-24 (fp32),   t_d the trend's first-order unit,
and every ratio err / e_d must stay <= 10, the bound the blended leave-one-out tests use for their cond2 u units.
Under a trend the trend's part is checked on its own as well: the same model without the trend gives the simple-kriging
part with the same bits, the difference of the two device results is the trend's part within two double roundings of
the whole gradient, and it must stay within ONE unit of its own, (n + 32) u t_d (a first-order worst case): in fp32
the first term of e_d is larger than the whole trend part and the check of the sum alone would not see it.
A patch of one point near the edge of a compact support has a tolerance of its own (test_one_point_patch_near_the_edge).
kappa2(L_r) <= 10^3 is asserted for every patch.  tests/test_vgrad_refs.py checks on the same inputs that a float64
numpy / LAPACK evaluation of the formula stays below one unit.

Blend.  fetch_vgrad against mix_vgrad_ref fed with the device's own items,
    |err| <= 16 m 2^-53 sum_i (|wn_i^2 GV_i| + |2 wn_i v_i d wn_i|)   for a query of m items,
and, end to end, against central differences of the device's own Vq (pmk_predict_mixture_multi_fitted) under the rule of
tests/test_grad_refs.py: |fd_h - dVq| <= |fd_2h - fd_h| + 2 eps_f / h on queries whose neighbour signature is constant
over the stencil, eps_f = (n + 32) u v_unit of the worst item.

Every measured ratio is printed ("VGRAD {json}", run with -s) and a run of the whole module writes them to
profiles/vgrad_accuracy.json.
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
import _vgrad_refs as VR
from test_gpu_grad import FAMILIES, U_OF, Blend, _explicit_query, _model, _targets, _tree8, _worst_ratio

pytestmark = pytest.mark.gpu

SIGMA2 = VR.SIGMA2
COUNTS = [5, 3, 17, 4, 6, 9, 0, 2]              # items per region, rotated per case
RATIO_MAX = 10.0
TREND_RATIO_MAX = 1.0          # the trend's part against its own first-order unit (tests/_vgrad_refs.py)

_RECORDS = []
ACCURACY_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "vgrad_accuracy.json")


def _record(**kw):
    _RECORDS.append(kw)
    print("VGRAD " + json.dumps(kw, sort_keys=True))


@pytest.fixture(scope="module", autouse=True)
def _write_accuracy_file():
    """only a run of the whole module replaces the file"""
    yield
    if {r["test"] for r in _RECORDS} >= {"items", "items_mixed", "blend", "blend_fd"}:
        with open(ACCURACY_JSON, "w") as f:
            f.write("[\n" + ",\n".join(" " + json.dumps(r, sort_keys=True) for r in _RECORDS) + "\n]\n")


def _item_ratios(GV, xq, region, Xs, oths, dtype, trend, flagged, GV0=None):
    """worst err / e_d over the items, the largest kappa2(L), and with GV0 (the same model's gradients without the trend)
    the worst error of the trend's part GV - GV0 over its own unit; NaN exactly where the patch is flagged"""
    worst, kappa, worst_trend = 0.0, 0.0, 0.0
    u = U_OF[dtype]
    for r in sorted(set(int(x) for x in region)):
        sel = np.nonzero(region == r)[0]
        if flagged[r]:
            assert np.all(np.isnan(GV[sel])), r
            continue
        ref = VR.PatchRef(oths[r], Xs[r], SIGMA2[dtype], trend)
        kappa = max(kappa, ref.kappa()[0])
        out = ref.items(xq[sel])
        assert not out["clamped"].any()
        assert np.all(np.isfinite(GV[sel])), r
        err = np.abs(np.asarray(GV[sel], dtype=VR.LD) - out["grad"]).astype(np.float64)
        worst = max(worst, _worst_ratio(err, (len(Xs[r]) + 32) * u * out["unit"]))
        if GV0 is not None:
            assert np.all(np.isfinite(GV0[sel])), r
            part = np.asarray(GV[sel], dtype=VR.LD) - np.asarray(GV0[sel], dtype=VR.LD)
            err = np.abs(part - out["trend"]).astype(np.float64)
            round2 = 4 * 2.0 ** -53 * np.abs(out["grad"]).astype(np.float64)      # the device's sum and this difference
            worst_trend = max(worst_trend, _worst_ratio(np.maximum(err - round2, 0.0), (len(Xs[r]) + 32) * u * out["tunit"]))
    return (worst, kappa) if GV0 is None else (worst, kappa, worst_trend)


ITEM_CASES = [(D, "spline34", "f64", None) for D in (1, 2, 3, 4)] + \
             [(2, fam, "f64", None) for fam in ("spline12", "spline32", "gaussian", "rq", "trq")] + \
             [(1, "modsqexp", "f64", None), (2, "spline34", "f32", None), (3, "rq", "f32", None), (4, "spline34", "f32", None),
              (2, "spline34", "f64", "constant"), (2, "gaussian", "f64", "linear"), (3, "spline34", "f64", "linear"),
              (4, "rq", "f64", "constant"), (1, "spline12", "f64", "linear"), (2, "spline32", "f32", "linear"), (3, "gaussian", "f32", "constant"),
              (1, "rq", "f32", "linear")]


@pytest.mark.parametrize("D,family,dtype,trend", ITEM_CASES)
def test_item_variance_gradients(D, family, dtype, trend):
    case = ITEM_CASES.index((D, family, dtype, trend))
    th, oth = FAMILIES[family]
    Xs = VR.case_patches(100 + case, D, dtype)
    Ys = [_targets(X, 2) for X in Xs]
    model = _model(Xs, Ys, th, dtype, trend)
    assert np.all(model.info() == 0)
    xq, region = VR.case_items(200 + case, Xs, list(np.roll(COUNTS, case)), dtype)
    q = _explicit_query(model, xq, region)
    q.items_multi(th, True)
    U0, v0 = q.item_values_multi()
    q.items_vgrad(th)
    GV = q.item_vgrads()
    assert GV.shape == (len(xq), D)
    U1, v1 = q.item_values_multi()
    assert np.array_equal(U1, U0, equal_nan=True) and np.array_equal(v1, v0, equal_nan=True)     # the items keep their bits
    tinfo = model.trend_info() if trend else np.zeros(len(Xs), dtype=np.int32)
    if trend == "linear":
        assert [int(f != 0) for f in tinfo] == [int(n < 1 + D) for n in VR.SIZES]     # n < q points: flagged, NaN
    # one home item per query with weight 1: the blend returns the item's gradient bit for bit
    w = pmk.Spline34KernelType(1.0)
    q.mix_multi(w)
    q.mix_vgrad(w)
    assert np.array_equal(q.fetch_vgrad(), GV, equal_nan=True)
    if trend:
        # the trend's part on its own: the same factor without the trend gives the simple-kriging part
        model.set_trend(None)
        model.solve_multi()
        q0 = _explicit_query(model, xq, region)
        q0.items_multi(th, True)
        q0.items_vgrad(th)
        worst, kappa, worst_trend = _item_ratios(GV, xq, region, Xs, [oth] * len(Xs), dtype, trend, tinfo != 0, q0.item_vgrads())
        _record(test="items", D=D, family=family, dtype=dtype, trend=trend, ratio=worst, kappa=kappa, trend_ratio=worst_trend)
        assert worst_trend <= TREND_RATIO_MAX, worst_trend
    else:
        worst, kappa = _item_ratios(GV, xq, region, Xs, [oth] * len(Xs), dtype, trend, tinfo != 0)
        _record(test="items", D=D, family=family, dtype=dtype, trend=trend, ratio=worst, kappa=kappa)
    assert kappa <= VR.KAPPA_MAX, kappa
    assert worst <= RATIO_MAX, worst


def test_mixed_families_per_patch_and_the_models_own_kernels():
    D = 2
    names = ["spline34", "gaussian", "rq", "spline12", "trq", "spline32", "spline34", "rq"]
    thetas, oths = [FAMILIES[n][0] for n in names], [FAMILIES[n][1] for n in names]
    for dtype in ("f64", "f32"):
        Xs = VR.case_patches(301, D, dtype)
        model = _model(Xs, [_targets(X, 2) for X in Xs], thetas, dtype)
        assert np.all(model.info() == 0)
        xq, region = VR.case_items(302, Xs, COUNTS, dtype)
        q = _explicit_query(model, xq, region)
        q.items_multi_fitted(True)
        q.items_vgrad()                                              # theta = None: the model's own per-patch kernels
        worst, kappa = _item_ratios(q.item_vgrads(), xq, region, Xs, oths, dtype, None, np.zeros(8, dtype=bool))
        _record(test="items_mixed", dtype=dtype, ratio=worst, kappa=kappa)
        assert kappa <= VR.KAPPA_MAX and worst <= RATIO_MAX, (kappa, worst)
    # every patch Spline34 through fit_patches: the per-patch Spline34 instantiation equals the uniform one bit for bit
    Xs = VR.case_patches(303, D, "f64")
    Ys = [_targets(X, 2) for X in Xs]
    th = FAMILIES["spline34"][0]
    xq, region = VR.case_items(304, Xs, COUNTS, "f64")
    out = []
    for theta, own in ((th, False), ([th] * 8, True)):
        q = _explicit_query(_model(Xs, Ys, theta), xq, region)
        q.items_multi(th, True)
        q.items_vgrad(None if own else th)
        out.append(q.item_vgrads())
    assert np.array_equal(out[0], out[1])


# ------------------------------------------------------------------------------------------ strip and wave edges
EDGE_COUNTS = [1, 47, 48, 49, 63, 64, 65, 79, 80, 81, 127, 128, 129, 161, 257]     # cap - 1, cap, cap + 1 of every D


@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_items_keep_their_bits_whatever_shares_their_strip(D):
    th, oth = FAMILIES["spline34"]
    rng = np.random.default_rng(500 + D)
    sizes = [129, 40, 130, 7, 257, 128, 33, 131]
    Xs = [rng.uniform(-2, 2, (n, D)) for n in sizes]
    model = _model(Xs, [_targets(X, 1) for X in Xs], th)
    assert np.all(model.info() == 0)
    seen = {}
    for batch in (EDGE_COUNTS[:8], EDGE_COUNTS[8:] + [0]):
        region = np.concatenate([np.full(c, r, dtype=np.int32) for r, c in enumerate(batch)])
        xq = rng.uniform(-2.5, 2.5, (len(region), D))
        q = _explicit_query(model, xq, region)
        q.items_multi(th, True)
        q.items_vgrad(th)
        GV = q.item_vgrads()
        assert np.all(np.isfinite(GV))
        # the same items in another order, with other companions in front of them and between them
        perm = rng.permutation(len(region))
        extra_r = rng.integers(0, 8, 37).astype(np.int32)
        extra_x = rng.uniform(-2.5, 2.5, (37, D))
        q2 = _explicit_query(model, np.vstack([extra_x[:20], xq[perm], extra_x[20:]]),
                             np.concatenate([extra_r[:20], region[perm], extra_r[20:]]))
        q2.items_multi(th, True)
        q2.items_vgrad(th)
        GV2 = q2.item_vgrads()[20:20 + len(region)]
        assert np.array_equal(GV2, GV[perm])
        # and the values are right at both ends and in the middle of every region's list
        for r, c in enumerate(batch):
            if c == 0:
                continue
            sel = np.nonzero(region == r)[0]
            pick = sel[sorted({0, c // 2, c - 1})]
            if r not in seen:
                seen[r] = VR.PatchRef(oth, Xs[r], SIGMA2["f64"])
            out = seen[r].items(xq[pick])
            err = np.abs(np.asarray(GV[pick], dtype=VR.LD) - out["grad"]).astype(np.float64)
            assert _worst_ratio(err, (sizes[r] + 32) * U_OF["f64"] * out["unit"]) <= RATIO_MAX, (D, r, c)


@pytest.mark.parametrize("family", ["spline34", "spline12", "spline32"])
def test_outside_every_support_is_exactly_zero(family):
    D = 3
    th, _ = FAMILIES[family]
    Xs = VR.case_patches(400, D, "f64")
    model = _model(Xs, [_targets(X, 2) for X in Xs], th)
    far = np.array([[50.0, -40.0, 9.0], [-7.0, 300.0, 0.0], [0.3, 0.1, -0.2]])
    for r in (1, 5):
        q = _explicit_query(model, far, np.full(3, r))
        q.items_multi(th, True)
        q.items_vgrad(th)
        GV = q.item_vgrads()
        assert np.array_equal(GV[:2], np.zeros((2, D))) and not np.signbit(GV[:2]).any()
        assert np.all(GV[2] != 0)


@pytest.mark.parametrize("family,dtype", [("spline34", "f64"), ("spline34", "f32"), ("spline12", "f64"), ("spline32", "f32")])
def test_one_point_patch_near_the_edge_of_its_support(family, dtype):
    """What the unit of the other tests leaves out: t = 1 - r has lost digits near the support's edge, and with one point
    nothing else carries the sum.  There the gradient is the closed form -2 phi(tau) psi(tau) (x - z) / (k(0) + sigma2),
    and its error is that of phi psi.  The distance carries about 2.5 u (differences, squares, sum, root), the scale a
    as the model's real number one u, the product r = a tau one more: r, close to 1, is within 5 u, and so is t = 1 - r,
    which is 5 u / t relatively.  phi psi is t^p times a polynomial in r of a few u, p = 11, 5 and 7 for Spline34, 12
    and 32.  Tolerance: (32 + 5 p / t) u |gradient|, t taken at the query."""
    D, p = 2, {"spline34": 11, "spline12": 5, "spline32": 7}[family]
    th, oth = FAMILIES[family]
    Xs = VR.case_patches(700, D, dtype)
    model = _model(Xs, [_targets(X, 1) for X in Xs], th, dtype)
    z, u, support = Xs[0][0], U_OF[dtype], 1.0 / oth.p[0]
    fr = np.array([0.5, 0.9, 0.99, 0.999])
    ang = np.array([0.3, 1.1, 2.9, 4.0])
    xq = z[None, :] + (fr * support)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    if dtype == "f32":
        xq = xq.astype(np.float32).astype(np.float64)
    q = _explicit_query(model, xq, np.zeros(len(xq), dtype=np.int32))
    q.items_multi(th, True)
    q.items_vgrad(th)
    GV = q.item_vgrads()
    out = VR.PatchRef(oth, Xs[0], SIGMA2[dtype]).items(xq)
    t = 1.0 - np.sqrt(((xq - z) ** 2).sum(1)) / support
    assert np.all(t > 0) and t.min() < 2e-3
    tol = ((32 + 5 * p / t) * u)[:, None] * np.abs(out["grad"]).astype(np.float64)
    err = np.abs(np.asarray(GV, dtype=VR.LD) - out["grad"]).astype(np.float64)
    worst = _worst_ratio(err, tol)
    _record(test="edge", family=family, dtype=dtype, ratio=worst, t_min=float(t.min()))
    assert worst <= 1.0, worst


# ------------------------------------------------------------------------------------------ the blend
def _staged(b, Xq=None, radius=None, own=False):
    q = M.DeviceQuery(b.model, b.Xq if Xq is None else Xq)
    q.plan(b.radius if radius is None else radius, b.delta)
    if own:
        q.items_multi_fitted(True)
        q.items_grad()
        q.items_vgrad()
    else:
        q.items_multi(b.th, True)
        q.items_grad(b.th)
        q.items_vgrad(b.th)
    q.mix_multi(b.wth)
    q.mix_grad(b.wth)
    q.mix_vgrad(b.wth)
    return q


BLEND_CASES = [(2, "spline34", None, "f64"), (2, "gaussian", "linear", "f64"), (3, "rq", "constant", "f64"),
               (3, "spline32", None, "f32"), (1, "modsqexp", "linear", "f64"), (2, "spline34", "linear", "f32")]


@pytest.mark.parametrize("D,family,trend,dtype", BLEND_CASES)
def test_blend_against_the_reference_fed_with_the_devices_items(D, family, trend, dtype):
    b = Blend(D, 2, family, trend, dtype)
    q = M.DeviceQuery(b.model, b.Xq)
    q.plan(b.radius, b.delta)
    q.items_multi(b.th, True)
    q.items_grad(b.th)
    q.mix_multi(b.wth)
    q.mix_grad(b.wth)
    Y0, V0 = q.fetch_multi(2)
    U0, v0 = q.item_values_multi()
    dY0 = q.fetch_grad()
    q.items_vgrad(b.th)
    q.mix_vgrad(b.wth)
    dV = q.fetch_vgrad()
    assert dV.shape == (len(b.Xq), D) and np.all(np.isfinite(dV))
    # u, v, Y, V and dY of the query keep their bits through the variance-gradient calls
    Y1, V1 = q.fetch_multi(2)
    U1, v1 = q.item_values_multi()
    assert np.array_equal(Y1, Y0) and np.array_equal(V1, V0) and np.array_equal(U1, U0) and np.array_equal(v1, v0)
    assert np.array_equal(q.fetch_grad(), dY0)
    dbg = q.debug()
    GV = q.item_vgrads()
    _, plane = q.item_grads()
    off, t = dbg["item_offsets"], dbg["item_t"]
    worst, n_nb = 0.0, int((plane >= 0).sum())
    assert n_nb >= 20                                           # the workload exercises the blend
    for j in range(len(b.Xq)):
        items = range(off[j], off[j + 1])
        ref, mag = VR.mix_vgrad_ref(items, GV, v0, t, plane, b.hp_v, b.owth)
        bound = 16 * len(items) * 2.0 ** -53 * mag.astype(np.float64)
        err = np.abs(np.asarray(dV[j], dtype=VR.LD) - ref).astype(np.float64)
        worst = max(worst, _worst_ratio(err, bound))
        assert np.all(err <= bound), (j, err, bound)
    _record(test="blend", D=D, family=family, trend=trend, dtype=dtype, ratio=worst, neighbour_items=n_nb)


def test_radius_zero_is_the_home_items_gradient():
    b = Blend(2, 2, "spline34", "linear")
    q = _staged(b, radius=0.0)
    assert q.total == len(b.Xq)
    assert np.array_equal(q.fetch_vgrad(), q.item_vgrads())


def _predict_var(b, Xq):
    Xq = np.ascontiguousarray(Xq)
    Y, V = np.empty((len(Xq), b.R), order="F"), np.empty(len(Xq))
    w = b.wth.desc()
    _lib.check(pmk.lib().pmk_predict_mixture_multi_fitted(b.model.h, C.byref(w), len(Xq), M._d(Xq), b.radius, b.delta, M._d(Y),
                                                          len(Xq), M._d(V)), "pmk_predict_mixture_multi_fitted")
    return V


@pytest.mark.parametrize("D,family,trend", [(2, "spline34", None), (2, "rq", "linear"), (3, "gaussian", "constant")])
def test_device_gradient_equals_central_differences_of_the_device_variance(D, family, trend):
    """fp64 models only: with u = 2^-24 the term 2 eps_f / h is as large as the gradient at any h whose truncation is
    still small, and the rule could not fail"""
    b = Blend(D, 2, family, trend)
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
    dV = _staged(b, Xc).fetch_vgrad()
    Vfd = _predict_var(b, np.vstack([p for x in Xc for p in stencil(x)])).reshape(len(Xc), D, 4)
    refs, worst = {}, 0.0
    for k, x in enumerate(Xc):
        home, reg, _ = signature(x)
        eps_f = 0.0
        for r in list(reg) + [home]:
            if r not in refs:
                refs[r] = VR.PatchRef(b.oth, b.Xs[r], SIGMA2["f64"], trend)
            eps_f = max(eps_f, (len(b.Xs[r]) + 32) * 2.0 ** -53 * float(refs[r].items(x[None, :])["vunit"][0]))
        for d in range(D):
            fp, fm, fp2, fm2 = Vfd[k, d]
            fd_h, fd_2h = (fp - fm) / (2 * h), (fp2 - fm2) / (4 * h)
            tol = abs(fd_2h - fd_h) + 2 * eps_f / h
            err = abs(fd_h - dV[k, d])
            worst = max(worst, err / tol)
            assert err <= tol, (k, d, err, tol)
    _record(test="blend_fd", D=D, family=family, trend=trend, ratio=worst, with_neighbours=len([j for j in pick if j in with_nb]))


# ------------------------------------------------------------------------------------------ behaviour
def test_one_shot_equals_the_staged_calls():
    for trend in (None, "linear"):
        b = Blend(2, 3, "spline34", trend)
        q = _staged(b, own=True)
        (Ys, Vs), dYs, dVs = q.fetch_multi(b.R), q.fetch_grad(), q.fetch_vgrad()
        Nq = len(b.Xq)
        Y1, V1 = np.empty((Nq, b.R), order="F"), np.empty(Nq)
        dY1, dV1 = np.empty((b.R, b.D, Nq + 3)), np.empty((b.D, Nq + 5))
        w = b.wth.desc()
        Xc = np.ascontiguousarray(b.Xq)
        L = pmk.lib()
        _lib.check(L.pmk_predict_mixture_vgrad_fitted(b.model.h, C.byref(w), Nq, M._d(Xc), b.radius, b.delta, M._d(Y1), Nq,
                                                      M._d(V1), M._d(dY1), Nq + 3, M._d(dV1), Nq + 5),
                   "pmk_predict_mixture_vgrad_fitted")
        assert np.array_equal(Y1, Ys) and np.array_equal(V1, Vs)
        assert np.array_equal(dY1[:, :, :Nq].transpose(2, 0, 1), dYs)
        assert np.array_equal(dV1[:, :Nq].T, dVs)
        # any output pointer may be NULL
        dV2 = np.empty((b.D, Nq))
        _lib.check(L.pmk_predict_mixture_vgrad_fitted(b.model.h, C.byref(w), Nq, M._d(Xc), b.radius, b.delta, None, 0, None,
                                                      None, 0, M._d(dV2), Nq), "pmk_predict_mixture_vgrad_fitted")
        assert np.array_equal(dV2.T, dVs)
        # and the model's own kernels equal the same theta passed explicitly
        assert np.array_equal(_staged(b).fetch_vgrad(), dVs)
    # the front end
    eta = pmk.MixtureGPType(b.Xs, pmk.fetchhyperplanes(b.root))
    Yall = _targets(b.X, 2)
    pmk.fitmixtureGP_trend_(eta, [Yall[i] for i in b.inds], b.th, 1e-2, trend="linear")
    Xq = b.Xq[:40]
    Yq, Vq, dYq, dVq = pmk.querymixtureGP_grad(Xq, eta, b.root, b.levels, b.radius, b.delta, b.th, 1e-2, b.wth, variance=True)
    assert Yq.shape == (40, 2) and Vq.shape == (40,) and dYq.shape == (40, 2, 2) and dVq.shape == (40, 2)
    assert np.all(np.isfinite(dVq))
    Ym, Vm = pmk.querymixtureGP_multi(Xq, eta, b.root, b.levels, b.radius, b.delta, b.th, 1e-2, b.wth)
    assert np.array_equal(Yq, Ym) and np.array_equal(Vq, Vm)
    Y2, dY2 = pmk.querymixtureGP_grad(Xq, eta, b.root, b.levels, b.radius, b.delta, b.th, 1e-2, b.wth)     # the default stays
    assert np.array_equal(Y2, Yq) and np.array_equal(dY2, dYq)


def test_failed_patch_gives_nan_and_the_rest_keep_their_bits():
    sound, broken = Blend(2, 2, "spline34", "constant"), Blend(2, 2, "spline34", "constant", diag_patch=2)
    assert broken.model.info()[2] != 0 and np.all(np.delete(broken.model.info(), 2) == 0)
    qs, qb = _staged(sound), _staged(broken)
    Gs, Gb = qs.item_vgrads(), qb.item_vgrads()
    dbg = qb.debug()
    reg, off = dbg["item_region"], dbg["item_offsets"]
    bad_item = reg == 2
    assert bad_item.any() and not bad_item.all()
    assert np.all(np.isnan(Gb[bad_item])) and np.array_equal(Gb[~bad_item], Gs[~bad_item])
    bad_q = np.array([bad_item[off[j]:off[j + 1]].any() for j in range(len(sound.Xq))])
    dVs, dVb = qs.fetch_vgrad(), qb.fetch_vgrad()
    assert bad_q.any() and not bad_q.all()
    assert np.all(np.isnan(dVb[bad_q])) and np.array_equal(dVb[~bad_q], dVs[~bad_q])


def test_trend_flagged_patch_gives_nan_and_the_rest_keep_their_bits():
    D = 2
    th, _ = FAMILIES["spline34"]
    Xs = VR.case_patches(600, D, "f64")
    Ys = [_targets(X, 2) for X in Xs]
    xq, region = VR.case_items(601, Xs, [4] * 8, "f64")
    out = {}
    for name, xs, ys in (("flagged", Xs, Ys), ("sound", [Xs[1][:5]] + Xs[1:], [Ys[1][:5]] + Ys[1:])):
        model = _model(xs, ys, th, "f64", "linear")
        q = _explicit_query(model, xq, region)
        q.items_multi(th, True)
        q.items_vgrad(th)
        out[name] = (q.item_vgrads(), model.trend_info())
    assert out["flagged"][1][0] != 0 and np.all(out["flagged"][1][1:] == 0) and np.all(out["sound"][1] == 0)     # n = 1 < q = 3
    assert np.all(np.isnan(out["flagged"][0][region == 0]))
    assert np.array_equal(out["flagged"][0][region != 0], out["sound"][0][region != 0])
    assert np.all(np.isfinite(out["sound"][0]))


def test_refusals():
    L = pmk.lib()
    b = Blend(2, 2, "spline34", None, N=240, nq=40)
    d, w = b.th.desc(), b.wth.desc()
    bb = pmk.BrownianBridge10(1.0).desc()
    q = M.DeviceQuery(b.model, b.Xq)
    buf = np.empty((b.D, q.Nq))
    assert L.pmk_query_items_vgrad(q.h, C.byref(d)) == -1                    # before the plan
    q.plan(b.radius, b.delta)
    assert L.pmk_query_items_vgrad(q.h, C.byref(d)) == -2                    # before items_multi
    q.items_multi(b.th, False)
    assert L.pmk_query_items_vgrad(q.h, C.byref(d)) == -2                    # after mean-only items
    assert b"want_var = 1" in L.pmk_last_error()
    assert L.pmk_query_get_items_vgrad(q.h, M._d(buf), b.D) == -2
    q.items_multi(b.th, True)
    assert L.pmk_query_mix_vgrad(q.h, C.byref(w), 0, q.Nq) == -2             # mix_vgrad before items_vgrad
    assert L.pmk_query_items_vgrad(q.h, C.byref(bb)) == -2                   # a Brownian-bridge theta ...
    assert b"PMK_BB10" in L.pmk_last_error()
    msq = pmk.ModulatedSqExpKernelType(2.0, 1.3).desc()
    assert L.pmk_query_items_vgrad(q.h, C.byref(msq)) == -2                  # ModSqExp at D = 2
    q.set_diag(np.full(q.Nq, 0.25))
    q.items_multi(b.th, True)
    assert L.pmk_query_items_vgrad(q.h, C.byref(d)) == -2                    # pmk_query_set_diag addends
    assert b"pmk_query_set_diag" in L.pmk_last_error()
    q.set_diag(None)
    q.items_multi(b.th, True)
    assert L.pmk_query_items_vgrad(q.h, C.byref(d)) == 0
    assert L.pmk_query_mix_vgrad(q.h, C.byref(bb), 0, q.Nq) == -2            # ... and a Brownian-bridge weight kernel
    assert L.pmk_query_fetch_vgrad(q.h, M._d(buf), q.Nq) == -2               # fetch before mix_vgrad
    assert L.pmk_query_mix_vgrad(q.h, C.byref(w), 0, q.Nq + 1) == -3
    assert L.pmk_query_mix_vgrad(q.h, C.byref(w), 0, q.Nq) == 0
    assert L.pmk_query_fetch_vgrad(q.h, M._d(buf), q.Nq - 1) == -4
    assert L.pmk_query_get_items_vgrad(q.h, M._d(np.empty((q.total, b.D))), b.D - 1) == -4
    assert L.pmk_query_fetch_vgrad(q.h, M._d(buf), q.Nq) == 0
    # new items, and a new plan, discard the results
    q.items_multi(b.th, True)
    assert L.pmk_query_mix_vgrad(q.h, C.byref(w), 0, q.Nq) == -2
    assert L.pmk_query_items_vgrad(q.h, C.byref(d)) == 0 and L.pmk_query_mix_vgrad(q.h, C.byref(w), 0, q.Nq) == 0
    q.plan(b.radius, b.delta)
    assert L.pmk_query_mix_vgrad(q.h, C.byref(w), 0, q.Nq) == -2
    assert L.pmk_query_fetch_vgrad(q.h, M._d(buf), q.Nq) == -2
    # stale weights: set_trend, and a new fit
    q.items_multi(b.th, True)
    b.model.set_trend("constant")
    assert L.pmk_query_items_vgrad(q.h, C.byref(d)) == -3
    b.model.solve_multi()
    q.items_multi(b.th, True)
    assert L.pmk_query_items_vgrad(q.h, C.byref(d)) == 0
    b.model.fit(b.th, 2e-2)
    assert L.pmk_query_items_vgrad(q.h, C.byref(d)) == -3


def test_refused_after_the_blended_leave_one_out_and_the_device_fetch():
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
    q.items_loo_multi(False, True)
    d = th.desc()
    assert L.pmk_query_items_vgrad(q.h, C.byref(d)) == -2                    # a member item is a lookup, not a function of x
    assert b"lookup" in L.pmk_last_error()
    q.items_multi_fitted(True)
    q.items_vgrad()
    q.mix_multi(wth)
    q.mix_vgrad(wth)
    dV = q.fetch_vgrad()
    assert np.all(np.isfinite(dV))
    import torch
    dev = torch.empty((2, len(X)), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    q.fetch_vgrad_into(dev)
    model.ctx.synchronize()
    assert np.array_equal(dev.cpu().numpy().T, dV)
