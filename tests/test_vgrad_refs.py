"""CPU-side checks of the gradient of the blended variance (no device compute).

1. tests/_vgrad_refs.py is pinned to the oracle, on the workload of tests/test_grad_refs.py (D = 2, 4 leaves of about 40
   points, 64 queries, those kept whose neighbour signature is constant over the stencil):
   item_vgrad_ref against central differences of the oracle's queryinner variance in the query's home patch, and
   mix_vgrad_ref against central differences of the oracle's query_mixture variance, for every stationary family.  Under a
   constant and a linear trend the oracle's variance gets the trend's term |L_G^-1 (h - kq C_H)|^2 added in plain fp64
   (tests/_trend_refs.py), and the blend is put together from the oracle's pieces as test_grad_refs.py does for the mean.
   Tolerance per component, the construction of test_grad_refs.py:  |FD_h - analytic| <= |FD_2h - FD_h| + 2 eps_f / h,
   eps_f = (n + 32) 2^-53 v_unit, the rounding of one variance in the units of _vgrad_refs.py.
2. The clamp: an item whose k(x,x) - b lies below min_v has gradient exactly 0, and so have the oracle's differences.
3. On the inputs of tests/test_gpu_vgrad.py a numpy / LAPACK evaluation of the item formula in the model's own precision
   stays below one error unit e_d, its trend part below one unit of its own, and kappa2(L) <= 10^3 for every patch.
4. The new symbols are in the header, the ctypes table, the library, the host-only stub launchers and the Julia ccalls;
   the argument checks run without a device; the Python front end refuses closure-carrying and Brownian-bridge kernels
   before any device call.
"""
import re

import numpy as np
import pytest
import scipy.linalg as sla

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
from patchmixturekriging_amd import mixture as M
from oracle import oracle as O
from test_julia_binding import header_prototypes, julia_ccalls
from test_multi_output_abi import _cat, _NoDevice
from test_grad_refs import DELTA, FAMILIES, H, RADIUS, SIGMA2, U53, Workload
import _grad_refs as GR
import _trend_refs as T
import _vgrad_refs as VR

NEW = ["pmk_query_items_vgrad", "pmk_query_mix_vgrad", "pmk_query_fetch_vgrad", "pmk_query_fetch_vgrad_dev",
       "pmk_query_get_items_vgrad", "pmk_predict_mixture_vgrad_fitted"]
TRENDS = [None, "constant", "linear"]


@pytest.fixture(scope="module")
def wl():
    return Workload()


class Fit:
    """per patch: the oracle's factor, the fp64 trend operands, and the long-double reference"""

    def __init__(self, wl, th, trend):
        self.wl, self.th, self.trend = wl, th, trend
        self.L, self.c, self.CH, self.LG, self.ref = [], [], [], [], []
        for X, Y in zip(wl.Xs, wl.Ys):
            f = O.fit_patch(th, X, Y[:, 0], SIGMA2)
            assert f["info"] == 0
            self.L.append(f["L"]); self.c.append(f["c_chol"])
            if trend:
                g = T.gls_fp64(O.kernel_matrix(th, X), SIGMA2, Y, T.basis(X, trend))
                self.CH.append(g["C_H"]); self.LG.append(g["LG"])
            self.ref.append(VR.PatchRef(th, X, SIGMA2, trend))

    def var(self, r, x, min_v=1e-12):
        """the oracle's queryinner variance of patch r at x, plus the trend's term in plain fp64"""
        v = O.queryinner(self.th, self.wl.Xs[r], self.c[r], self.L[r], x, min_v)[1]
        if self.trend:
            kq = O.cross_kernel_matrix(self.th, x[None, :], self.wl.Xs[r])[0]
            rho = T.basis(x[None, :], self.trend)[0] - kq @ self.CH[r]
            z = sla.solve_triangular(self.LG[r], rho, lower=True)
            v = v + z @ z
        return v

    def blend(self, x):
        """the blended variance at x: the oracle's query_mixture, or with a trend its blend of the items above"""
        wl = self.wl
        if not self.trend:
            return O.query_mixture(wl.ob, self.th, wl.wth, wl.Xs, self.c, self.L, x[None, :], RADIUS, DELTA)[1][0]
        home, reg, _, ts = wl.signature(x)
        w = np.array([O.profile(wl.wth, abs(t)) for t in ts] + [1.0])
        w = w / w.sum()
        return sum(wi * (self.var(r, x) * wi) for wi, r in zip(w, list(reg) + [home]))


def _fd_check(f, x, grad, eps_f, what):
    """the central-difference rule on f at x against grad [D]; returns the worst err / tol"""
    worst = 0.0
    for d in range(len(x)):
        e = np.zeros(len(x))
        e[d] = 1.0
        fd_h = (f(x + H * e) - f(x - H * e)) / (2 * H)
        fd_2h = (f(x + 2 * H * e) - f(x - 2 * H * e)) / (4 * H)
        tol = abs(fd_2h - fd_h) + 2 * eps_f / H
        err = abs(fd_h - float(grad[d]))
        worst = max(worst, err / tol)
        assert err <= tol, (what, d, err, tol)
    return worst


@pytest.mark.parametrize("trend", TRENDS)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_references_equal_central_differences_of_the_oracle(wl, family, trend):
    th = FAMILIES[family]
    fit = Fit(wl, th, trend)
    kept = wl.kept()
    assert len(kept) >= 48
    worst_item = worst_blend = 0.0
    for j in kept:
        x = wl.Xq[j]
        home, reg, planes, ts = wl.signature(x)
        regions = list(reg) + [home]
        out = [fit.ref[r].items(x[None, :]) for r in regions]
        eps = [(len(wl.Xs[r]) + 32) * U53 * float(o["vunit"][0]) for r, o in zip(regions, out)]
        assert not any(o["clamped"][0] for o in out)
        # the item of the home patch
        worst_item = max(worst_item, _fd_check(lambda p: fit.var(home, p), x, out[-1]["grad"][0], eps[-1], (family, trend, j)))
        assert item_close(VR.item_vgrad_ref(th, wl.Xs[home], SIGMA2, x, trend=trend), out[-1]["grad"][0])
        # the blend
        GV = np.stack([o["grad"][0] for o in out])
        v = np.array([o["v"][0] for o in out])
        dV, _ = VR.mix_vgrad_ref(range(len(regions)), GV, v, np.concatenate([ts, [0.0]]), np.array(list(planes) + [-1]),
                                 wl.hp_v, wl.wth)
        worst_blend = max(worst_blend, _fd_check(fit.blend, x, dV, max(eps), (family, trend, j, "blend")))
    print("VGRADREF family=%s trend=%s kept=%d worst err/tol item=%.3g blend=%.3g" % (family, trend, len(kept), worst_item, worst_blend))


def item_close(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def test_the_blend_of_the_pieces_is_the_oracles_query_mixture(wl):
    """what Fit.blend puts together under a trend is, without one, the oracle's own blend"""
    fit = Fit(wl, FAMILIES["spline34"], None)
    for j in wl.kept()[:16]:
        x = wl.Xq[j]
        home, reg, _, ts = wl.signature(x)
        w = np.array([O.profile(wl.wth, abs(t)) for t in ts] + [1.0])
        w = w / w.sum()
        mine = sum(wi * (fit.var(r, x) * wi) for wi, r in zip(w, list(reg) + [home]))
        assert abs(mine - fit.blend(x)) <= 8 * U53 * abs(mine)


def test_a_clamped_item_has_gradient_exactly_zero(wl):
    th = FAMILIES["spline34"]
    fit = Fit(wl, th, None)
    x = wl.Xq[wl.kept()[0]]
    home = wl.signature(x)[0]
    v = float(fit.ref[home].items(x[None, :])["v"][0])
    for min_v, clamped in ((2.0 * v, True), (0.5 * v, False)):
        out = fit.ref[home].items(x[None, :], min_v)
        assert bool(out["clamped"][0]) == clamped
        fd = [(fit.var(home, x + H * e, min_v) - fit.var(home, x - H * e, min_v)) / (2 * H) for e in np.eye(2)]
        if clamped:
            assert np.array_equal(out["grad"][0], np.zeros(2)) and fd == [0.0, 0.0] and float(out["v"][0]) == min_v
        else:
            assert np.all(out["grad"][0] != 0) and all(f != 0.0 for f in fd)
    # under a trend the clamp stops the simple-kriging part only
    tr = VR.PatchRef(th, wl.Xs[home], SIGMA2, "linear")
    free, held = tr.items(x[None, :]), tr.items(x[None, :], 2.0 * v)
    sk = fit.ref[home].items(x[None, :])["grad"][0]
    assert held["clamped"][0] and np.all(np.abs((free["grad"][0] - sk) - held["grad"][0]) <= 1e-17 * np.abs(free["grad"][0]).max())


# ------------------------------------------------------------------------------------------ the unit on the GPU tests' inputs
def _plain_item_grads(th, X, sigma2, Xq, trend, T_):
    """the item formula in the model's own precision T_ (float64 or float32) with numpy and LAPACK: what a careful
    implementation in that precision gives.  The trend's q x q algebra is in float64, as on the device."""
    X, Xq = X.astype(T_), Xq.astype(T_)
    n, D = X.shape
    dX = X[:, None, :] - X[None, :, :]
    U = (GR.phi(th, np.sqrt((dX * dX).sum(2))) + T_(sigma2) * np.eye(n, dtype=T_)).astype(T_)
    L = sla.cholesky(U, lower=True)
    assert L.dtype == T_
    diff = Xq[None, :, :] - X[:, None, :]
    tau = np.sqrt((diff * diff).sum(2))
    kq, g = GR.phi(th, tau), GR.psi(th, tau)[:, :, None] * diff
    VW = sla.solve_triangular(L, np.concatenate([kq[:, :, None], g], 2).reshape(n, -1), lower=True).reshape(n, len(Xq), 1 + D)
    grad = (-2.0 * (VW[:, :, :1] * VW[:, :, 1:]).sum(0)).astype(np.float64)
    if trend:
        Hm = T.basis(X, trend).astype(T_)
        C_H = sla.cho_solve((L, True), Hm)
        q = Hm.shape[1]
        LG = sla.cholesky(Hm.astype(np.float64).T @ C_H.astype(np.float64), lower=True)
        C_H = C_H.astype(np.float64)
        z = sla.solve_triangular(LG, (T.basis(Xq, trend) - (kq.T @ C_H.astype(T_)).astype(np.float64)).T, lower=True)      # q x m
        dh = np.zeros((D, q))
        if q > 1:
            dh[np.arange(D), 1 + np.arange(D)] = 1.0
        gC = np.einsum("nmd,nq->qmd", g, C_H.astype(T_)).astype(np.float64)
        y = sla.solve_triangular(LG, (dh.T[:, None, :] - gC).reshape(q, -1), lower=True).reshape(q, len(Xq), D)
        grad = grad + 2.0 * (z[:, :, None] * y).sum(0)
    return grad


def _gpu_item_cases():
    from test_gpu_vgrad import ITEM_CASES
    return ITEM_CASES


@pytest.mark.parametrize("D,family,dtype,trend", _gpu_item_cases())
def test_a_plain_evaluation_stays_below_one_unit_on_the_gpu_inputs(D, family, dtype, trend):
    from test_gpu_vgrad import COUNTS, ITEM_CASES, FAMILIES as GPU_FAMILIES
    case = ITEM_CASES.index((D, family, dtype, trend))
    oth = GPU_FAMILIES[family][1]
    T_, u = (np.float32, 2.0 ** -24) if dtype == "f32" else (np.float64, U53)
    Xs = VR.case_patches(100 + case, D, dtype)
    xq, region = VR.case_items(200 + case, Xs, list(np.roll(COUNTS, case)), dtype)
    worst = worst_trend = 0.0
    for r in sorted(set(int(x) for x in region)):
        n = len(Xs[r])
        if trend == "linear" and n < 1 + D:
            continue
        ref = VR.PatchRef(oth, Xs[r], VR.SIGMA2[dtype], trend)
        assert ref.kappa()[0] <= VR.KAPPA_MAX
        sel = region == r
        out = ref.items(xq[sel])
        plain = _plain_item_grads(oth, Xs[r], VR.SIGMA2[dtype], xq[sel], trend, T_)
        err = np.abs(plain - out["grad"]).astype(np.float64)
        unit = (n + 32) * u * out["unit"]
        assert np.all(err[unit == 0] == 0)
        worst = max(worst, float((err[unit > 0] / unit[unit > 0]).max()))
        if trend:
            # the trend's part alone, as the GPU test takes it: the difference to the same evaluation without the trend,
            # exact but for two double roundings of the whole gradient
            part = plain - _plain_item_grads(oth, Xs[r], VR.SIGMA2[dtype], xq[sel], None, T_)
            err = np.maximum(np.abs(part - out["trend"]).astype(np.float64) - 4 * U53 * np.abs(out["grad"]).astype(np.float64), 0.0)
            tunit = (n + 32) * u * out["tunit"]
            assert np.all(err[tunit == 0] == 0)
            worst_trend = max(worst_trend, float((err[tunit > 0] / tunit[tunit > 0]).max()))
    print("VGRADUNIT D=%d family=%s dtype=%s trend=%s plain worst err/unit=%.3g trend part=%.3g" % (D, family, dtype, trend, worst,
                                                                                                  worst_trend))
    assert worst < 1.0 and worst_trend < 1.0, (worst, worst_trend)


# ------------------------------------------------------------------------------------------ the ABI (fails without the feature)
def _header():
    return open(_lib.os.path.join(_lib._HERE, "..", "include", "pmk.h")).read()


def test_header_and_signatures_agree():
    protos = header_prototypes()
    L = pmk.lib()
    for name in NEW:
        assert name in protos, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
        res, args = _lib.SIGNATURES[name]
        cret, cargs = protos[name]
        assert [_cat(a) for a in args] == cargs, name
        assert _cat(res) == cret, name
    assert L.pmk_version() == 103
    assert '"items_vgrad", "mix_vgrad"' in _header()
    flat = re.sub(r"[\s*]+", " ", _header())
    assert "-2 V . W_d" in flat and "exactly 0 where the clamp holds" in flat


def test_stub_launchers_and_julia_ccalls():
    stubs = open(_lib.os.path.join(_lib.CSRC, "pmk_nogpu_stubs.cpp")).read()
    for name in ("launch_items_vgrad", "launch_trend_vgrad", "launch_mix_vgrad"):
        assert name in stubs, name
    protos = header_prototypes()
    seen = set()
    for name, ret, args, line in julia_ccalls():
        if name in NEW:
            assert (ret, args) == protos[name], (name, line)
            seen.add(name)
    assert seen >= set(NEW) - {"pmk_query_fetch_vgrad_dev"}, set(NEW) - seen


def test_argument_checks_need_no_device():
    L = pmk.lib()
    calls = {"pmk_query_items_vgrad": lambda: L.pmk_query_items_vgrad(None, None),
             "pmk_query_mix_vgrad": lambda: L.pmk_query_mix_vgrad(None, None, 0, 0),
             "pmk_query_fetch_vgrad": lambda: L.pmk_query_fetch_vgrad(None, None, 0),
             "pmk_query_fetch_vgrad_dev": lambda: L.pmk_query_fetch_vgrad_dev(None, None, 0),
             "pmk_query_get_items_vgrad": lambda: L.pmk_query_get_items_vgrad(None, None, 0),
             "pmk_predict_mixture_vgrad_fitted": lambda: L.pmk_predict_mixture_vgrad_fitted(None, None, 0, None, 0.0, 0.0, None, 0,
                                                                                            None, None, 0, None, 0)}
    assert sorted(calls) == sorted(NEW)
    for name, call in calls.items():
        assert call() == -1, name
        assert name.encode() in L.pmk_last_error(), name


def test_python_refuses_kernels_before_any_device_call(monkeypatch):
    DQ = M.DeviceQuery

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(M, "DeviceQuery", no_device)

    class Warped:
        warped = True

    class WithDiag:
        def diag_addend(self, X):
            return np.zeros(len(X))

    ok = pmk.Spline34KernelType(1.0)
    Xq = np.zeros((3, 2))
    for th in (Warped(), WithDiag()):
        with pytest.raises(TypeError, match="closure-carrying"):
            pmk.querymixtureGP_grad(Xq, _NoDevice([5, 7]), None, 2, 1.0, 1e-5, th, 1e-5, ok, variance=True)
    for bb in (pmk.BrownianBridge10(1.0), pmk.BrownianBridge2eps(1.0)):
        with pytest.raises(ValueError, match="Brownian-bridge"):
            pmk.querymixtureGP_grad(Xq, _NoDevice([5, 7]), None, 2, 1.0, 1e-5, bb, 1e-5, ok, variance=True)
        with pytest.raises(ValueError, match="Brownian-bridge"):
            pmk.querymixtureGP_grad(Xq, _NoDevice([5, 7]), None, 2, 1.0, 1e-5, ok, 1e-5, bb, variance=True)

    # the staged methods check their kernel before the library is asked
    class Handle:
        h, model, Nq = None, None, 0

        class L:
            def __getattr__(self, name):
                raise AssertionError("a library call was made: " + name)
        L = L()

    for th, exc in ((Warped(), TypeError), (pmk.BrownianBridge20(1.0), ValueError)):
        with pytest.raises(exc):
            DQ.items_vgrad(Handle(), th)
        with pytest.raises(exc):
            DQ.mix_vgrad(Handle(), th)


def test_docs_name_the_feature():
    root = _lib.os.path.join(_lib._HERE, "..")
    for doc, word in (("DESIGN.md", "pmk_vgrad.hip"), ("README.md", "variance=True"), ("INTEGRATION.md", "pmk_predict_mixture_vgrad_fitted")):
        assert word in open(_lib.os.path.join(root, doc), encoding="utf-8").read(), doc
