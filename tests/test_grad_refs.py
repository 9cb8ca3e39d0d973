"""CPU-side checks of the gradient of the blended mean (no device compute).

1. tests/_grad_refs.py is pinned to the oracle: its analytic gradient of the blended multi-output predictor equals central
   differences of that predictor evaluated with the oracle's own pieces (findpartition, findneighbourpartitions, the cross
   kernel matrix and the weight profile of oracle/oracle.py), for every stationary family with and without a linear trend.
   D = 2, P = 4 leaves of about 40 points, R = 2, 64 random queries.  A query is kept if its home leaf and neighbour list
   agree at x, x +- h e_d and x +- 2h e_d (the gradient holds the item list fixed); at most a quarter may be dropped.
   Tolerance per component:  |FD_h - analytic| <= |FD_2h - FD_h| + 2 eps_f / h  with h = 2^-17 of the domain width.
   FD_2h - FD_h ~ 3 h^2 f''' / 6 is three times the estimated truncation of FD_h; eps_f = n 2^-53 sum |k c| is the rounding
   of one oracle evaluation (n products and sums per item; the blend is a convex combination of the items).
2. psi itself against central differences of the oracle's profile, every family.
3. The new symbols are in the header, the ctypes table, the library, the host-only stub launchers and the Julia ccalls;
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
import _grad_refs as GR
import _trend_refs as T

NEW = ["pmk_query_items_grad", "pmk_query_mix_grad", "pmk_query_fetch_grad", "pmk_query_fetch_grad_dev",
       "pmk_query_get_items_grad", "pmk_predict_mixture_grad_fitted"]

FAMILIES = {
    "spline34": O.kernel(O.SPLINE34, 1 / 3.0),
    "spline12": O.kernel(O.SPLINE12, 1 / 3.0),
    "spline32": O.kernel(O.SPLINE32, 1 / 3.0),
    "gaussian": O.kernel(O.GAUSSIAN, 0.5),
    "rq": O.kernel(O.RQ, 2.0),
    "trq": O.kernel(O.TRQ, 2.0, 0.7),
}
WIDTH = 8.0                         # the points are uniform in [-4, 4]^2
H = WIDTH * 2.0 ** -17
RADIUS, DELTA, SIGMA2, SEED = 1.0, 1e-5, 1e-2, 11
U53 = 2.0 ** -53


class Workload:
    """the tree, the leaves' points and targets, the 64 queries: built once"""

    def __init__(self):
        rng = np.random.default_rng(SEED)
        self.X = rng.uniform(-4, 4, (160, 2))
        self.ob = O.BSP(self.X, 3)
        assert self.ob.P == 4
        off, inds = self.ob.leaves()
        self.Xs = [self.X[inds[off[r]:off[r + 1]]] for r in range(4)]
        self.Ys = [np.stack([np.sin(0.7 * x[:, 0]) * np.cos(0.4 * x[:, 1]) + 0.3 * x[:, 0],
                             np.cos(0.5 * x[:, 0] + 0.2 * x[:, 1]) - 0.1 * x[:, 1] + 1.0], 1) for x in self.Xs]
        self.Xq = rng.uniform(-3.8, 3.8, (64, 2))
        self.hp_v, _ = self.ob.hyperplanes()
        self.wth = O.kernel(O.SPLINE34, 1 / RADIUS)

    def signature(self, x):
        home = self.ob.findpartition(x)
        reg, ts, _, keep = self.ob.neighbours(x, RADIUS, DELTA, home)
        return home, tuple(int(r) for r in reg), tuple(int(p) for p in np.nonzero(keep)[0]), ts[keep]

    def stencil(self, x):
        pts = []
        for d in range(2):
            e = np.zeros(2)
            e[d] = 1.0
            pts += [x + H * e, x - H * e, x + 2 * H * e, x - 2 * H * e]
        return pts

    def kept(self):
        """the queries whose home leaf and neighbour list agree on the whole stencil"""
        keep = []
        for j, x in enumerate(self.Xq):
            s0 = self.signature(x)[:3]
            if all(self.signature(p)[:3] == s0 for p in self.stencil(x)):
                keep.append(j)
        return keep


@pytest.fixture(scope="module")
def wl():
    return Workload()


def _fit(wl, th, trend):
    """per-patch weights (and beta under the linear trend) from a plain fp64 solve of the oracle's kernel matrix"""
    Cs, betas = [], []
    for X, Y in zip(wl.Xs, wl.Ys):
        K = O.kernel_matrix(th, X)
        if trend:
            f = T.gls_fp64(K, SIGMA2, Y, T.basis(X, "linear"))
            Cs.append(f["C"]); betas.append(f["beta"])
        else:
            Cs.append(sla.solve(K + SIGMA2 * np.eye(len(X)), Y, assume_a="pos")); betas.append(None)
    return Cs, betas


def _oracle_blend(wl, th, Cs, betas, x):
    """the blended multi-output predict at x from the oracle's pieces -> (Y [R], eps_f [R])"""
    home, reg, planes, ts = wl.signature(x)
    regions = list(reg) + [home]
    w = np.array([O.profile(wl.wth, abs(t)) for t in ts] + [1.0])
    S = w.sum()
    Y, mag = 0.0, 0.0
    for wi, r in zip(w, regions):
        kq = O.cross_kernel_matrix(th, x[None, :], wl.Xs[r])[0]
        u, a = kq @ Cs[r], np.abs(kq) @ np.abs(Cs[r])
        n = len(kq)
        if betas[r] is not None:
            h = np.concatenate([[1.0], x])
            u, a, n = u + h @ betas[r], a + np.abs(h) @ np.abs(betas[r]), n + len(h)
        Y = Y + (wi / S) * u
        mag = mag + (wi / S) * (n + len(regions) + 8) * a
    return Y, U53 * mag


def test_the_seed_keeps_three_quarters_of_the_queries(wl):
    kept = wl.kept()
    assert len(kept) >= 48, len(kept)
    # and the workload exercises the blend: some kept queries have neighbours
    assert sum(1 for j in kept if wl.signature(wl.Xq[j])[1]) >= 4


@pytest.mark.parametrize("trend", [False, True])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_analytic_gradient_equals_central_differences_of_the_oracle(wl, family, trend):
    th = FAMILIES[family]
    Cs, betas = _fit(wl, th, trend)
    kept = wl.kept()
    assert len(kept) >= 48
    worst = 0.0
    for j in kept:
        x = wl.Xq[j]
        home, reg, planes, ts = wl.signature(x)
        regions = list(reg) + [home]
        m = len(regions)
        # the restatement: per-item gradients and means in long double, then the blend
        G = np.stack([np.asarray(GR.item_grad_ref(th, wl.Xs[r], Cs[r], x, betas[r])).T for r in regions])     # m x R x D
        U = np.stack([np.asarray(O.cross_kernel_matrix(th, x[None, :], wl.Xs[r])[0], dtype=GR.LD) @ np.asarray(Cs[r], dtype=GR.LD)
                      + (0 if betas[r] is None else np.concatenate([[1.0], x]).astype(GR.LD) @ np.asarray(betas[r], dtype=GR.LD))
                      for r in regions])
        t = np.concatenate([ts, [0.0]])
        plane = np.array(list(planes) + [-1])
        dY, _ = GR.mix_grad_ref(range(m), G, U, t, plane, wl.hp_v, wl.wth)                                     # R x D
        for d in range(2):
            e = np.zeros(2)
            e[d] = 1.0
            (fp, ep), (fm, em) = _oracle_blend(wl, th, Cs, betas, x + H * e), _oracle_blend(wl, th, Cs, betas, x - H * e)
            (fp2, _), (fm2, _) = _oracle_blend(wl, th, Cs, betas, x + 2 * H * e), _oracle_blend(wl, th, Cs, betas, x - 2 * H * e)
            fd_h, fd_2h = (fp - fm) / (2 * H), (fp2 - fm2) / (4 * H)
            tol = np.abs(fd_2h - fd_h) + 2 * np.maximum(ep, em) / H
            err = np.abs(fd_h - np.asarray(dY[:, d], dtype=np.float64))
            worst = max(worst, float((err / tol).max()))
            assert np.all(err <= tol), (family, trend, j, d, err, tol)
    print("GRADREF family=%s trend=%s kept=%d worst err/tol=%.3g" % (family, trend, len(kept), worst))


@pytest.mark.parametrize("th", list(FAMILIES.values()) + [O.kernel(O.MODSQEXP, 0.5, 1.3)], ids=lambda k: "fam%d" % k.family)
def test_psi_is_the_derivative_of_the_oracle_profile_over_tau(th):
    h = 1e-6
    taus = np.linspace(0.05, 1.2 * min(GR.support(th), 6.0), 41)
    for tau in taus:
        fd = (O.profile(th, tau + h) - O.profile(th, tau - h)) / (2 * h)
        assert abs(fd - float(GR.psi(th, np.float64(tau))) * tau) <= 2e-9 * max(1.0, GR.lip(th)), (th.family, tau)
    assert abs(float(GR.phi(th, np.float64(0.7))) - O.profile(th, 0.7)) <= 1e-15
    assert np.isfinite(float(GR.psi(th, np.float64(0.0))))
    if th.family in GR.COMPACT:
        assert float(GR.psi(th, np.float64(1.0001 / th.p[0]))) == 0.0


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
    assert '"items_grad", "mix_grad"' in _header()
    flat = re.sub(r"[\s*]+", " ", _header())
    assert "ITEM LIST HELD FIXED" in flat


def test_stub_launchers_and_julia_ccalls():
    stubs = open(_lib.os.path.join(_lib.CSRC, "pmk_nogpu_stubs.cpp")).read()
    for name in ("launch_items_grad", "launch_mix_grad"):
        assert name in stubs, name
    protos = header_prototypes()
    seen = set()
    for name, ret, args, line in julia_ccalls():
        if name in NEW:
            assert (ret, args) == protos[name], (name, line)
            seen.add(name)
    assert seen >= set(NEW) - {"pmk_query_fetch_grad_dev"}, set(NEW) - seen


def test_argument_checks_need_no_device():
    L = pmk.lib()
    assert L.pmk_query_items_grad(None, None) == -1
    assert b"pmk_query_items_grad" in L.pmk_last_error()
    assert L.pmk_query_mix_grad(None, None, 0, 0) == -1
    assert L.pmk_query_fetch_grad(None, None, 0) == -1
    assert L.pmk_query_fetch_grad_dev(None, None, 0) == -1
    assert L.pmk_query_get_items_grad(None, None, 0, None) == -1
    assert L.pmk_predict_mixture_grad_fitted(None, None, 0, None, 0.0, 0.0, None, 0, None, 0) == -1


def test_python_refuses_kernels_before_any_device_call(monkeypatch):
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
            pmk.querymixtureGP_grad(Xq, _NoDevice([5, 7]), None, 2, 1.0, 1e-5, th, 1e-5, ok)
    for bb in (pmk.BrownianBridge10(1.0), pmk.BrownianBridge20(1.0), pmk.BrownianBridge1eps(1.0), pmk.BrownianBridge2eps(1.0)):
        with pytest.raises(ValueError, match="Brownian-bridge"):
            pmk.querymixtureGP_grad(Xq, _NoDevice([5, 7]), None, 2, 1.0, 1e-5, bb, 1e-5, ok)
        with pytest.raises(ValueError, match="Brownian-bridge"):
            pmk.querymixtureGP_grad(Xq, _NoDevice([5, 7]), None, 2, 1.0, 1e-5, ok, 1e-5, bb)


def test_docs_name_the_feature():
    root = _lib.os.path.join(_lib._HERE, "..")
    for doc, word in (("DESIGN.md", "pmk_grad.hip"), ("README.md", "querymixtureGP_grad"), ("INTEGRATION.md", "pmk_predict_mixture_grad_fitted")):
        assert word in open(_lib.os.path.join(root, doc), encoding="utf-8").read(), doc
