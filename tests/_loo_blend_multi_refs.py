"""References of the multi-output blended leave-one-out tests (tests/test_loo_blend_multi_abi.py,
tests/test_gpu_loo_blend_multi.py): R target columns on the workload of tests/_loo_blend_refs.py, with or without a trend.

  targets         the R target columns: column 0 is the base workload's y, column 2 carries an offset and a slope (the
                  trend matters for it), the others are smooth fields
  MultiOracle     _loo_blend_refs.Oracle (tree, index lists, kernel matrices, plan) plus per-patch multi-output fits
  closed form     a member item is Y[i, :] - C[i, :] / Q_ii with variance 1 / Q_ii (- sigma2_r), Q_ii = d_i - |L_G^-1 C_H[i]|^2
                  (Q = d without a trend); a non-member item is the fitted predictor's.  fp64 scipy (_trend_refs.gls_fp64
                  and predict_fp64 with a trend).
  refits          BRUTE FORCE: the patch fitted again without the point, trend included, then the predictor at the point.
                  "fp64": scipy, for the CPU check of the identity.  "ref": the reference of the GPU tests, long double
                  (_trend_refs.trend_reference / predict_reference) with a trend, the oracle's Cholesky without one.  A
                  long-double refit of a 200-point patch takes 55 ms and the three cases need 1388 of them per trend, so
                  those of the members are RECORDED in tests/golden/loo_blend_multi_refits.npz (written by
                  tests/golden/make_loo_blend_multi.py from this module, rounded to double); an entry the file does not
                  hold is computed here.  The file serves the workload it was recorded from and no other
                  (MultiOracle.is_recorded_workload): its keys name eps and the trend only.

MultiOracle takes the tree depth as an argument (default: the base workload's) and the dimension from X.

Every item function returns, per point, (ts, U [k, R], v [k]) in reference order (neighbours in hyperplane order, the home
item last); blend() mixes them per column with _loo_blend_refs.blend_items.
"""
import os

import numpy as np
import scipy.linalg as sla

from oracle import oracle as O

import _loo_blend_refs as BR
import _trend_refs as TR

LD = np.longdouble
TRENDS = (None, "constant", "linear")
MIN_V = BR.MIN_V
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loo_blend_multi_refits.npz")
GOLDEN_R = 3


def targets(R=3):
    """X of the base workload and Y (N, R), column-major"""
    X, y = BR.workload()
    rng = np.random.default_rng(11)
    Y = np.empty((BR.N, R), order="F")
    for c in range(R):
        if c == 0:
            Y[:, c] = y
        elif c == 2:
            Y[:, c] = 2.0 + 0.4 * X[:, 0] - 0.25 * X[:, 1] + 0.5 * np.sin(0.6 * X[:, 0]) + 0.02 * rng.standard_normal(BR.N)
        else:
            Y[:, c] = (np.cos((0.3 + 0.1 * c) * X[:, 0] + 0.2 * c) * np.sin(0.4 * X[:, 1]) + 0.1 * c
                       + 0.02 * rng.standard_normal(BR.N))
    return X, Y


_GOLDEN_WORKLOAD = []


def _golden_workload():
    """(X, Y) the recorded refits were made from, generated once"""
    if not _GOLDEN_WORKLOAD:
        _GOLDEN_WORKLOAD.append(targets(GOLDEN_R))
    return _GOLDEN_WORKLOAD[0]


def basis(X, trend):
    X = np.atleast_2d(X)
    return np.zeros((X.shape[0], 0)) if trend is None else TR.basis(X, trend)


def fit_fp64(K, sigma2, Y, H):
    """_trend_refs.gls_fp64, and the same dict without a trend (H has no columns: Q = d, C = U^-1 Y)"""
    if H.shape[1] > 0:
        return TR.gls_fp64(K, sigma2, Y, H)
    n = K.shape[0]
    cf = sla.cho_factor(np.asarray(K, dtype=np.float64) + sigma2 * np.eye(n), lower=True)
    Cw = sla.cho_solve(cf, Y)
    Linv = sla.solve_triangular(cf[0], np.eye(n), lower=True)
    Q = (Linv * Linv).sum(0)
    return dict(C=Cw, Q=Q, L=np.tril(cf[0]), C_H=np.zeros((n, 0)), LG=np.zeros((0, 0)), beta=np.zeros((0, Y.shape[1])))


def predict_fp64(ref, Kq, kqq, Hq):
    if Hq.shape[1] > 0:
        return TR.predict_fp64(ref, Kq, kqq, Hq, MIN_V)
    Z = sla.solve_triangular(ref["L"], Kq.T, lower=True)
    return Kq @ ref["C"], np.maximum(np.asarray(kqq) - (Z * Z).sum(0), MIN_V)


class MultiOracle(BR.Oracle):
    """the oracle's view of one multi-output model: Y (N, R), trend None / "constant" / "linear", hyper as Oracle"""

    def __init__(self, X, Y, eps, hyper, trend, levels=BR.LEVELS):
        super().__init__(X, np.ascontiguousarray(Y[:, 0]), eps, hyper, levels)
        self.Y, self.trend, self.R = np.asarray(Y), trend, Y.shape[1]
        self._fit64, self._fitref, self._refit = {}, {}, {}
        self._golden = None

    # ---- per patch
    def kq(self, r, j):
        """(k(x_j, X_r) [1, n_r], k(x_j, x_j))"""
        Kq = O.cross_kernel_matrix(self.th[r], self.X[j:j + 1], self.X[self.sets[r]])
        return np.ascontiguousarray(Kq), O.kernel_eval(self.th[r], self.X[j], self.X[j])

    def fit64(self, r):
        if r not in self._fit64:
            s = self.sets[r]
            self._fit64[r] = fit_fp64(self.fits[r]["K"], self.s2[r], self.Y[s], basis(self.X[s], self.trend))
        return self._fit64[r]

    def member64(self, r, i, noisy):
        f = self.fit64(r)
        var = 1.0 / f["Q"][i]
        return self.Y[self.sets[r][i]] - f["C"][i] / f["Q"][i], (var if noisy else max(var - self.s2[r], MIN_V))

    def other64(self, r, j, noisy):
        Kq, kqq = self.kq(r, j)
        mu, v = predict_fp64(self.fit64(r), Kq, [kqq], basis(self.X[j], self.trend))
        return mu[0], float(v[0]) + (self.s2[r] if noisy else 0.0)

    def refit64(self, r, i, noisy):
        """patch r fitted without its row i in fp64 scipy, then the predictor at that point"""
        s, K = self.sets[r], self.fits[r]["K"]
        keep = np.arange(len(s)) != i
        H = basis(self.X[s], self.trend)
        ref = fit_fp64(K[np.ix_(keep, keep)], self.s2[r], self.Y[s][keep], H[keep])
        mu, v = predict_fp64(ref, K[i:i + 1, keep], [K[i, i]], H[i:i + 1])
        return mu[0], float(v[0]) + (self.s2[r] if noisy else 0.0)

    # ---- the reference of the GPU tests
    def _cols_from_L(self, L, Y):
        return sla.solve_triangular(L, sla.solve_triangular(L, Y, lower=True), lower=True, trans="T")

    def fitref(self, r):
        """the full fit of patch r: long double with a trend, the oracle's factor without"""
        if r not in self._fitref:
            s = self.sets[r]
            if self.trend is None:
                self._fitref[r] = dict(L=self.fits[r]["L"], C=self._cols_from_L(self.fits[r]["L"], self.Y[s]))
            else:
                self._fitref[r] = TR.trend_reference(self.fits[r]["K"], self.s2[r], self.Y[s], basis(self.X[s], self.trend))
        return self._fitref[r]

    def _predict_ref(self, ref, th, Xs, Kq, kqq, xq):
        """(mu [R], latent v) of one point from a fit of fitref's kind"""
        if self.trend is None:
            uv = [O.queryinner(th, Xs, np.ascontiguousarray(ref["C"][:, c]), ref["L"], xq, MIN_V) for c in range(self.R)]
            return np.array([a for a, _ in uv]), uv[0][1]
        mu, v = TR.predict_reference(ref, Kq, [kqq], basis(xq, self.trend), MIN_V)
        return np.asarray(mu[0], dtype=np.float64), float(v[0])

    def otherref(self, r, j, noisy):
        Kq, kqq = self.kq(r, j)
        mu, v = self._predict_ref(self.fitref(r), self.th[r], self.X[self.sets[r]], Kq, kqq, self.X[j])
        return mu, v + (self.s2[r] if noisy else 0.0)

    def golden_key(self):
        return "eps%g_%s" % (self.eps, self.trend)

    def is_recorded_workload(self):
        """the recorded refits belong to ONE workload: targets(GOLDEN_R) under a tree of BR.LEVELS levels, fitted with
        BR.A and BR.SIGMA2.  N, D, the levels, the hyperparameters and every bit of X and Y must be that workload's; any
        other one computes its refits (the (r, j) pairs alone do not tell two workloads apart)"""
        if not (self.uniform and self.R == GOLDEN_R and self.levels == BR.LEVELS and self.X.shape == (BR.N, BR.D)
                and self.hyper[0] == (("s34", BR.A), BR.SIGMA2)):
            return False
        Xg, Yg = _golden_workload()
        return bool(np.array_equal(self.X, Xg) and np.array_equal(self.Y, Yg))

    def _recorded(self):
        if self._golden is None:
            self._golden = {}
            if self.trend is not None and self.is_recorded_workload() and os.path.exists(GOLDEN):
                z, k = np.load(GOLDEN), self.golden_key()
                if k + "_rj" in z.files:
                    self._golden = {(int(a), int(b)): (z[k + "_mu"][n], float(z[k + "_v"][n]))
                                    for n, (a, b) in enumerate(z[k + "_rj"])}
        return self._golden

    def refitref_compute(self, r, j):
        """(mu [R], latent v): patch r fitted without global point j, then the predictor at x_j"""
        s = self.sets[r]
        i = self.row_of(r, j)
        keep = np.arange(len(s)) != i
        Xk = self.X[s][keep]
        K = self.fits[r]["K"]
        if self.trend is None:
            f = O.fit_patch(self.th[r], Xk, self.Y[s][keep][:, 0].copy(), self.s2[r])
            assert f["info"] == 0
            ref = dict(L=f["L"], C=self._cols_from_L(f["L"], self.Y[s][keep]))
        else:
            ref = TR.trend_reference(K[np.ix_(keep, keep)], self.s2[r], self.Y[s][keep], basis(Xk, self.trend))
        return self._predict_ref(ref, self.th[r], Xk, K[i:i + 1, keep], K[i, i], self.X[j])

    def refitref(self, r, j, noisy):
        if (r, j) not in self._refit:
            rec = self._recorded().get((r, j))
            self._refit[(r, j)] = rec if rec is not None else self.refitref_compute(r, j)
        mu, v = self._refit[(r, j)]
        return mu, v + (self.s2[r] if noisy else 0.0)

    # ---- items and blends
    def items(self, radius, kind, noisy=False, points=None):
        """kind "closed64": the closed form in fp64; "refit64": fp64 refits for the members; "ref": the GPU tests'
        reference.  -> {j: (ts, U [k, R], v [k], member [k])}"""
        home, regs, tss = self.plan(radius)
        out = {}
        for j in (range(len(self.X)) if points is None else points):
            us, vs, mem = [], [], []
            for r in [int(a) for a in regs[j]] + [int(home[j])]:
                i = self.row_of(r, j)
                if i < 0:
                    u, v = self.otherref(r, j, noisy) if kind == "ref" else self.other64(r, j, noisy)
                elif kind == "closed64":
                    u, v = self.member64(r, i, noisy)
                elif kind == "refit64":
                    u, v = self.refit64(r, i, noisy)
                else:
                    u, v = self.refitref(r, j, noisy)
                us.append(u)
                vs.append(v)
                mem.append(i >= 0)
            out[j] = (tss[j], np.array(us, dtype=np.float64), np.array(vs, dtype=np.float64), np.array(mem))
        return out

    def blend(self, wth, items):
        """-> (points, MU [len, R], V [len])"""
        pts = sorted(items)
        MU, V = np.empty((len(pts), self.R)), np.empty(len(pts))
        for k, j in enumerate(pts):
            ts, U, v, _ = items[j]
            for c in range(self.R):
                MU[k, c], V[k] = BR.blend_items(wth, ts, U[:, c], v)
        return pts, MU, V


def ratios(MU, V, MUref, Vref, cond, u, ymax, k0s2):
    """(max |dMU| / (cond u max|Y|), max |dV| / (cond u (k(0) + sigma2))): the solve's forward-error bound"""
    return (float(np.abs(MU - MUref).max() / (cond * u * ymax)), float(np.abs(V - Vref).max() / (cond * u * k0s2)))
