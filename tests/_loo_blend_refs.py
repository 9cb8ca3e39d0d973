"""References of the blended leave-one-out tests (tests/test_loo_blend_abi.py, tests/test_gpu_loo_blend.py), all on the
CPU with the oracle.

  Workload        the base workload of both files and its three (eps, radius) cases
  Oracle          tree, index lists, per-patch fits and the plan (home, neighbours, t) of the training points
  blend_refit     BRUTE FORCE: for point j every patch that holds j is refitted without it, then the mixture is queried at
                  x_j.  With one theta for every patch that query is the oracle's query_mixture; with per-patch
                  hyperparameters (which query_mixture does not take) it is the oracle's queryinner per item and the blend
                  of mixtureGP.jl:224-272 written out here (blend_items; checked against query_mixture in the CPU tests).
  blend_closed    the identity under test, in double: a member item is y_i - c_i / d_i with variance 1 / d_i (- sigma2_r), a
                  non-member item the oracle's queryinner; no refit.

Refits depend on (index lists, point, patch) only, not on the radius: they are cached per Oracle object, so the cases
that share eps share them.
"""
import numpy as np
import scipy.linalg as sla

from oracle import oracle as O

N, D, LEVELS = 620, 2, 3
A, SIGMA2, DELTA = 0.5, 1e-3, 1e-5
CASES = [(0.3, 0.25), (0.3, 0.6), (0.0, 0.4)]           # (eps, radius)
MIN_V = 1e-12

FAMILY = {"s34": O.SPLINE34, "rq": O.RQ}


def workload():
    """620 uniform points in [-4, 4]^2 and smooth targets plus noise of 0.02"""
    rng = np.random.default_rng(5)
    X = rng.uniform(-4, 4, (N, D))
    y = np.sin(0.7 * X[:, 0]) * np.cos(0.3 * X[:, -1]) + 0.05 * X[:, 0] + 0.02 * rng.standard_normal(N)
    return X, y


def okernel(h):
    """("s34" | "rq", a) -> oracle kernel"""
    return O.kernel(FAMILY[h[0]], float(h[1]))


def blend_items(wth, ts, us, vs):
    """mixtureGP.jl:224-272: neighbour weights phi_w(|t|) in hyperplane order, the home weight 1 last, normalised;
    Y = sum w u, V = sum w (v w)"""
    wt = np.array([O.profile(wth, abs(float(t))) for t in ts] + [1.0])
    w = wt / wt.sum()
    us, vs = np.asarray(us), np.asarray(vs)
    return float(np.sum(w * us)), float(np.sum(w * (vs * w)))


class Oracle:
    """the oracle's view of one model: tree of X, index lists for eps (None: the tree's leaves), fits with hyper[r] =
    ((family, a), sigma2) per patch.  The tree has `levels` levels (2^(levels - 1) leaves); the dimension is X's"""

    def __init__(self, X, y, eps, hyper, levels=LEVELS):
        self.X, self.y, self.eps, self.levels = X, y, eps, levels
        self.D = X.shape[1]
        self.bsp = self._tree(X, levels)
        self.P = self.bsp.P
        if eps is None:
            off, inds = self.bsp.leaves()
        else:
            off, inds, _, _ = self.bsp.assign(X, eps)
        self.sets = [np.sort(inds[off[r]:off[r + 1]]) for r in range(self.P)]
        if len(hyper) == 1:
            hyper = list(hyper) * self.P
        self.hyper = hyper
        self.uniform = all(h == hyper[0] for h in hyper)
        self.th = [okernel(h[0]) for h in hyper]
        self.s2 = [float(h[1]) for h in hyper]
        self.fits = [O.fit_patch(self.th[r], X[s], y[s], self.s2[r], want_K=True) for r, s in enumerate(self.sets)]
        assert all(f["info"] == 0 for f in self.fits)
        self._refits = {}
        self._plans = {}

    def _tree(self, X, levels):
        """the tree the index lists and the plan are made with: that of X (tests/_append_after_refs.py keeps the tree of
        the points a model was built on)"""
        return O.BSP(X, levels)

    def cond2(self):
        """cond_2 of U = K + sigma2 I, maximised over the patches"""
        worst = 0.0
        for f, s2 in zip(self.fits, self.s2):
            ev = np.linalg.eigvalsh(f["K"] + s2 * np.eye(len(f["K"])))
            worst = max(worst, float(ev[-1] / ev[0]))
        return worst

    def k0(self):
        """largest k(x, x) of the patches' kernels (1 for every stationary family used here)"""
        z = np.zeros(self.D)
        return max(O.kernel_eval(th, z, z) for th in self.th)

    def row_of(self, r, j):
        """row of global point j in patch r, or -1"""
        s = self.sets[r]
        i = int(np.searchsorted(s, j))
        return i if i < len(s) and s[i] == j else -1

    def plan(self, radius, delta=DELTA):
        """home [N], and per point its neighbour regions and t in hyperplane order (the home item comes last)"""
        key = (radius, delta)
        if key not in self._plans:
            f = self.fits
            _, _, home, off, reg, ts = O.query_mixture(self.bsp, self.th[0], self.th[0], [self.X[s] for s in self.sets],
                                                       [g["c_chol"] for g in f], [g["L"] for g in f], self.X, radius, delta,
                                                       debug=True)
            self._plans[key] = (home, [reg[off[j]:off[j + 1]] for j in range(len(self.X))],
                                [ts[off[j]:off[j + 1]] for j in range(len(self.X))])
        return self._plans[key]

    def counts(self, radius, delta=DELTA):
        """(items, non-member items, points with >= 2 neighbours, points whose home patch does not hold them)"""
        home, regs, _ = self.plan(radius, delta)
        total = strip = multi = homeless = 0
        for j in range(len(self.X)):
            items = list(regs[j]) + [home[j]]
            total += len(items)
            strip += sum(self.row_of(int(r), j) < 0 for r in items)
            multi += len(regs[j]) >= 2
            homeless += self.row_of(int(home[j]), j) < 0
        return total, strip, multi, homeless

    def refit_without(self, r, j):
        """patch r fitted without global point j (which it holds) -> (X, c, L)"""
        if (r, j) not in self._refits:
            s = self.sets[r]
            keep = s[s != j]
            assert len(keep) == len(s) - 1
            f = O.fit_patch(self.th[r], self.X[keep], self.y[keep], self.s2[r])
            assert f["info"] == 0
            self._refits[(r, j)] = (self.X[keep], f["c_chol"], f["L"])
        return self._refits[(r, j)]

    def blend_refit(self, wth, radius, points=None, delta=DELTA):
        """brute force -> (Y, V) at `points` (default: all): latent variances, clamped at 1e-12 per item as queryinner!"""
        points = range(len(self.X)) if points is None else points
        home, regs, tss = self.plan(radius, delta)
        Y, V = np.empty(len(points)), np.empty(len(points))
        for k, j in enumerate(points):
            Xs = [self.X[s] for s in self.sets]
            cs = [f["c_chol"] for f in self.fits]
            Ls = [f["L"] for f in self.fits]
            for r in range(self.P):
                if self.row_of(r, j) >= 0:
                    Xs[r], cs[r], Ls[r] = self.refit_without(r, j)
            if self.uniform:
                yq, vq = O.query_mixture(self.bsp, self.th[0], wth, Xs, cs, Ls, self.X[j:j + 1], radius, delta)
                Y[k], V[k] = yq[0], vq[0]
            else:
                uv = [O.queryinner(self.th[int(r)], Xs[int(r)], cs[int(r)], Ls[int(r)], self.X[j], MIN_V)
                      for r in list(regs[j]) + [home[j]]]
                Y[k], V[k] = blend_items(wth, tss[j], [a for a, _ in uv], [b for _, b in uv])
        return Y, V

    def loo_values(self):
        """per patch (mu_-i, 1 / d_i) in double from the oracle's factor: d = squared column norms of L^-1"""
        if not hasattr(self, "_loo"):
            self._loo = []
            for s, f in zip(self.sets, self.fits):
                Li = sla.solve_triangular(f["L"], np.eye(len(s)), lower=True)
                d = np.sum(Li * Li, axis=0)
                self._loo.append((self.y[s] - f["c_chol"] / d, 1.0 / d))
        return self._loo

    def items_closed(self, radius, noisy=False, delta=DELTA):
        """the closed form per item, in reference order (neighbours in hyperplane order, home last): lists per point of
        (region, member?, u, v)"""
        home, regs, _ = self.plan(radius, delta)
        loo = self.loo_values()
        out = []
        for j in range(len(self.X)):
            row = []
            for r in [int(v) for v in regs[j]] + [int(home[j])]:
                i = self.row_of(r, j)
                if i >= 0:
                    u, var = loo[r][0][i], loo[r][1][i]
                    v = var if noisy else max(var - self.s2[r], MIN_V)
                else:
                    f = self.fits[r]
                    u, v = O.queryinner(self.th[r], self.X[self.sets[r]], f["c_chol"], f["L"], self.X[j], MIN_V)
                    v = v + self.s2[r] if noisy else v
                row.append((r, i >= 0, float(u), float(v)))
            out.append(row)
        return out

    def blend_closed(self, wth, radius, noisy=False, delta=DELTA):
        """the closed form blended -> (Y, V) at every point"""
        _, _, tss = self.plan(radius, delta)
        items = self.items_closed(radius, noisy, delta)
        Y, V = np.empty(len(self.X)), np.empty(len(self.X))
        for j, row in enumerate(items):
            Y[j], V[j] = blend_items(wth, tss[j], [a[2] for a in row], [a[3] for a in row])
        return Y, V


def ratios(Y, V, Yref, Vref, cond, u, ymax, k0s2):
    """(max |dY| / (cond u max|y|), max |dV| / (cond u (k(0) + sigma2))): the solve's forward-error bound"""
    return (float(np.abs(Y - Yref).max() / (cond * u * ymax)), float(np.abs(V - Vref).max() / (cond * u * k0s2)))
