"""Inputs and references of the tests of what runs AFTER an append (tests/test_append_after_refs.py on the CPU,
tests/test_gpu_append_after.py on the GPU): host data and the oracle only.

  Oracle / MultiOracle   tests/_loo_blend_refs.Oracle and tests/_loo_blend_multi_refs.MultiOracle for an APPENDED model: the
                         tree is that of the points the model was built on (an append keeps it), the index lists are the
                         oracle's assignment of the extended array under that tree, sorted.  The new points carry the
                         global indices N, N + 1, ..., above every old one, so a sorted list is the old list followed by
                         the new entries in the order append_global gives them.
  tree_oracle            the oracle of tests/_append_cases.Tree, one per precision, with the points at which the CPU file
                         refits by brute force
  shapes / shape_call    a model that takes three calls of different shape (large, small, a changing set of receiving
                         patches), patches 0 to 2 ending exactly full
  trend_case / targets2  the patches of the trend test: SMALL_SIZES and a patch of two points that has fewer points than a
                         linear trend has basis functions before the append and more after it (and two patches more, for
                         a tree of eight leaves)
"""
import numpy as np

from oracle import oracle as O

import _append_cases as AC
import _loo_blend_refs as BR
import _loo_blend_multi_refs as MR

A = 1 / 3.0                                             # AC.FAMILIES["spline34"]


class _OriginalTree:
    def _tree(self, X, levels):
        return O.BSP(self._X0, levels)


class Oracle(_OriginalTree, BR.Oracle):
    """BR.Oracle of the extended points X under the tree of the first len(X0) of them"""

    def __init__(self, X0, X, y, eps, hyper, levels):
        assert np.array_equal(X[:len(X0)], X0)
        self._X0 = X0
        super().__init__(X, y, eps, hyper, levels)

    def blend_refit_noisy(self, wth, radius, points, delta=BR.DELTA):
        """blend_refit with the variances of the observation: every item's sigma2_r is added before the blend.  Item by
        item (queryinner and blend_items, the route blend_refit takes for per-patch hyperparameters): query_mixture
        returns the blended variance only"""
        home, regs, tss = self.plan(radius, delta)
        Y, V = np.empty(len(points)), np.empty(len(points))
        for k, j in enumerate(points):
            us, vs = [], []
            for r in [int(a) for a in regs[j]] + [int(home[j])]:
                if self.row_of(r, j) >= 0:
                    Xr, c, L = self.refit_without(r, j)
                else:
                    Xr, c, L = self.X[self.sets[r]], self.fits[r]["c_chol"], self.fits[r]["L"]
                u, v = O.queryinner(self.th[r], Xr, c, L, self.X[j], BR.MIN_V)
                us.append(u)
                vs.append(v + self.s2[r])
            Y[k], V[k] = BR.blend_items(wth, tss[j], us, vs)
        return Y, V


class MultiOracle(_OriginalTree, MR.MultiOracle):
    def __init__(self, X0, X, Y, eps, hyper, trend, levels):
        assert np.array_equal(X[:len(X0)], X0)
        self._X0 = X0
        super().__init__(X, Y, eps, hyper, trend, levels)


def hyper(dtype):
    return [(("s34", A), AC.SIGMA2[dtype])]


_TREE = {}


def tree_oracle(dtype):
    """(AC.Tree, Oracle of its extended array) of a precision, made once"""
    if dtype not in _TREE:
        t = AC.Tree(dtype)
        _TREE[dtype] = (t, Oracle(t.X, t.Xall, t.yall, t.EPS, hyper(dtype), t.LEVELS))
    return _TREE[dtype]


def multiplicity(o, first):
    """number of index lists that hold each of the points first .. N - 1"""
    return np.array([sum(o.row_of(r, j) >= 0 for r in range(o.P)) for j in range(first, len(o.X))])


def check_points(t):
    """the 18 new points and 18 old ones (every 22nd, so all four leaves are met)"""
    n0 = len(t.X)
    return list(range(n0, n0 + len(t.Xnew))) + list(range(3, n0, 22))[:18]


def targets2(X):
    """two target columns: AC.target and a field with an offset and a slope, which a trend has something to explain"""
    return np.stack([AC.target(X), 0.5 + 0.3 * X[:, 0] - 0.2 * X[:, -1] + 0.4 * np.cos(0.5 * X[:, -1])], 1)


# ---- calls of different shape on one model
SHAPE_N = (40, 200, 129, 513)
SHAPE_CALLS = [(60, 0, 100, 3), (1, 5, 0, 0), (27, 51, 27, 0)]
SHAPE_SIZES = [(n, sum(c[r] for c in SHAPE_CALLS)) for r, n in enumerate(SHAPE_N)]


def shapes(dtype):
    return AC.Case(SHAPE_SIZES, 2, dtype, 985)


def shape_call(case, k):
    """(Xn, yn) of call k: per patch the next SHAPE_CALLS[k][r] of its new points"""
    lo = [sum(c[r] for c in SHAPE_CALLS[:k]) for r in range(case.P)]
    hi = [a + SHAPE_CALLS[k][r] for r, a in enumerate(lo)]
    return ([np.ascontiguousarray(case.Xn[r][lo[r]:hi[r]]) for r in range(case.P)],
            [case.yn[r][lo[r]:hi[r]].copy() for r in range(case.P)])


def shape_sets(case, k):
    """(Xs, ys) after call k (k = -1: as fitted)"""
    hi = [sum(c[r] for c in SHAPE_CALLS[:k + 1]) for r in range(case.P)]
    return ([np.ascontiguousarray(np.vstack([case.Xs[r], case.Xn[r][:hi[r]]])) for r in range(case.P)],
            [np.concatenate([case.ys[r], case.yn[r][:hi[r]]]) for r in range(case.P)])


# ---- trend and multi-output state across an append
# the multi-output items need a model that holds every leaf of its tree, and a tree has 2^k leaves: two more patches (one
# that receives nothing) complete the eight
TREND_TWO = len(AC.SMALL_SIZES)                          # the patch of two points
TREND_SIZES = AC.SMALL_SIZES + [(2, 2), (17, 0), (45, 2)]


def trend_case(dtype="f64"):
    return AC.Case(TREND_SIZES, 2, dtype, 990)


def kappas(Xs, oth, s2):
    """kappa2(L) of every patch"""
    import _append_refs as AR
    return [AR.kappa_of(O.kernel_matrix(oth, X) + s2 * np.eye(len(X))) for X in Xs]
