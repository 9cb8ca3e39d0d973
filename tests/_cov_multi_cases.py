"""Inputs of the tests of the joint covariance on the multi-output path (tests/test_cov_multi_refs.py on the CPU,
tests/test_gpu_cov_multi.py on the GPU): host data only, so that what the CPU file asserts of an input (kappa2(L) <= 10^3,
a plain evaluation in the model's precision below one error unit) holds of the input the GPU file runs.  The settings per
precision (sigma2, the families, the bounds) are those of tests/_cov_cases.py.
"""
import numpy as np

import patchmixturekriging_amd as pmk
from oracle import oracle as O
import _cov_cases as CC

TRENDS = ("constant", "linear")
Q_OF = {None: lambda D: 0, "constant": lambda D: 1, "linear": lambda D: 1 + D}


def targets(X, R):
    """R smooth columns with a drift; the covariance does not depend on them"""
    X = np.asarray(X, dtype=np.float64)
    s = X.sum(1)
    return np.stack([np.sin(0.7 * X[:, 0] + 0.3 * c) * np.cos(0.4 * s) + 0.2 * (c + 1) * X[:, 0] + c for c in range(R)], 1)


class Main:
    """D = 2, four leaves with eps-sets of 130 to 180 points (two block rows), 420 queries of which 290 crowd the first
    leaf: that region holds more than 256 items (two strips, so pairs of different strips occur), the others fewer"""

    LEVELS, EPS, RADIUS, DELTA, NQ, CROWD = 3, 0.25, 0.6, 1e-5, 420, 290

    def __init__(self, dtype="f64", seed=47):
        rng = np.random.default_rng(seed)
        self.dtype = dtype
        self.X = CC.rnd(rng.uniform(-4, 4, (520, 2)), dtype)
        self.root, _, _ = pmk.setuppartition(self.X, self.LEVELS)
        self.Xs, self.inds, _, _ = pmk.organizetrainingsets(self.root, self.LEVELS, self.X, self.EPS)
        crowd = self.Xs[0][rng.integers(0, len(self.Xs[0]), self.CROWD)] + rng.uniform(-0.2, 0.2, (self.CROWD, 2))
        rest = rng.uniform(-3.9, 3.9, (self.NQ - self.CROWD, 2))
        self.Xq = CC.rnd(np.vstack([crowd, rest])[rng.permutation(self.NQ)], dtype)
        self.wth, self.owth = pmk.Spline34KernelType(1 / self.RADIUS), O.kernel(O.SPLINE34, 1 / self.RADIUS)

    def Ys(self, R):
        return [targets(x, R) for x in self.Xs]

    def oracle_items(self):
        return CC.oracle_items(self)


# ---- kernel edges through explicit items: eight regions of an 8-leaf tree.  (D, trend) gives q = 1, 2, 3 and 5 = TQ_MAX;
# R = 16 - q is the widest item row.  Patch 0 has n = q points (a finite block), patch 6 has q - 1 (flagged: n < q) for
# q >= 2; region 1 holds one item, region 3 holds 257 (two strips), region 5 none.
EDGE_TRENDS = [(2, "constant"), (1, "linear"), (2, "linear"), (4, "linear")]
EDGE_COUNTS = [5, 1, 256, 257, 300, 0, 3, 17]


def edge_sizes(q):
    return [q, 127, 128, 129, 260, 40, max(q - 1, 1), 90]


def edge_patches(D, trend, dtype, seed=800):
    rng = np.random.default_rng(seed + D)
    return [CC.rnd(rng.uniform(-2, 2, (n, D)), dtype) for n in edge_sizes(Q_OF[trend](D))]


def edge_items(Xs, dtype, seed=810):
    """(xq [m, D], region [m]) in a shuffled order (CC.edge_items with this file's counts)"""
    return CC.edge_items(Xs, EDGE_COUNTS, dtype, seed)


def flagged(D, trend):
    """the patches with fewer points than basis functions"""
    q = Q_OF[trend](D)
    return [r for r, n in enumerate(edge_sizes(q)) if n < q]
