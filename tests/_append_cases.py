"""Inputs of the append tests (tests/test_append_refs.py on the CPU, tests/test_gpu_append.py on the GPU): host data only,
so that what the CPU file asserts of a case (kappa2(L') <= 10^3, the restatement within one unit of the oracle) holds of
the case the GPU file runs.

A case is a list of patches (n points, m appended) of one model.  The sizes are those at which the border can go wrong:
n + m on, just before and just after a 32-row block and a 128-row tile, a whole block, a whole tile's worth of rows, the
last block row holding 1, 2, 3 or 4 pairs of 32 rows (513, 672, 865 points: 5 to 7 block rows), a patch that receives
nothing and a full patch (n = 128) that can receive nothing.
"""
import numpy as np

import patchmixturekriging_amd as pmk
from oracle import oracle as O

SIGMA2 = {"f64": 1e-2, "f32": 0.05}
KAPPA_MAX = 1e3
RATIO_MAX = 10.0

FAMILIES = {
    "spline34": (pmk.Spline34KernelType(1 / 3.0), O.kernel(O.SPLINE34, 1 / 3.0)),
    "gaussian": (pmk.GaussianKernel1DType(2.0), O.kernel(O.GAUSSIAN, 2.0)),
    "rq": (pmk.RationalQuadraticKernelType(2.0), O.kernel(O.RQ, 2.0)),
    "spline12": (pmk.Spline12KernelType(1 / 3.0), O.kernel(O.SPLINE12, 1 / 3.0)),
}

# (n, m): n -> n + m
MAIN_SIZES = [(1, 1), (1, 127), (30, 5), (31, 1), (32, 1), (96, 32), (127, 1), (129, 127), (272, 26), (300, 1), (200, 0),
              (128, 0)]
TALL_SIZES = [(513, 7), (672, 1), (865, 31)]
SMALL_SIZES = [(30, 5), (127, 1), (129, 3), (40, 0), (300, 1)]
DIAG_SIZES = [(31, 1), (127, 1), (272, 26), (64, 0)]
SPLIT_SIZES = [(300, 1), (513, 7), (129, 127)]
MIXED_SIZES = [(30, 5), (96, 32), (129, 2), (40, 0), (127, 1)]
MIXED_NAMES = ["spline34", "gaussian", "rq", "spline12", "rq"]
MIXED_SIGMA2 = {"f64": [1e-2, 2e-2, 5e-2, 1e-2, 3e-2], "f32": [0.05, 0.08, 0.1, 0.05, 0.06]}
THREE_SIZES = [(30, 3), (125, 3), (300, 3)]
# the border kernel walks a column of width cw = the power of two >= max(m, 16): m on both sides of 16, 32 (MAIN_SIZES has
# m = 32) and 64, and cw = 64 (four row groups) on one, two, three and five block rows
WIDTH_SIZES = [(100, 16), (100, 17), (60, 33), (64, 64), (63, 65), (200, 56), (300, 48), (513, 40)]


def column_width(m):
    """cw of append_border_kernel for m new rows"""
    cw = 16
    while cw < m:
        cw *= 2
    return cw


def rnd(a, dtype):
    return a.astype(np.float32).astype(np.float64) if dtype == "f32" else a


def target(X):
    return np.sin(0.7 * X[:, 0]) * np.cos(0.4 * X[:, -1]) + 0.1 * X[:, 0]


class Case:
    """the patches of one model: Xs / ys the fitted points and targets, Xn / yn the appended ones (m_r x D, possibly
    empty), Xe / ye the extended lists; with addends: ds / dn / de.  The points are uniform in a box whose volume grows
    with the patch, so that the density, and with it kappa2, stays that of a small patch."""

    def __init__(self, sizes, D, dtype, seed, addends=False):
        rng = np.random.default_rng(seed + 10 * D)
        self.sizes, self.D, self.dtype = sizes, D, dtype
        self.Xs, self.ys, self.Xn, self.yn = [], [], [], []
        for n, m in sizes:
            half = 1.5 * max(1.0, (n + m) / 64.0) ** (1.0 / D)
            pts = rnd(rng.uniform(-half, half, (n + m, D)), dtype)
            self.Xs.append(np.ascontiguousarray(pts[:n]))
            self.Xn.append(np.ascontiguousarray(pts[n:]))
            self.ys.append(target(pts[:n]))
            self.yn.append(target(pts[n:]))
        self.Xe = [np.ascontiguousarray(np.vstack([a, b])) for a, b in zip(self.Xs, self.Xn)]
        self.ye = [np.concatenate([a, b]) for a, b in zip(self.ys, self.yn)]
        self.ds = self.dn = self.de = None
        if addends:
            self.ds = [rnd(rng.uniform(0.0, 0.05, n), dtype) for n, _ in sizes]
            self.dn = [rnd(rng.uniform(0.0, 0.05, m), dtype) for _, m in sizes]
            self.de = [np.concatenate([a, b]) for a, b in zip(self.ds, self.dn)]
        self.P = len(sizes)


def main(dtype, D=2):
    return Case(MAIN_SIZES, D, dtype, 900)


def tall(dtype):
    return Case(TALL_SIZES, 2, dtype, 910)


def small(D, dtype):
    return Case(SMALL_SIZES, D, dtype, 920)


def with_addends(dtype):
    return Case(DIAG_SIZES, 2, dtype, 930, addends=True)


def split(dtype):
    return Case(SPLIT_SIZES, 2, dtype, 940)


def mixed(dtype):
    return Case(MIXED_SIZES, 2, dtype, 950)


def three(dtype):
    return Case(THREE_SIZES, 2, dtype, 960)


def widths(dtype):
    return Case(WIDTH_SIZES, 2, dtype, 980)


def all_cases(dtype):
    """(name, case, per-patch family names, per-patch sigma2) of every case of a precision"""
    s2 = SIGMA2[dtype]
    out = [("main", main(dtype), ["spline34"] * len(MAIN_SIZES), [s2] * len(MAIN_SIZES)),
           ("main_gaussian", main(dtype), ["gaussian"] * len(MAIN_SIZES), [s2] * len(MAIN_SIZES)),
           ("tall", tall(dtype), ["spline34"] * len(TALL_SIZES), [s2] * len(TALL_SIZES)),
           ("d1", small(1, dtype), ["spline34"] * len(SMALL_SIZES), [s2] * len(SMALL_SIZES)),
           ("d4", small(4, dtype), ["rq"] * len(SMALL_SIZES), [s2] * len(SMALL_SIZES)),
           ("addends", with_addends(dtype), ["spline34"] * len(DIAG_SIZES), [s2] * len(DIAG_SIZES)),
           ("split", split(dtype), ["spline34"] * len(SPLIT_SIZES), [s2] * len(SPLIT_SIZES)),
           ("mixed", mixed(dtype), MIXED_NAMES, MIXED_SIGMA2[dtype]),
           ("three", three(dtype), ["spline34"] * len(THREE_SIZES), [s2] * len(THREE_SIZES)),
           ("widths", widths(dtype), ["spline34"] * len(WIDTH_SIZES), [s2] * len(WIDTH_SIZES))]
    return out


# ---- a tree with eps-sets for append_global: new points in one, two and more patches
class Tree:
    LEVELS, EPS, RADIUS, DELTA = 3, 0.3, 0.6, 1e-5

    def __init__(self, dtype="f64", seed=970):
        rng = np.random.default_rng(seed)
        self.dtype = dtype
        self.X = rnd(rng.uniform(-3, 3, (400, 2)), dtype)
        self.y = target(self.X)
        self.root, _, _ = pmk.setuppartition(self.X, self.LEVELS)
        hv, hc = pmk.partition.hyperplane_arrays(self.root)
        # new points: scattered ones, and points on the root's hyperplane and near where two hyperplanes meet
        on_root = hc[0] * hv[0] / (hv[0] @ hv[0]) + np.array([[-hv[0][1], hv[0][0]]]) * rng.uniform(-2, 2, (6, 1))
        # the root's hyperplane meets those of its two children at one point each: the nearer one is within eps of both
        meet = min((np.linalg.solve(np.stack([hv[0], hv[k]]), np.array([hc[0], hc[k]])) for k in (1, 2)),
                   key=lambda p: float(p @ p))
        self.Xnew = rnd(np.vstack([rng.uniform(-2.9, 2.9, (10, 2)), on_root + rng.uniform(-0.05, 0.05, (6, 2)),
                                   meet + rng.uniform(-0.02, 0.02, (2, 2))]), dtype)
        self.ynew = target(self.Xnew)
        self.Xall = np.ascontiguousarray(np.vstack([self.X, self.Xnew]))
        self.yall = np.concatenate([self.y, self.ynew])
        self.Xq = rnd(rng.uniform(-2.9, 2.9, (60, 2)), dtype)
        self.wth = pmk.Spline34KernelType(1 / self.RADIUS)
