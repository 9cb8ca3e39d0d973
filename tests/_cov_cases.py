"""Inputs of the joint-covariance tests (tests/test_cov_refs.py on the CPU, tests/test_gpu_cov.py on the GPU): host data
only, so that what the CPU file asserts of an input (kappa2(L) <= 10^3, a plain evaluation in the model's precision below
one error unit) holds of the input the GPU file runs.

A tree of `levels` has 2^(levels - 1) leaves in this package (setuppartition, oracle.BSP): the four leaves of the main
workload are levels = 3, the 512 leaves of the task-loop case levels = 10.
"""
import numpy as np

import patchmixturekriging_amd as pmk
from oracle import oracle as O

U_OF = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
SIGMA2 = {"f64": 1e-2, "f32": 0.05}
KAPPA_MAX = 1e3
RATIO_MAX = 10.0
TQ = 256                                                     # items of a strip

FAMILIES = {
    "spline34": (pmk.Spline34KernelType(1 / 3.0), O.kernel(O.SPLINE34, 1 / 3.0)),
    "gaussian": (pmk.GaussianKernel1DType(2.0), O.kernel(O.GAUSSIAN, 2.0)),
    "rq": (pmk.RationalQuadraticKernelType(2.0), O.kernel(O.RQ, 2.0)),
    "spline12": (pmk.Spline12KernelType(1 / 3.0), O.kernel(O.SPLINE12, 1 / 3.0)),
    "bb10": (pmk.BrownianBridge10(1.0), O.kernel(O.BB10, 1.0)),
}


def rnd(a, dtype):
    return a.astype(np.float32).astype(np.float64) if dtype == "f32" else a


class Main:
    """D = 2, four leaves with eps-sets of 260 to 300 points (three block rows, the last mostly padding), 700 queries of
    which 420 crowd the first leaf: one region holds more than 512 items (three strips), one fewer than 256"""

    LEVELS, EPS, RADIUS, DELTA, NQ = 3, 0.25, 0.6, 1e-5, 700

    def __init__(self, dtype="f64", seed=41):
        rng = np.random.default_rng(seed)
        self.dtype = dtype
        self.X = rnd(rng.uniform(-4, 4, (960, 2)), dtype)
        self.root, _, _ = pmk.setuppartition(self.X, self.LEVELS)
        self.Xs, self.inds, _, _ = pmk.organizetrainingsets(self.root, self.LEVELS, self.X, self.EPS)
        crowd = self.Xs[0][rng.integers(0, len(self.Xs[0]), 450)] + rng.uniform(-0.2, 0.2, (450, 2))
        self.Xq = rnd(np.vstack([crowd, rng.uniform(-3.9, 3.9, (self.NQ - 450, 2))])[rng.permutation(self.NQ)], dtype)
        self.y = np.sin(0.7 * self.X[:, 0]) * np.cos(0.4 * self.X[:, 1])
        self.wth, self.owth = pmk.Spline34KernelType(1 / self.RADIUS), O.kernel(O.SPLINE34, 1 / self.RADIUS)

    def oracle_items(self):
        return oracle_items(self)


def oracle_items(w):
    """(item_offsets, item_region, item_t) of the oracle's plan for a workload: per query its neighbours in hyperplane
    order, home last"""
    ob = O.BSP(w.X, w.LEVELS)
    off, reg, t = [0], [], []
    for x in w.Xq:
        home = ob.findpartition(x)
        r, ts, _, keep = ob.neighbours(x, w.RADIUS, w.DELTA, home)
        reg += [int(v) for v in r] + [int(home)]
        t += [float(v) for v in ts[keep]] + [0.0]
        off.append(len(reg))
    return np.array(off, dtype=np.int64), np.array(reg, dtype=np.int64), np.array(t)


def blocks_of(items, Xq):
    """per region with items: (query index of each row, ascending, a query that holds two items of the region twice;
    their points)"""
    off, reg = items[0], items[1]
    query_of = np.repeat(np.arange(len(off) - 1), np.diff(off))
    out = {}
    for r in sorted(set(int(v) for v in reg)):
        idx = np.sort(query_of[reg == r])
        out[r] = (idx, Xq[idx])
    return out


# ---- strip and patch edges through explicit items: eight regions of an 8-leaf tree
EDGE_SIZES = [1, 127, 128, 129, 300, 40, 200, 90]            # points per patch
EDGE_COUNTS = [255, 1, 256, 257, 513, 0, 3, 17]              # items per region
MIXED_NAMES = ["spline34", "gaussian", "rq", "spline12", "spline34", "rq", "gaussian", "spline12"]      # per-patch families


def edge_patches(D, dtype, seed=700):
    rng = np.random.default_rng(seed + D)
    return [rnd(rng.uniform(-2, 2, (n, D)), dtype) for n in EDGE_SIZES]


def edge_items(Xs, counts, dtype, seed=710):
    """(xq [m, D], region [m]) in a shuffled order; per region random points around the patch, one on a training point.
    A patch of fewer than 16 points has its queries within half a unit per coordinate of its points: near the edge of a
    compact support the error unit does not see the digits lost in t = 1 - r (tests/_vgrad_edge_cases.py)."""
    rng = np.random.default_rng(seed)
    D = Xs[0].shape[1]
    xq, region = [], []
    for r, cnt in enumerate(counts):
        if cnt == 0:
            continue
        if len(Xs[r]) < 16:
            pts = Xs[r][np.arange(cnt) % len(Xs[r])] + rng.uniform(-0.5, 0.5, (cnt, D))
        else:
            pts = rng.uniform(-2.5, 2.5, (cnt, D))
        pts[0] = Xs[r][len(Xs[r]) // 2]
        xq.append(pts)
        region += [r] * cnt
    perm = rng.permutation(len(region))
    return rnd(np.vstack(xq), dtype)[perm], np.array(region, dtype=np.int32)[perm]


# ---- Brownian bridge at D = 1: points and queries inside (0, 1)
def bb_patches(dtype="f64", seed=720):
    rng = np.random.default_rng(seed)
    return [rnd(np.sort(rng.uniform(0.02, 0.98, (n, 1)), 0), dtype) for n in (40, 129, 7, 64, 130, 20, 33, 90)]


def bb_items(dtype="f64", seed=721):
    rng = np.random.default_rng(seed)
    counts = [5, 17, 3, 9, 33, 0, 2, 6]
    region = np.repeat(np.arange(8, dtype=np.int32), counts)
    return rnd(rng.uniform(0.05, 0.95, (len(region), 1)), dtype), region


# ---- more tasks than workgroups: 512 leaves of about 20 points, one query per leaf centre.  Query 89 holds two items of
# region 88 (the neighbour search accepts that leaf through two hyperplanes): tests/test_cov_refs.py asserts it
class Many:
    LEVELS, EPS, RADIUS, DELTA = 10, 0.03, 0.25, 1e-5

    def __init__(self, seed=43):
        rng = np.random.default_rng(seed)
        self.X = rng.uniform(-4, 4, (8000, 2))
        self.root, _, _ = pmk.setuppartition(self.X, self.LEVELS)
        self.Xs, self.inds, _, _ = pmk.organizetrainingsets(self.root, self.LEVELS, self.X, self.EPS)
        self.Xq = np.array([x.mean(0) for x in self.Xs])
        self.y = np.sin(0.7 * self.X[:, 0]) * np.cos(0.4 * self.X[:, 1])
        self.wth, self.owth = pmk.Spline34KernelType(1 / self.RADIUS), O.kernel(O.SPLINE34, 1 / self.RADIUS)
