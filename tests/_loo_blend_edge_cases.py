"""Workloads of the blended leave-one-out edge tests (tests/test_loo_blend_edges_refs.py on the CPU,
tests/test_gpu_loo_blend_edges.py on the GPU): both files build their inputs and oracles here, so that the preconditions
the CPU test asserts (patch sizes, item counts, homeless points, the growth inequality) are those of the GPU test's inputs.

Every workload: points uniform in [-box, box]^D, targets smooth fields plus noise of 0.02 (the shapes of
_loo_blend_multi_refs.targets in any dimension), Spline34 a = 0.5, sigma2 = 1e-3, a tree of `levels` levels
(3 -> 4 leaves, 4 -> 8 leaves).  eps=None: the tree's own leaf lists.  Oracles are cached per process.
"""
import numpy as np

import _loo_blend_refs as BR
import _loo_blend_multi_refs as MR

UNIFORM = [(("s34", BR.A), BR.SIGMA2)]
Q_OF = {None: lambda D: 0, "constant": lambda D: 1, "linear": lambda D: 1 + D}


def points(seed, N, D, box):
    return np.random.default_rng(seed).uniform(-box, box, (N, D))


def fields(X, R, seed):
    """Y (N, R), column-major: column 0 the shape of the base workload's y, column 2 an offset and a slope in every
    coordinate (the trend matters for it), the others smooth fields; noise 0.02"""
    rng = np.random.default_rng(seed)
    N, D = X.shape
    x0, xl = X[:, 0], X[:, -1]
    slope = np.array([0.4, -0.25, 0.15, -0.1])[:D]
    Y = np.empty((N, R), order="F")
    for c in range(R):
        if c == 0:
            f = np.sin(0.7 * x0) * np.cos(0.3 * xl) + 0.05 * x0
        elif c == 2:
            f = 2.0 + X @ slope + 0.5 * np.sin(0.6 * x0)
        else:
            f = np.cos((0.3 + 0.1 * c) * x0 + 0.2 * c) * np.sin(0.4 * xl) + 0.1 * c
        Y[:, c] = f + 0.02 * rng.standard_normal(N)
    return Y


# ---- the dimensions: D = 1, 3, 4 (D = 2 is the base workload), and a deep tree at D = 3
DIMS = {
    "D1": dict(D=1, N=150, levels=4, box=4.0, eps=0.0, radius=0.4, seed=101, homeless=True),
    "D3": dict(D=3, N=200, levels=3, box=2.0, eps=0.3, radius=0.6, seed=103, homeless=False),
    "D3_deep": dict(D=3, N=200, levels=4, box=2.0, eps=0.0, radius=0.4, seed=103, homeless=False),
    "D4": dict(D=4, N=240, levels=3, box=2.0, eps=0.3, radius=0.6, seed=104, homeless=False),
}
DIM_MULTI = [(name, trend, 3) for name in DIMS for trend in MR.TRENDS] + \
            [("D4", "linear", 11), ("D4", "constant", 15)]         # R + q = 16 both times
DIM_FP32 = [("D1", "linear", 3), ("D3", "linear", 3), ("D4", "linear", 11)]

# ---- small patches: leaf lists under an 8-leaf tree, every patch has exactly N / 8 points
SMALL_PLAIN = [8, 16, 32]                                           # D = 2, no trend: patches of 1, 2, 4 points
SMALL_TREND = [(1, 24, "linear"), (2, 32, "linear"), (2, 16, "constant")]       # (D, N, trend): n = q + 1
AT_Q = [(2, 24, "linear"), (2, 8, "constant")]                      # n = q: no leave-one-out prediction exists
SMALL = dict(levels=4, box=2.0, radius=0.6, R=2)

# ---- item-count edges
COUNT_NS = [256, 257]
COUNT = dict(D=2, levels=3, box=4.0)

# ---- duplicated points
DUP = dict(D=2, N=200, levels=3, box=3.0, eps=0.3, radius=0.6, seed=131, pairs=10)

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def dim_inputs(name, R=3):
    c = DIMS[name]
    X = _cached(("dimX", name), lambda: points(c["seed"], c["N"], c["D"], c["box"]))
    return X, _cached(("dimY", name, R), lambda: fields(X, R, c["seed"] + 1000))


def dim_oracle(name, trend=None, R=3):
    """MultiOracle of a DIMS row; its single-output view (column 0) is the Oracle part of it"""
    c = DIMS[name]
    X, Y = dim_inputs(name, R)
    return _cached(("dimO", name, trend, R), lambda: MR.MultiOracle(X, Y, c["eps"], UNIFORM, trend, c["levels"]))


SMALL_SEEDS = {(2, 32): (11, 61)}          # D = 2, N = 32: a draw whose worst leave-one-out variance is about 25 k(0)


def small_inputs(D, N):
    sx, sy = SMALL_SEEDS.get((D, N), (200 + 10 * D + N, 300 + 10 * D + N))
    X = _cached(("smallX", D, N), lambda: points(sx, N, D, SMALL["box"]))
    return X, _cached(("smallY", D, N), lambda: fields(X, SMALL["R"], sy))


def small_oracle(D, N, trend):
    X, Y = small_inputs(D, N)
    return _cached(("smallO", D, N, trend), lambda: MR.MultiOracle(X, Y, None, UNIFORM, trend, SMALL["levels"]))


MIXED = dict(D=2, levels=4, eps=0.3, radius=0.6, trend="linear", R=2)


def mixed_inputs():
    """eight tight clusters of three points in [-3, 3]^2 under an 8-leaf tree: every leaf holds three points.  A leaf
    whose points all lie farther than eps from its planes keeps a list of three (n = q under the linear trend); a cluster
    cut by a plane, or closer to one than eps, puts its points into the list on the other side as well (n = 5 or more).
    The seed was picked so that no list has n = q + 1; the CPU test asserts the sizes from the oracle"""
    def make():
        rng = np.random.default_rng(48)
        centres = rng.uniform(-3, 3, (8, 2))
        X = np.vstack([c + rng.uniform(-0.04, 0.04, (3, 2)) for c in centres])
        return X, fields(X, MIXED["R"], 172)
    return _cached("mixed", make)


def mixed_oracle():
    X, Y = mixed_inputs()
    return _cached("mixedO", lambda: MR.MultiOracle(X, Y, MIXED["eps"], UNIFORM, MIXED["trend"], MIXED["levels"]))


def count_inputs(N):
    X = _cached(("countX", N), lambda: points(400 + N, N, COUNT["D"], COUNT["box"]))
    return X, _cached(("countY", N), lambda: fields(X, 3, 500 + N))


def count_oracle(N, trend=None):
    X, Y = count_inputs(N)
    return _cached(("countO", N, trend), lambda: MR.MultiOracle(X, Y, None, UNIFORM, trend, COUNT["levels"]))


def radius_with_no_neighbours(o):
    """a radius at which the oracle's plan has home items only: 0.05 halved until it is so.  A node that splits an odd
    number of points puts its plane THROUGH the median point (t == 0.0 exactly), and that point has a neighbour item at
    every positive radius: for such a data set (N = 257) the answer is the radius 0, which the plan takes (|t| < radius is
    never true)"""
    r = 0.05
    while o.counts(r)[0] != len(o.X):
        r = 0.5 * r if r > 1e-6 else 0.0
    return r


def radius_with_one_non_member(o, lo, hi=0.5):
    """bisection on the oracle's counts(radius): a radius with exactly one non-member item.  lo has none, hi has more
    than one; the count grows with the radius, one item at a time unless two points are equally far from a plane.  None
    if the count jumps over 1 (the N = 257 data set: its two median points, see above, come together at any radius > 0)"""
    assert o.counts(lo)[1] == 0 and o.counts(hi)[1] > 1
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        n = o.counts(mid)[1]
        if n == 1:
            return mid
        lo, hi = (mid, hi) if n == 0 else (lo, mid)
    return None


def dup_inputs():
    def make():
        c = DUP
        X = points(c["seed"], c["N"], c["D"], c["box"])
        h, k = c["N"] // 2, c["pairs"]
        X[h:h + k] = X[:k]                       # twins: the same coordinates under two global indices
        return X, fields(X, 3, c["seed"] + 1)
    return _cached("dup", make)


def dup_oracle(trend=None):
    X, Y = dup_inputs()
    return _cached(("dupO", trend), lambda: MR.MultiOracle(X, Y, DUP["eps"], UNIFORM, trend, DUP["levels"]))


# ---- buffer growth on the base workload's points and targets: a plan whose items fit the first reservation's slack never
# reallocates.  Under the base tree of 4 leaves no radius gets there: the largest plan has 1589 items, the reservation of
# the smallest (630) holds 630 + 78 + 1024 = 1732.  Under 16 leaves the plans go from 642 to 2186 items.
GROW = dict(eps=0.3, levels=5, small=0.01, large=20.0)


def grow_oracle(trend=None, R=3):
    X, Y = MR.targets(R)
    return _cached(("growO", trend, R), lambda: MR.MultiOracle(X, Y, GROW["eps"], UNIFORM, trend, GROW["levels"]))


def reserve_slack(total):
    """what the library's reservation for `total` items holds beyond them (total / 8 + 1024)"""
    return total // 8 + 1024
