"""Workloads of the gradient edge tests (tests/test_grad_edges_refs.py on the CPU, tests/test_gpu_grad_edges.py on the GPU):
both files build their inputs here, once per process, so that the preconditions the CPU file asserts from the oracle
(neighbour items, plane indices, item counts, exact t, stable stencils) are those of the GPU file's inputs.

A workload is host data only: points uniform in [-box, box]^D (or given), a tree of `levels` levels, the eps-sets as
patches, the targets of tests/test_gpu_grad.py, queries uniform in [-qbox, qbox]^D (or given), and the oracle's tree.
workload("base2") and workload("base3") are the inputs of test_gpu_grad.Blend at D = 2 and 3 (the GPU file asserts the equality).
plan() is the oracle's plan of a query set: per query (home, regions, accepted pre-order planes, t of those planes).
"""
import numpy as np

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd.partition import hyperplane_arrays
from oracle import oracle as O

import _degenerate as DG
import _query_refs as QR
from test_gpu_grad import FAMILIES, _round, _targets

DELTA = 1e-5
PLAN_STAGE, PLAN_LDS_NODES = QR.PLAN_STAGE, QR.PLAN_LDS_NODES       # read from pmk_kernels.hip


class Workload:
    def __init__(self, name, D, R, levels, N=None, nq=160, box=4.0, qbox=None, radius=0.8, eps=0.3, seed=7, family="spline34",
                 trend=None, dtype="f64", X=None, queries_are_points=False):
        self.name, self.D, self.R, self.levels, self.radius, self.eps, self.delta = name, D, R, levels, radius, eps, DELTA
        self.box, self.width, self.family, self.trend, self.dtype = box, 2.0 * box, family, trend, dtype
        self.th, self.oth = FAMILIES[family]
        rng = np.random.default_rng(seed + D)
        if X is None:
            X = rng.uniform(-box, box, (N, D))
        self.X = _round(np.ascontiguousarray(X, dtype=np.float64), dtype)
        self.Xq = self.X.copy() if queries_are_points else rng.uniform(-(qbox or box), qbox or box, (nq, D))
        self._host = None
        self._plans = {}

    # ---- the tree, the patches, the oracle: built on first use
    def _built(self):
        if self._host is None:
            root, _, _ = pmk.setuppartition(self.X, self.levels)
            Xs, inds, _, _ = pmk.organizetrainingsets(root, self.levels, self.X, self.eps)
            hp_v, hp_c = hyperplane_arrays(root)
            self._host = dict(root=root, Xs=Xs, inds=inds, hp_v=hp_v, hp_c=hp_c, ob=O.BSP(self.X, self.levels))
        return self._host

    root = property(lambda self: self._built()["root"])
    Xs = property(lambda self: self._built()["Xs"])
    inds = property(lambda self: self._built()["inds"])
    hp_v = property(lambda self: self._built()["hp_v"])
    hp_c = property(lambda self: self._built()["hp_c"])
    ob = property(lambda self: self._built()["ob"])
    P = property(lambda self: 2 ** (self.levels - 1))

    def Ys(self, R=None):
        return [_targets(x, self.R if R is None else R) for x in self.Xs]

    def queries(self, n, seed=900):
        """n further queries in the base box (the ranges and blocks of group E)"""
        return np.random.default_rng(seed + n).uniform(-0.975 * self.box, 0.975 * self.box, (n, self.D))

    def signature(self, x, radius=None):
        ob = self.ob
        home = ob.findpartition(x)
        reg, ts, _, keep = ob.neighbours(x, self.radius if radius is None else radius, self.delta, home)
        return home, tuple(int(r) for r in reg), tuple(int(p) for p in np.nonzero(keep)[0]), ts[keep].copy()

    def plan(self, radius=None, Xq=None, key=None):
        """the oracle's plan; cached under (radius, key) when the queries are named by `key` (None: self.Xq)"""
        radius = self.radius if radius is None else radius
        k = (radius, key)
        if Xq is not None and key is None:
            return [self.signature(x, radius) for x in Xq]
        if k not in self._plans:
            self._plans[k] = [self.signature(x, radius) for x in (self.Xq if Xq is None else Xq)]
        return self._plans[k]

    def counts(self, radius=None):
        """neighbour items per query of self.Xq"""
        return np.array([len(s[1]) for s in self.plan(radius)])

    def stencil(self, x, h=None):
        h = self.width * 2.0 ** -17 if h is None else h
        return [x + s * h * np.eye(self.D)[d] for d in range(self.D) for s in (1, -1, 2, -2)]

    def stable_pick(self, pred, radius=None, n=16, n_pred=8, Xq=None, h=None):
        """(indices of n queries whose home, regions and planes are constant over the central-difference stencil of spacing h,
        how many of them satisfy pred(signature)): up to n_pred of the first kind first, as test_gpu_grad picks its 16"""
        key = ("pick", self.radius if radius is None else radius, pred.__name__, n, n_pred, h)
        if Xq is None and key in self._plans:
            return self._plans[key]
        Q = self.Xq if Xq is None else Xq
        kept, good = [], []
        for j, x in enumerate(Q):
            s0 = self.signature(x, radius)[:3]
            if all(self.signature(p, radius)[:3] == s0 for p in self.stencil(x, h)):
                kept.append(j)
                if pred(s0):
                    good.append(j)
            if len(good) >= n_pred and len(kept) >= n + n_pred:
                break
        first = good[:n_pred]
        pick = (first + [j for j in kept if j not in first])[:n]
        out = (pick, len([j for j in pick if j in good]))
        if Xq is None:
            self._plans[key] = out
        return out


def has_neighbours(sig):
    return len(sig[1]) > 0


def has_deep_plane(sig):
    return any(p >= 32 for p in sig[2])


# ------------------------------------------------------------------------------------ A. weight families
A_RADIUS = {2: 1.2, 3: 1.5}


def weight_kernels(r):
    """name -> (device kernel, oracle kernel) of the seven blending profiles of group A at plan radius r"""
    return {
        "spline12": (pmk.Spline12KernelType(1 / r), O.kernel(O.SPLINE12, 1 / r)),
        "spline32": (pmk.Spline32KernelType(1 / r), O.kernel(O.SPLINE32, 1 / r)),
        "gaussian": (pmk.GaussianKernel1DType(4 / r ** 2), O.kernel(O.GAUSSIAN, 4 / r ** 2)),
        "rq": (pmk.RationalQuadraticKernelType(r ** 2 / 4), O.kernel(O.RQ, r ** 2 / 4)),
        "trq": (pmk.TunableRationalQuadraticKernelType(r ** 2 / 4, 0.7), O.kernel(O.TRQ, r ** 2 / 4, 0.7)),
        "modsqexp": (pmk.ModulatedSqExpKernelType(4 / r ** 2, 1 / r), O.kernel(O.MODSQEXP, 4 / r ** 2, 1 / r)),
        "spline34_narrow": (pmk.Spline34KernelType(2 / r), O.kernel(O.SPLINE34, 2 / r)),
    }


def spline34_weight(r):
    return pmk.Spline34KernelType(1 / r), O.kernel(O.SPLINE34, 1 / r)


# ------------------------------------------------------------------------------------ B. larger trees
# name -> (D, levels, points per leaf); radius scaled by 1 / sqrt(P) as _deep_case of tests/test_gpu_query_edges.py.
# DEEP_FITTED: the cases that also fit a model, and its trend; the others are plan-only
DEEP = {"L7": (2, 7, 24), "L7_D4": (4, 7, 24), "L10": (2, 10, 8), "L12": (2, 12, 4), "L13": (2, 13, 4)}
DEEP_FITTED = {"L7": "linear", "L7_D4": None, "L10": None}


def _deep(name):
    D, levels, per_leaf = DEEP[name]
    P = 2 ** (levels - 1)
    radius = 0.6 / np.sqrt(P) if D == 2 else 0.25
    return Workload(name, D, 2, levels, N=per_leaf * P, nq=300, box=1.0, radius=radius, eps=0.5 * radius, seed=400 + levels,
                    trend=DEEP_FITTED.get(name))


# ------------------------------------------------------------------------------------ C. many neighbours
C_RADII = {"mid": 0.8, "wide": 10.0}          # wide: larger than the box, most leaves are neighbours


def _many():
    """D = 3, 64 leaves of 20 points.  On scattered points a neighbour is accepted only at an ancestor plane of the home
    leaf, at most levels - 1 = 6 of them: the depth is what lets a query exceed PLAN_STAGE (tests/test_grad_edges_refs.py);
    the polygon workload below has the queries of 12 and more items"""
    return Workload("many", 3, 2, 7, N=1280, nq=600, box=2.0, radius=C_RADII["mid"], eps=0.3, seed=520)


def reorderings(wl):
    """two orders of wl.Xq under the mid radius: A puts the queries with more than PLAN_STAGE neighbours first (block 0
    re-walks the planes), B puts them last behind at least 256 others (block 0 copies its staged hits)"""
    cnt = wl.counts()
    heavy, light = np.nonzero(cnt > PLAN_STAGE)[0], np.nonzero(cnt <= PLAN_STAGE)[0]
    return np.concatenate([heavy, light]), np.concatenate([light, heavy]), heavy, light


def polygon_points(levels=12, per_leaf=4, spread=0.01, seed=1):
    """A point set whose tree puts a polygon of levels - 1 ancestor planes round the origin, so that a query there is
    accepted at every one of them.  The tree takes a node's normal from (first point - mean) and cuts at the midpoint of
    the two middle projections.  From the home leaf upwards, node k is [pilot p_k, cluster A_k at n_k = (cos, sin)(2 pi k /
    K), node k + 1]: A_k and p_k are one half of the node and are cut off, and p_k is placed so that p_k - mean is
    parallel to n_k.  The later clusters next to n_k project to cos(2 pi / K) on it, so every plane lies about 0.92 from
    the origin and contains the foot of the origin inside its own side of the polygon; one point of the home leaf stands
    guard at cos(2 pi / K) n_{K-1} for the last plane, which has no later cluster.  tests/test_grad_edges_refs.py asserts
    the outcome from the oracle"""
    K = levels - 1
    rng = np.random.default_rng(seed)
    normal = lambda k: np.array([np.cos(2 * np.pi * k / K), np.sin(2 * np.pi * k / K)])
    S = spread * rng.uniform(-1, 1, (per_leaf, 2))
    S[0] += np.cos(2 * np.pi / K) * normal(K - 1)
    for k in range(K - 1, -1, -1):
        M, n = len(S), normal(k)
        A = n + spread * rng.uniform(-1, 1, (M - 1, 2))
        T = (S.sum(0) + A.sum(0)) / (2 * M)
        p = ((1.0 - T @ n) * n + T) / (1 - 1 / (2 * M))
        S = np.vstack([p[None, :], A, S])
    return np.ascontiguousarray(S)


POLYGON = dict(levels=12, spread=0.01, radius=10.0, nq=48)


def _polygon():
    """2048 leaves of 4 points (eps = 0: the leaves are the patches), 48 queries next to the origin, a radius wider than
    the box: 12 items and more per query"""
    c = POLYGON
    wl = Workload("polygon", 2, 2, c["levels"], box=1.0 + c["spread"], radius=c["radius"], eps=0.0,
                  X=polygon_points(c["levels"], 4, c["spread"]))
    wl.Xq = 0.5 * c["spread"] * np.random.default_rng(5).uniform(-1, 1, (c["nq"], 2))
    return wl


# ------------------------------------------------------------------------------------ D. exact t
def _on_plane():
    """D = 1, two leaves, 101 points: the plane passes through the median point; query 0 sits on it"""
    wl = Workload("on_plane", 1, 2, 2, N=101, nq=7, box=4.0, radius=0.8, eps=0.3, seed=610)
    v, c = wl.hp_v[0, 0], wl.hp_c[0]
    x0 = np.array([c / v])
    wl.Xq = np.vstack([x0[None, :], wl.Xq])
    return wl


def _grid():
    """a 32 x 32 lattice of spacing 1/4, whose diagonal root plane passes through lattice points; every second training
    point is a query"""
    wl = Workload("grid", 2, 2, 4, box=4.0, radius=0.6, eps=0.3, trend="linear", X=DG.lattice(32, 32), queries_are_points=True)
    wl.Xq = wl.X[::2].copy()
    return wl


def _dups():
    """241 points, 20 of them twins of others; an odd count at a node puts its plane through the median point, and every
    such point of a first tree is then written twice more into the set: triplets ON the planes of the final tree"""
    X = np.random.default_rng(631).uniform(-3, 3, (241, 2))
    X[120:140] = X[:20]
    first = Workload("dups0", 2, 2, 4, box=3.0, radius=0.6, eps=0.3, trend="linear", X=X, queries_are_points=True)
    on = [i for i, s in enumerate(first.plan()) if len(s[3]) and np.abs(s[3]).min() < 1e-12]
    X = X.copy()
    for k, i in enumerate(on):
        X[140 + 2 * k] = X[141 + 2 * k] = X[i]
    return Workload("dups", 2, 2, 4, box=3.0, radius=0.6, eps=0.3, trend="linear", X=X, queries_are_points=True)


HUGE_RADII = [1e150, 1e300]

# ------------------------------------------------------------------------------------ E, F, G
E_NQ = [1, 255, 256, 257, 513]
E_CUTS = [0, 100, 257, 513]


def range_chain(nq):
    """ranges that tile [0, nq) at non-multiples of 256"""
    cuts = sorted({min(c, nq) for c in E_CUTS})
    return list(zip(cuts[:-1], cuts[1:]))


F_RADII = {"small": 0.05, "large": 3.0}
MIXED_NAMES = ["spline34", "gaussian", "rq", "spline12", "trq", "spline32", "spline34", "rq"]
MIXED_SIGMA2 = {"f64": [1e-2 * (1 + 0.25 * r) for r in range(8)], "f32": [0.05 * (1 + 0.25 * r) for r in range(8)]}

_MAKERS = {
    "base2": lambda: Workload("base2", 2, 2, 4, N=480, nq=160, box=4.0, qbox=3.9, radius=A_RADIUS[2]),
    "base3": lambda: Workload("base3", 3, 2, 4, N=480, nq=160, box=4.0, qbox=3.9, radius=A_RADIUS[3]),
    "base2_f32": lambda: Workload("base2_f32", 2, 2, 4, N=480, nq=160, box=4.0, qbox=3.9, radius=A_RADIUS[2], dtype="f32"),
    "many": _many, "polygon": _polygon, "on_plane": _on_plane, "grid": _grid, "dups": _dups,
}
_MAKERS.update({name: (lambda name=name: _deep(name)) for name in DEEP})
_CACHE = {}


def workload(name):
    if name not in _CACHE:
        _CACHE[name] = _MAKERS[name]()
    return _CACHE[name]
