"""Inputs of the block-kriging tests (tests/test_block_refs.py on the CPU, tests/test_gpu_block.py on the GPU): host data
only, so that what the CPU file asserts of an input (kappa2(L) <= 10^3, a plain evaluation in the model's precision below
one error unit, every aggregate 100 units above its floor) holds of the input the GPU file runs.  The families and the bounds
are those of tests/_cov_cases.py, and so is sigma2 in fp64.

sigma2 in fp32 is 10, not the 0.05 of the covariance tests.  A unit is (n + 32) u kappa2(L) (k0 + |V| |V'|) per unit weight
and the variance of a block average inside the data is about k0 rho sigma2 / (sigma2 + lambda) (rho the mean correlation of
the members, lambda the eigenvalue of K along their mean): with sigma2 = 0.05 on patches of 272 to 298 points kappa2(L) is 23
to 29 and the variance 0.18 to 0.58 of ONE fp32 unit, so a rounding error could put an aggregate on its floor unseen.  With
sigma2 = 10 (noisy data, signal variance 1) kappa2(L) is 1.9 to 2.3 and the least margin, computed in long double, 154 units
(sigma2 = 1: 14 units).  The choice rests on the long-double reference alone.
"""
import numpy as np

import patchmixturekriging_amd as pmk
import _cov_cases as CC
import _cov_multi_cases as CMC

SIZES = (1, 2, 16, 31, 32, 33, 64, 65)                       # members of consecutive groups, repeated
SIGMA2 = {"f64": CC.SIGMA2["f64"], "f32": 10.0}
MARGIN_MIN = 100.0                                           # units between an aggregate's kappa - |Vbar|^2 and its floor
TREND_R = [(None, 1), ("constant", 3), ("linear", 13)]       # R = 1, 3 and 16 - q at D = 2


def cut(n, sizes=SIZES):
    """group [n] int32, non-decreasing from 0: consecutive groups of sizes[0], sizes[1], .. members, the last one cut"""
    g, k = [], 0
    while len(g) < n:
        g += [k] * sizes[k % len(sizes)]
        k += 1
    return np.array(g[:n], dtype=np.int32)


def averages(group, rng=None):
    """a [n]: 1 / (members of the group), the block average; with rng scaled by a factor in [0.5, 1.5] per query"""
    group = np.asarray(group)
    cnt = np.bincount(group)
    a = 1.0 / cnt[group]
    return a if rng is None else a * rng.uniform(0.5, 1.5, len(group))


class Main(CC.Main):
    """the four-leaf workload of tests/_cov_cases.py (patches of 272 to 298 points, 700 queries), its queries ordered by
    home leaf so that a group's members share their regions: the crowded leaf holds aggregates of 1 and of 65 members next
    to each other.  Groups of 1, 2, 16, 31-33 and 64-65 queries, coefficients of a perturbed block average."""

    def __init__(self, dtype="f64", seed=41):
        super().__init__(dtype, seed)
        off, reg, _ = CC.oracle_items(self)
        self.Xq = self.Xq[np.argsort(reg[off[1:] - 1], kind="stable")]
        self.group = cut(self.NQ)
        self.F = int(self.group[-1]) + 1
        self.a = averages(self.group, np.random.default_rng(seed + 1))

    def Ys(self, R):
        return [CMC.targets(x, R) for x in self.Xs]


# ---- strip and patch edges: the patches of tests/_cov_cases.py (1, 127, 128, 129, 300, 40, 200 and 90 points) under an
# 8-leaf tree; a blending radius so small that a query holds its home item alone, so the aggregates of region r are the
# groups of the queries in leaf r: 255, 1, 256, 257, 513, 0, 3 and 17 of them
EDGE_AGGS = CC.EDGE_COUNTS
EDGE_RADIUS, EDGE_DELTA = 1e-9, 1e-12
EDGE_SIZES = (1, 2, 3, 5)                                    # members of consecutive groups


def tree8(D):
    return pmk.setuppartition(np.random.default_rng(5).uniform(-4, 4, (64, D)), 4)[0]


def edge_queries(D, dtype, seed=900):
    """(Xq, group, a, home [Nq]): queries inside the leaves of tree8(D), ordered by leaf, near the patch of their leaf
    (points of the patch, perturbed, as CC.edge_items places the items of a small patch)"""
    rng = np.random.default_rng(seed + D)
    root = tree8(D)
    Xs = CC.edge_patches(D, dtype)
    pool = {r: [] for r in range(8)}
    need = {r: sum(EDGE_SIZES[k % len(EDGE_SIZES)] for k in range(c)) for r, c in enumerate(EDGE_AGGS)}
    for _ in range(400):
        x = CC.rnd(rng.uniform(-4, 4, (4096, D)), dtype)
        for p in x:
            r = pmk.findpartition(p, root)
            if len(pool[r]) < need[r]:
                pool[r].append(p)
        if all(len(pool[r]) >= need[r] for r in range(8)):
            break
    assert all(len(pool[r]) >= need[r] for r in range(8)), {r: (len(pool[r]), need[r]) for r in range(8)}
    Xq, group, home, g = [], [], [], 0
    for r, c in enumerate(EDGE_AGGS):
        pts, used = pool[r], 0
        for k in range(c):
            m = EDGE_SIZES[k % len(EDGE_SIZES)]
            Xq += pts[used:used + m]
            group += [g] * m
            home += [r] * m
            used += m
            g += 1
    Xq = np.array(Xq).reshape(-1, D)
    group = np.array(group, dtype=np.int32)
    return root, Xs, Xq, group, averages(group, rng), np.array(home)


def edge_items(home):
    """the item lists of a plan whose queries hold their home item alone"""
    n = len(home)
    return np.arange(n + 1, dtype=np.int64), np.asarray(home, dtype=np.int64), np.zeros(n)
