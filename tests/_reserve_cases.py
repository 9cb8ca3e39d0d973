"""Inputs of the reserve tests (tests/test_reserve_refs.py on the CPU, tests/test_gpu_reserve.py on the GPU): host data
only, so that what the CPU file asserts of a case (every extended set positive definite, kappa2(L') <= 10^3) holds of the
case the GPU file runs.  The points, targets and families are those of tests/_append_cases.py (Case: n fitted points and m
appended ones per patch, uniform in a box that grows with the patch).

STRIDE: patch sizes on both sides of one and two tiles with reserves of 0, 1, 128 and 200 rows mixed; the patch of 100
points with 0 rows and the one of 129 with 1 row keep their stride, the others get one, one and two more block rows.

CROSS: every way an append meets a 128-row boundary on a reserved model, one patch each, in one model of eight patches
(a tree of eight leaves can name them as regions):
    100 -> 128  fills the tile                      128 -> 129  enters a tile with one row
    120 -> 140  straddles the edge in one call      127 -> 255  128 rows over five 32-row diagonal blocks
      1 -> 129                                      250 -> 260  nt 2 -> 3
    200 -> 256  stays inside its block row and fills it (the arithmetic of an unreserved model)
     64 -> 64   receives nothing
REORDER: the smallest patch of four becomes the largest (60 -> 188), so max_nt goes 1 -> 2 and the factorisation order
changes; one patch grows inside its tile, two receive nothing.  ALONE: 127 -> 255 as the only patch (P = 1).
"""
import numpy as np

import _append_cases as AC

SIGMA2 = AC.SIGMA2
KAPPA_MAX = AC.KAPPA_MAX
RATIO_MAX = AC.RATIO_MAX

STRIDE_SIZES = [1, 100, 128, 129, 300]
STRIDE_RESERVE = [200, 0, 1, 1, 128]
STRIDE_RESERVE_MORE = [200, 30, 129, 1, 300]     # a second, larger reserve: 100 grows now, 129 still has the room
STRIDE_FAMILIES = {1: ["spline34"] * 5, 2: ["spline34", "gaussian", "rq", "spline12", "rq"], 4: ["rq"] * 5}
STRIDE_SIGMA2 = {"f64": [1e-2, 2e-2, 5e-2, 1e-2, 3e-2], "f32": [0.05, 0.08, 0.1, 0.05, 0.06]}

CROSS_SIZES = [(100, 28), (128, 1), (120, 20), (127, 128), (1, 128), (250, 10), (200, 56), (64, 0)]
REORDER_SIZES = [(60, 128), (100, 5), (128, 0), (90, 0)]
ALONE_SIZES = [(127, 128)]
RESERVE_ROWS = 130                                # what every patch of a crossing case is given


def ld_after(n, rows, ld=None):
    """the stride pmk_model_reserve leaves a patch of n points that had stride ld (None: 128 ceil(n / 128))"""
    ld = 128 * ((n + 127) // 128) if ld is None else ld
    return max(ld, 128 * ((n + rows + 127) // 128))


def stride(D, dtype):
    """the patches of the stride checks: a Case whose appended part is empty, with addends at D = 2"""
    return AC.Case([(n, 0) for n in STRIDE_SIZES], D, dtype, 1200, addends=(D == 2))


def crossing(name, dtype):
    sizes = {"cross": CROSS_SIZES, "reorder": REORDER_SIZES, "alone": ALONE_SIZES}[name]
    return AC.Case(sizes, 2, dtype, 1210 + len(sizes))


CROSSING_NAMES = ["cross", "reorder", "alone"]


def all_extended(dtype):
    """(name, points, addends or None, family, sigma2) of every patch whose factor a bound of the GPU file depends on"""
    out = []
    for D in (1, 2, 4):
        c = stride(D, dtype)
        for r in range(c.P):
            out.append(("stride-D%d-%d" % (D, r), c.Xe[r], None if c.de is None else c.de[r], STRIDE_FAMILIES[D][r],
                        STRIDE_SIGMA2[dtype][r]))
    for name in CROSSING_NAMES:
        c = crossing(name, dtype)
        for r in range(c.P):
            out.append(("%s-%d" % (name, r), c.Xe[r], None, "spline34", SIGMA2[dtype]))
    return out


def query_points(P, n, seed):
    """points for a planned query and a tree of P leaves (P a power of two) to name the patches as regions"""
    import patchmixturekriging_amd as pmk

    rng = np.random.default_rng(seed)
    root, _, _ = pmk.setuppartition(rng.uniform(-3, 3, (16 * P, 2)), int(np.log2(P)) + 1)     # levels count the root
    return root, np.ascontiguousarray(rng.uniform(-2.5, 2.5, (n, 2)))


class Tree8(AC.Tree):
    """the tree case of tests/_append_cases.py with one more level: eight leaves"""
    LEVELS = 4


class TreeCross(AC.Tree):
    """the tree case of tests/_append_cases.py (four eps-sets of 122 to 153 points; new points in one, two and more
    patches) with 90 more scattered new points: every patch receives 29 to 46 points in one call, the patches of 122 and
    123 points more than the 6 and 5 rows they have without a reserve, and both enter their second block row"""
    EXTRA = 90

    def __init__(self, dtype="f64"):
        super().__init__(dtype)
        rng = np.random.default_rng(1234)
        self.Xnew = np.ascontiguousarray(np.vstack([self.Xnew, AC.rnd(rng.uniform(-2.9, 2.9, (self.EXTRA, 2)), dtype)]))
        self.ynew = AC.target(self.Xnew)
        self.Xall = np.ascontiguousarray(np.vstack([self.X, self.Xnew]))
        self.yall = np.concatenate([self.y, self.ynew])
