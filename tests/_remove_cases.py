"""Inputs of the removal tests (tests/test_remove_refs.py on the CPU, tests/test_gpu_remove.py on the GPU): host data only,
so that what the CPU file asserts of a case (kappa2(L) <= 10^3, the restatement within one unit of the oracle) holds of
the case the GPU file runs.

A case is a list of patches (n points, the rows that leave) of one model.  The sizes and rows are those at which the
deletion can go wrong: the first row (k0 = 0: everything is transformed), the last row (nothing is), rows on both sides of
a 32-row block and of a 128-row tile, rows spread over three tiles, as many rows as one call takes
(PMK_REMOVE_MAX_ROWS = 32, more than the 32 reflectors of a column block can be long), the last rows only, a patch of two
points that keeps one, a patch that loses nothing, and the slabs of SLAB_SIZES (full patches, runs of 32 rows, more than
512 rows below the first removed one).  The geometry (density, families, sigma2) is that of
tests/_append_cases.py.
"""
import numpy as np

import _append_cases as AC

SIGMA2, KAPPA_MAX, RATIO_MAX, FAMILIES = AC.SIGMA2, AC.KAPPA_MAX, AC.RATIO_MAX, AC.FAMILIES
rnd, target = AC.rnd, AC.target
MAX_ROWS = 32                   # PMK_REMOVE_MAX_ROWS

# 32 of the 300 rows, fixed: the first and the last row among them, and rows of every tile
_CAP_ROWS = sorted(set([0, 299] + [int(v) for v in np.random.default_rng(7).choice(np.arange(1, 299), 30, replace=False)]))

# (n, rows)
SMALL_SIZES = [(2, [0]), (2, [1]), (33, [0]), (33, [31]), (33, [32]), (130, [0]), (130, [127]), (130, [128])]
TILE_SIZES = [(130, [129]), (300, [5, 127, 128, 299]), (300, _CAP_ROWS), (384, [383]), (384, [380, 381, 382, 383]), (300, [])]
DIM_SIZES = [(33, [0]), (131, [127, 128]), (300, [5, 127, 128, 299]), (40, [])]
DIAG_SIZES = [(33, [31]), (131, [0, 128]), (300, [5, 127, 128, 299]), (64, [])]
SPLIT_SIZES = [(300, [5, 127, 128, 299]), (384, [383]), (130, [0])]
MIXED_SIZES = [(33, [0]), (130, [127]), (300, [5, 127, 128, 299]), (40, []), (2, [1])]
# eight patches (the leaves of a tree of 4 levels: multi-output items name their regions), every one keeps more points than
# a linear trend has basis functions, and every live 32-row pair is met: rows leave a first, a middle and a last pair
CONSUMER_SIZES = [(33, [0]), (33, [31]), (130, [0]), (130, [127]), (300, [5, 127, 128, 299]), (300, _CAP_ROWS),
                  (384, [380, 381, 382, 383]), (40, [])]
# slabs the sweep has to meet as well: a FULL patch (n = ld) that loses its first row, its last row (nothing is transformed)
# and both; one contiguous run of 32 rows, where s jumps from 0 to 32 at one row and every reflector has 33 entries from
# the first column on, inside a tile and astride the 128-row tile edge; t = n' - k0 > 512 rows below the first removed one
# (a third chunk of the row loop), with few rows and with as many as one call takes
_SPREAD_ROWS = sorted(set([0] + [int(v) for v in np.linspace(19, 599, 31).round()]))
SLAB_SIZES = [(128, [0]), (128, [127]), (256, [0, 255]), (256, list(range(96, 128))), (300, list(range(100, 132))),
              (640, [0, 255, 256, 511, 512, 639]), (600, _SPREAD_ROWS)]
MIXED_NAMES = ["spline34", "gaussian", "rq", "spline12", "rq"]
MIXED_SIGMA2 = AC.MIXED_SIGMA2


def removable(n):
    """the rows a patch of n points can lose and stay in its last block row"""
    return n - 128 * ((n + 127) // 128 - 1) - 1


class Case:
    """the patches of one model: Xs / ys (/ ds) the fitted points, targets (and addends), rows[r] the ascending rows that
    leave, keep[r] the rows that stay, Xr / yr (/ dr) the reduced lists"""

    def __init__(self, sizes, D, dtype, seed, addends=False):
        rng = np.random.default_rng(seed + 10 * D)
        self.sizes, self.D, self.dtype, self.P = sizes, D, dtype, len(sizes)
        self.Xs, self.ys, self.rows, self.keep = [], [], [], []
        for n, rows in sizes:
            half = 1.5 * max(1.0, n / 64.0) ** (1.0 / D)
            pts = rnd(rng.uniform(-half, half, (n, D)), dtype)
            self.Xs.append(np.ascontiguousarray(pts))
            self.ys.append(target(pts))
            self.rows.append(np.array(sorted(rows), dtype=np.int64))
            self.keep.append(np.setdiff1d(np.arange(n), rows))
        self.ds = [rnd(rng.uniform(0.0, 0.05, n), dtype) for n, _ in sizes] if addends else None
        self.Xr = [np.ascontiguousarray(x[k]) for x, k in zip(self.Xs, self.keep)]
        self.yr = [y[k] for y, k in zip(self.ys, self.keep)]
        self.dr = None if self.ds is None else [d[k] for d, k in zip(self.ds, self.keep)]


def all_cases(dtype):
    """(name, case, per-patch family names, per-patch sigma2) of every case of a precision"""
    s2 = SIGMA2[dtype]
    uni = lambda sizes, fam: (["%s" % fam] * len(sizes), [s2] * len(sizes))
    return [("small", Case(SMALL_SIZES, 2, dtype, 1900)) + uni(SMALL_SIZES, "spline34"),
            ("tiles", Case(TILE_SIZES, 2, dtype, 1910)) + uni(TILE_SIZES, "spline34"),
            ("tiles_gaussian", Case(TILE_SIZES, 2, dtype, 1910)) + uni(TILE_SIZES, "gaussian"),
            ("d1", Case(DIM_SIZES, 1, dtype, 1920)) + uni(DIM_SIZES, "spline34"),
            ("d4", Case(DIM_SIZES, 4, dtype, 1920)) + uni(DIM_SIZES, "rq"),
            ("addends", Case(DIAG_SIZES, 2, dtype, 1930, addends=True)) + uni(DIAG_SIZES, "spline34"),
            ("split", Case(SPLIT_SIZES, 2, dtype, 1940)) + uni(SPLIT_SIZES, "spline34"),
            ("consumers", Case(CONSUMER_SIZES, 2, dtype, 1960)) + uni(CONSUMER_SIZES, "spline34"),
            ("mixed", Case(MIXED_SIZES, 2, dtype, 1950), MIXED_NAMES, MIXED_SIGMA2[dtype]),
            ("slabs", Case(SLAB_SIZES, 2, dtype, 1970)) + uni(SLAB_SIZES, "spline34")]
