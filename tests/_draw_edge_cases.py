"""Inputs of the edge tests of the block draws (tests/test_draw_edges_refs.py on the CPU, tests/test_gpu_draw_edges.py on the
GPU): host data only, so that what the CPU file asserts of an input holds of the input the GPU file runs.

The lattice.  22 x 18 nodes on [-3.8, 3.8]^2, every coordinate moved by up to 0.05, in a shuffled order: 396 queries spread
evenly over the four leaves of _cov_cases.Main (and of _cov_multi_cases.Main), so that every region block is several tiles
of 32 deep, well conditioned and free of repeated rows.  The crowd of Main.Xq is none of that.

The seams.  From the oracle's plan of the lattice at radius 0 (home items only) one query of the fullest region is given a
second time, at the query index that makes the copy's row in that region's block the first row of tile 2, the last row of
tile 2, or the last row of the block: the pivot of that row is the first the device's rule refuses.
"""
import numpy as np

import _cov_cases as CC
import _draw_refs as DR

NX, NY, SPAN, JITTER, SEED = 22, 18, 3.8, 0.05, 5
TILE = 32
SEAM_TILE = 2                                                # the tile of the second copy in the first two seam batches
SEAM_FIRST_ROW = 3                                           # the row of the first copy: inside the first tile
SEAMS = ("tile_first", "tile_last", "block_last")
Z_SEED, N_CHUNK_DRAWS = 21, 300                              # the draws whose bits must not depend on their chunk
SPLITS = (1, 31, 32, 33, 203)                                # 300 draws in separate calls
ALONE = (255, 256, 257)                                      # the rows on both sides of the first seam, each drawn alone
MAX_REL = 2.0 ** -26


def lattice_queries(dtype="f64"):
    rng = np.random.default_rng(SEED)
    gx, gy = np.meshgrid(np.linspace(-SPAN, SPAN, NX), np.linspace(-SPAN, SPAN, NY))      # rows of constant y
    X = np.stack([gx.ravel(), gy.ravel()], 1) + rng.uniform(-JITTER, JITTER, (NX * NY, 2))
    return np.ascontiguousarray(CC.rnd(X[rng.permutation(NX * NY)], dtype))


def lattice(m, radius=None):
    """what oracle_items needs: the workload m (a Main of _cov_cases.py or of _cov_multi_cases.py) with the lattice queries"""
    sub = DR.MainSub(m, lattice_queries(m.dtype))
    if radius is not None:
        sub.RADIUS = radius
    return sub


def seam_batches(m):
    """{name: dict(Xq, region, first, copy, row)} from the oracle's plan of the lattice at radius 0: query `first` (row
    SEAM_FIRST_ROW of the block of `region`) is given again at query index `copy`, which makes it row `row` (from 0) of that
    block in sorted-item order; the other regions hold the queries they held, in the same order"""
    sub = lattice(m, 0.0)
    off, reg, _ = CC.oracle_items(sub)
    assert np.all(np.diff(off) == 1)
    r_star = int(np.argmax(np.bincount(reg, minlength=4)))
    H = np.nonzero(reg == r_star)[0]
    first = int(H[SEAM_FIRST_ROW])
    rows = {"tile_first": TILE * SEAM_TILE, "tile_last": TILE * SEAM_TILE + TILE - 1, "block_last": len(H)}
    out = {}
    for name in SEAMS:
        row = rows[name]
        copy = int(H[row]) if row < len(H) else len(sub.Xq)
        Xq = np.ascontiguousarray(np.insert(sub.Xq, copy, sub.Xq[first], axis=0))
        out[name] = dict(Xq=Xq, region=r_star, first=first, copy=copy, row=row, rows_before=len(H))
    return out


def ladder_rungs():
    """the rel values of the jitter ladder as the front ends form them: 2^-52, then x 10 while the result is <= 2^-26"""
    rungs, rel = [], 2.0 ** -52
    while rel <= MAX_REL:
        rungs.append(rel)
        rel = 10.0 * rel
    return rungs
