"""A numpy restatement of the posterior draws from the region blocks (tests/test_draw_refs.py on the CPU,
tests/test_gpu_draw.py on the GPU), and the inputs the two files share.

With S_r = L_r L_r^T the long-double region blocks of tests/_cov_refs.py and W [Nq, total] the matrix that holds the
normalised weight wn_i of item i in row query(i) and in the column of the item's place in the sorted order (regions
ascending, a region's items in ascending query index, two items of one query in their item order),

    A = W blockdiag(L_r),      draw = Yq + A zeta,      A A^T = sum_r W_r S_r W_r^T = Cov,

the matrix of _cov_refs.mix_cov_ref, the cross term of a query with two items of one region included.

The error unit of a factor, entry (a, b) of L L^T - S:  (m + 8) 2^-53 sqrt(S_aa S_bb)  (Higham, Accuracy and Stability,
Thm 10.3: |L L^T - S| <= gamma_{m+1} |L| |L|^T, and (|L| |L|^T)_ab <= sqrt(S_aa S_bb) by Cauchy-Schwarz); the bound of the
GPU tests is 10 units.  Cholesky in double runs to completion when (m + 8) 2^-53 kappa2(S) m < 1 (the same theorem's
condition, loosely); KAPPA_S_MAX = 10^9 is far inside it for every block here (m <= 700).
"""
import numpy as np

import _cov_cases as CC
import _cov_refs as CR
from _loo_refs import LD

U53 = 2.0 ** -53
RATIO_MAX = 10.0
KAPPA_S_MAX = 1e9                                            # kappa2(S_r) of every block factored without jitter
NQ_MAIN = 40                                                 # the first queries of _cov_cases.Main

# ---- tile edges through explicit items: sixteen regions of a 16-leaf tree, patches of about 150 points
TILE_COUNTS = [1, 31, 32, 33, 127, 128, 129, 257, 385, 0, 5, 64, 0, 96, 2, 160]
TILE_PATCH = 150


def block_unit(S):
    """(m + 8) 2^-53 sqrt(S_aa S_bb) [m, m] float64"""
    d = np.sqrt(np.abs(np.asarray(np.diag(S), dtype=np.float64)))
    return (len(d) + 8) * U53 * np.outer(d, d)


def factor_ratio(L, S):
    """worst |L L^T - S| / unit, the product in long double"""
    L = np.asarray(L, dtype=LD)
    err = np.abs(L @ L.T - np.asarray(S, dtype=LD)).astype(np.float64)
    return float((err / block_unit(S)).max()) if len(L) else 0.0


def kappa2(S):
    s = np.linalg.svd(np.asarray(S, dtype=np.float64), compute_uv=False)
    return float(s[0] / s[-1]) if s[-1] > 0 else float("inf")


def sorted_layout(items):
    """(order [total]: item of each sorted position, roff {region: first position}) from (item_offsets, item_region)"""
    off, reg = np.asarray(items[0], dtype=np.int64), np.asarray(items[1], dtype=np.int64)
    query_of = np.repeat(np.arange(len(off) - 1), np.diff(off))
    order, roff = [], {}
    for r in sorted(set(int(v) for v in reg)):
        sel = np.nonzero(reg == r)[0]
        roff[r] = len(order)
        order += list(sel[np.argsort(query_of[sel], kind="stable")])
    return np.array(order, dtype=np.int64), roff


def weight_matrix(items, t, wth):
    """W [Nq, total] in long double: W[query(i), position(i)] = wn_i"""
    off = np.asarray(items[0], dtype=np.int64)
    order, _ = sorted_layout(items)
    wn = CR.blend_weights(off, t, wth)
    query_of = np.repeat(np.arange(len(off) - 1), np.diff(off))
    W = np.zeros((len(off) - 1, len(order)), dtype=LD)
    W[query_of[order], np.arange(len(order))] = wn[order]
    return W


def cholesky_psd_ld(S):
    """left-looking Cholesky in long double of a positive semi-definite block: a pivot that is zero to long-double rounding
    (the second item of a query that holds two items of the region repeats a row) gives a zero column, so L L^T = S holds
    for such a block too"""
    S = np.asarray(S, dtype=LD)
    n = len(S)
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        col = S[j:, j] - L[j:, :j] @ L[j, :j]
        if col[0] > 64 * np.finfo(LD).eps * S[j, j]:
            L[j:, j] = col / np.sqrt(col[0])
    return L


def region_factors(S_blocks):
    """{r: L_r} in long double from {r: (idx, S_r)}"""
    return {r: cholesky_psd_ld(S) for r, (_, S) in S_blocks.items()}


def blend_matrix(items, factors, t, wth):
    """A = W blockdiag(L_r) [Nq, total] in long double; factors {r: L_r} for every region with items"""
    W = weight_matrix(items, t, wth)
    _, roff = sorted_layout(items)
    A = np.zeros_like(W)
    for r, L in factors.items():
        m = len(L)
        A[:, roff[r]:roff[r] + m] = W[:, roff[r]:roff[r] + m] @ np.asarray(L, dtype=LD)
    return A


# ---- the inputs of the GPU tests
def main_queries(m):
    """about 40 queries of the main workload: its first NQ_MAIN"""
    return np.ascontiguousarray(m.Xq[:NQ_MAIN])


class MainSub:
    """the main workload of _cov_cases.py with the queries of main_queries: what oracle_items needs"""

    def __init__(self, m, Xq=None):
        self.X, self.LEVELS, self.RADIUS, self.DELTA = m.X, m.LEVELS, m.RADIUS, m.DELTA
        self.Xq = main_queries(m) if Xq is None else Xq


def duplicated_queries(m):
    """the queries of main_queries with query 7 given again at the end, and the plan radius 0 (home items only): one
    region holds the same point twice"""
    Xq = main_queries(m)
    return np.ascontiguousarray(np.vstack([Xq, Xq[7:8]]))


def tile_patches(seed=900):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-2, 2, (TILE_PATCH + 3 * r, 2)) for r in range(len(TILE_COUNTS))]


def tile_items(seed=901):
    """(xq [n, 2], region [n]) in a shuffled order: TILE_COUNTS[r] points for region r, spread over the square of its
    patch so that the blocks stay well conditioned"""
    rng = np.random.default_rng(seed)
    xq, region = [], []
    for r, cnt in enumerate(TILE_COUNTS):
        xq.append(rng.uniform(-2.5, 2.5, (cnt, 2)))
        region += [r] * cnt
    perm = rng.permutation(len(region))
    return np.vstack(xq)[perm], np.array(region, dtype=np.int32)[perm]
