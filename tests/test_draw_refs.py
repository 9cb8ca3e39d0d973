"""CPU checks of the reference of the block draws (tests/_draw_refs.py): the conditions the GPU tests of
tests/test_gpu_draw.py assume hold of the reference alone, on the same inputs.

1. A A^T, A = W blockdiag(L_r) from the long-double region blocks, equals _cov_refs.mix_cov_ref to long-double rounding,
   on the main workload's sub-batch and on the 512-leaf workload, which holds a query with two items of one region.
2. Plain numpy.linalg.cholesky in double stays under one unit (m + 8) 2^-53 sqrt(S_aa S_bb) of L L^T - S on every block
   the GPU file factors: a tenth of its bound.
3. Every block factored without jitter has kappa2(S_r) <= KAPPA_S_MAX = 10^9, and the pivot rule of the device (a pivot not
   above 2^-50 of its diagonal entry is no pivot) passes all of them at rel = 0; the block with a duplicated query fails
   it at the second copy, and passes on the ladder rel = 2^-52, x 10.
"""
import numpy as np
import pytest

import _cov_cases as CC
import _cov_refs as CR
import _draw_refs as DR

LD = DR.LD


def _ref_blocks(oth, Xs, sigma2, items, Xq):
    return {r: (idx, CR.RegionRef(oth, Xs[r], sigma2).cov(pts)["S"]) for r, (idx, pts) in CC.blocks_of(items, Xq).items()}


def pivot_rule(S, jitter=0.0):
    """left-looking Cholesky in double with the device's pivot rule -> 0, or the index (from 1) of the first pivot that is
    NaN or not above 2^-50 (S_kk + jitter)"""
    S = np.array(S, dtype=np.float64) + jitter * np.eye(len(S))
    L = np.zeros_like(S)
    for j in range(len(S)):
        s = S[j, j] - L[j, :j] @ L[j, :j]
        if not (s > 0.0 and s > 2.0 ** -50 * S[j, j]):
            return j + 1
        L[j, j] = np.sqrt(s)
        L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return 0


def _check_workload(name, oth, Xs, sigma2, items, Xq, owth, doubled=()):
    S_blocks = _ref_blocks(oth, Xs, sigma2, items, Xq)
    Cov = CR.mix_cov_ref(items[:2], S_blocks, items[2], owth)
    A = DR.blend_matrix(items[:2], DR.region_factors(S_blocks), items[2], owth)
    scale = np.sqrt(np.outer(np.diag(Cov), np.diag(Cov))).astype(np.float64)
    err = float((np.abs(A @ A.T - Cov).astype(np.float64) / scale).max())
    shared = CR.shared_region_mask(items[:2])
    assert np.all((A @ A.T)[~shared] == 0)
    lapack = kappa = 0.0
    for r, (idx, S) in S_blocks.items():
        Sd = np.asarray(S, dtype=np.float64)
        if r in doubled:
            # a query with two items of the region repeats a row: the block is singular and needs the jitter ladder
            assert pivot_rule(Sd) == int(np.nonzero(np.diff(idx) == 0)[0][0]) + 2, r
            continue
        kappa = max(kappa, DR.kappa2(Sd))
        lapack = max(lapack, DR.factor_ratio(np.linalg.cholesky(Sd), Sd))
        assert pivot_rule(Sd) == 0, r
    print("DRAWREF %s: A A^T against mix_cov_ref %.3g of sqrt(C_jj C_kk); LAPACK worst L L^T ratio %.3g; kappa2(S) <= %.3g"
          % (name, err, lapack, kappa))
    # long double carries 64 bits: a sum of a few hundred products of that precision
    assert err <= 1e3 * float(np.finfo(LD).eps), err
    assert lapack < 1.0 and kappa <= DR.KAPPA_S_MAX, (lapack, kappa)
    return S_blocks


@pytest.mark.parametrize("family,dtype", [("spline34", "f64"), ("gaussian", "f64"), ("spline34", "f32")])
def test_the_main_sub_batch(family, dtype):
    m = CC.Main(dtype)
    sub = DR.MainSub(m)
    items = CC.oracle_items(sub)
    assert len(set(int(r) for r in items[1])) == 4 and np.diff(items[0]).max() >= 2
    _check_workload("main %s %s" % (family, dtype), CC.FAMILIES[family][1], m.Xs, CC.SIGMA2[dtype], items, sub.Xq, m.owth)


def test_the_many_leaves_workload_with_a_doubled_query():
    mm = CC.Many()
    items = CC.oracle_items(mm)
    blocks = CC.blocks_of(items, mm.Xq)
    doubled = [r for r, (idx, _) in blocks.items() if np.any(np.diff(idx) == 0)]
    assert doubled, "no query holds two items of one region"
    _check_workload("many", CC.FAMILIES["spline34"][1], mm.Xs, CC.SIGMA2["f64"], items, mm.Xq, mm.owth, doubled)


def test_the_tile_edge_blocks():
    Xs = DR.tile_patches()
    xq, region = DR.tile_items()
    oth = CC.FAMILIES["spline34"][1]
    assert {1, 31, 32, 33, 127, 128, 129, 257, 385, 0} <= set(DR.TILE_COUNTS)
    lapack = kappa = 0.0
    for r, cnt in enumerate(DR.TILE_COUNTS):
        assert (region == r).sum() == cnt
        if cnt == 0:
            continue
        S = np.asarray(CR.RegionRef(oth, Xs[r], CC.SIGMA2["f64"]).cov(xq[region == r])["S"], dtype=np.float64)
        kappa = max(kappa, DR.kappa2(S))
        lapack = max(lapack, DR.factor_ratio(np.linalg.cholesky(S), S))
        assert pivot_rule(S) == 0, r
    print("DRAWREF tiles: LAPACK worst L L^T ratio %.3g; kappa2(S) <= %.3g" % (lapack, kappa))
    assert lapack < 1.0 and kappa <= DR.KAPPA_S_MAX, (lapack, kappa)


def test_the_duplicated_query_fails_at_rel_zero_and_passes_on_the_ladder():
    m = CC.Main("f64")
    Xq = DR.duplicated_queries(m)
    sub = DR.MainSub(m, Xq)
    sub.RADIUS = 0.0                                             # home items only: one region holds the two copies
    items = CC.oracle_items(sub)
    assert np.all(np.diff(items[0]) == 1)
    home = int(items[1][7])
    assert int(items[1][-1]) == home
    S_blocks = _ref_blocks(CC.FAMILIES["spline34"][1], m.Xs, CC.SIGMA2["f64"], items, Xq)
    for r, (idx, S) in S_blocks.items():
        Sd = np.asarray(S, dtype=np.float64)
        k = pivot_rule(Sd)
        if r != home:
            assert k == 0, (r, k)
            continue
        assert list(idx[-1:]) == [len(Xq) - 1] and k == len(idx), (idx, k)           # the second copy, the last row
        assert DR.kappa2(Sd) > 1e15
        rel, tried = 2.0 ** -52, 0
        while pivot_rule(Sd, rel * np.trace(Sd) / len(Sd)):
            rel *= 10.0
            tried += 1
            assert rel <= 2.0 ** -26
        print("DRAWREF duplicate: region %d fails at pivot %d of %d, passes at rel = 2^-52 x 10^%d" % (r, k, len(idx), tried))
