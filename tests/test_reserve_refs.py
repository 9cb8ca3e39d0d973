"""CPU-side checks of the inputs of tests/test_gpu_reserve.py (tests/_reserve_cases.py) against the oracle: every extended
point set has a positive definite K + sigma2 I (+ addends) that the oracle factors, and the kappa2(L') that the error unit
of the crossing cases multiplies stays below the 10^3 that tests/_append_cases.py promises of its own cases, in both
precisions' roundings of the points.  Also the arithmetic the GPU file expects of the strides."""
import numpy as np
import pytest

from oracle import oracle as O
import _append_cases as AC
import _append_refs as AR
import _reserve_cases as RC


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_every_extended_set_is_positive_definite_and_well_conditioned(dtype):
    worst = 0.0
    for name, X, diag, fam, s2 in RC.all_extended(dtype):
        fit = O.fit_patch(AC.FAMILIES[fam][1], X, AC.target(X), s2, want_K=True, diag=diag)
        assert fit["info"] == 0, name
        U = fit["K"].copy()
        U[np.diag_indices(len(U))] += s2
        assert np.linalg.eigvalsh(U).min() > 0, name
        kappa = AR.kappa_of(U)
        worst = max(worst, kappa)
        assert kappa <= RC.KAPPA_MAX, (name, kappa)
    print("RESERVE_REFS", dtype, "worst kappa2(L')", worst)


def test_the_sizes_meet_the_boundaries_they_are_named_for():
    tiles = lambda n: (n + 127) // 128
    by_n = {n: (n, m) for n, m in RC.CROSS_SIZES}
    assert by_n[100][0] + by_n[100][1] == 128 and by_n[128][1] == 1 and tiles(120 + by_n[120][1]) == 2
    n, m = by_n[127]
    assert m == 128 and (n + m - 1) // 32 - n // 32 + 1 == 5           # 128 rows over five diagonal blocks
    assert by_n[1][1] == 128 and tiles(250) == 2 and tiles(250 + by_n[250][1]) == 3
    assert tiles(200) == tiles(200 + by_n[200][1])                      # stays inside its block row
    assert all(m <= 128 and m <= RC.ld_after(n, RC.RESERVE_ROWS) - n for n, m in RC.CROSS_SIZES + RC.REORDER_SIZES)
    before = [tiles(n) for n, _ in RC.REORDER_SIZES]
    after = [tiles(n + m) for n, m in RC.REORDER_SIZES]
    assert min(range(4), key=lambda r: RC.REORDER_SIZES[r][0]) == 0 and max(before) == 1
    assert after[0] == 2 and max(after[1:]) == 1                        # the smallest patch becomes the largest
    # strides of the stride case: 100 + 0 and 129 + 1 keep theirs
    lds = [RC.ld_after(n, r) for n, r in zip(RC.STRIDE_SIZES, RC.STRIDE_RESERVE)]
    assert lds == [256, 128, 256, 256, 512]
    more = [RC.ld_after(n, r, ld) for n, r, ld in zip(RC.STRIDE_SIZES, RC.STRIDE_RESERVE_MORE, lds)]
    assert more == [256, 256, 384, 256, 640]


def test_the_tree_case_crosses_a_block_row_and_stays_well_conditioned():
    """RC.TreeCross: the oracle's assignment of the new points gives at least two patches more points than their free
    rows without a reserve and takes them into a second block row, at most 128 points per patch; the extended eps-sets
    are positive definite with kappa2(L') <= 10^3"""
    t = RC.TreeCross("f64")
    ob = O.BSP(t.X, t.LEVELS)
    off0 = ob.assign(t.X, t.EPS)[0]
    n0 = np.diff(off0)
    counts = np.diff(ob.assign(t.Xnew, t.EPS)[0])
    tiles = lambda v: (v + 127) // 128
    assert counts.max() <= 128
    assert (counts > 128 * tiles(n0) - n0).sum() >= 2 and (tiles(n0 + counts) > tiles(n0)).sum() >= 2, (n0, counts)
    off, inds = ob.assign(t.Xall, t.EPS)[:2]
    s2 = AC.SIGMA2["f64"]
    for r in range(len(n0)):
        X = t.Xall[inds[off[r]:off[r + 1]]]
        fit = O.fit_patch(AC.FAMILIES["spline34"][1], X, AC.target(X), s2, want_K=True)
        assert fit["info"] == 0 and AR.kappa_of(fit["K"] + s2 * np.eye(len(X))) <= RC.KAPPA_MAX, r
