"""What tests/test_gpu_remove_after.py relies on, checked without a device (references in tests/_remove_after_refs.py).

For the tree of tests/_append_cases.Tree in both precisions and the set G of _remove_after_refs.removed_set: G is what its
rule says (the ends of every list, the points 0 and N - 1, points of two patches, patch 0 at the edge of its band, no
patch beyond its removable rows or the 32 of one call); the reduced lists ascend; every point of G is homeless; kappa2 of
every reduced patch is <= 10^3; the closed form of the blended leave-one-out on the REDUCED factor agrees with brute-force
refits at kept points of patch 0 and of two patches and at points of G, within the bound tests/test_append_after_refs.py
holds the closed form to.  For the mixed appends and removals: every step stays within capacity, removable rows and the
cap.  For the new `slabs` case of tests/_remove_cases.py: it holds the shapes it is there for.
"""
import numpy as np
import pytest

import _append_cases as AC
import _append_refs as AR
import _loo_blend_refs as BR
import _remove_after_refs as RA
import _remove_cases as RC
from oracle import oracle as O


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_the_removed_set_is_what_its_rule_says(dtype):
    t, G, o = RA.tree_oracle(dtype)
    N = len(t.X)
    full = RA.tree_lists(t, t.X)
    assert [len(s) for s in full] == [149, 122, 153, 123]
    assert [RC.removable(len(s)) for s in full] == [20, 121, 24, 122]
    mult = RA.multiplicity(full, N)
    assert (mult == 2).sum() == 147 and mult.max() == 2 and mult.min() == 1
    assert len(set(G.tolist())) == len(G) and 0 in G and N - 1 in G
    for r, s in enumerate(full):
        assert s[0] in G and s[-1] in G, r
    assert (mult[G] == 2).sum() >= 4
    lost = np.array([int(np.isin(s, G).sum()) for s in full])
    assert lost[0] == 20 and len(o.sets[0]) == 129                          # patch 0 at the edge of its band
    assert np.all(lost <= [RC.removable(len(s)) for s in full]) and np.all(lost <= RC.MAX_ROWS) and np.all(lost >= 2), lost
    # the reduced lists: the full ones without G, ascending, with new first and last entries
    for r, s in enumerate(full):
        assert np.array_equal(o.sets[r], s[~np.isin(s, G)]), r
        assert np.all(np.diff(o.sets[r]) > 0), r
        assert o.sets[r][0] != s[0] and o.sets[r][-1] != s[-1], r
    for j in G:
        assert all(o.row_of(r, int(j)) < 0 for r in range(o.P)), j
    total, strip, multi, homeless = o.counts(t.RADIUS, t.DELTA)
    assert homeless == len(G) and multi >= 1 and 0 < strip < total
    # the plan is that of the whole array: the tree and the points have not changed
    whole = BR.Oracle(t.X, t.y, t.EPS, RA.hyper(dtype), t.LEVELS)
    assert whole.counts(t.RADIUS, t.DELTA)[0] == total
    s2 = AC.SIGMA2[dtype]
    for r, f in enumerate(o.fits):
        assert AR.kappa_of(f["K"] + s2 * np.eye(len(f["K"]))) <= AC.KAPPA_MAX, r
    mine, other, gone = RA.multi_points(o, G)
    assert all(o.row_of(0, j) >= 0 for j in mine) and mine[0] == o.sets[0][0] and mine[-1] == o.sets[0][-1]
    assert all(o.row_of(0, j) < 0 and j not in G for j in other) and all(j in G for j in gone)
    assert any(RA.multiplicity(o.sets, N)[j] == 2 for j in other)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_closed_form_of_a_reduced_model_against_refits(dtype):
    t, G, o = RA.tree_oracle(dtype)
    s2 = AC.SIGMA2[dtype]
    own, two = RA.kept_points(o)
    mult = RA.multiplicity(o.sets, len(t.X))
    assert all(o.row_of(0, j) >= 0 for j in own) and own[0] == o.sets[0][0] and own[2] == o.sets[0][-1]
    assert all(mult[j] == 2 for j in two)
    pts = own + two + [int(G[0]), int(G[-1])]
    wth = O.kernel(O.SPLINE34, 1.0 / t.RADIUS)
    for noisy in (False, True):
        Yr, Vr = (o.blend_refit_noisy if noisy else o.blend_refit)(wth, t.RADIUS, pts, t.DELTA)
        Yc, Vc = o.blend_closed(wth, t.RADIUS, noisy, t.DELTA)
        ry, rv = BR.ratios(Yc[pts], Vc[pts], Yr, Vr, o.cond2(), 2.0 ** -53, np.abs(o.y).max(), o.k0() + s2)
        print("REMOVE_AFTER_REF", dtype, noisy, dict(dY=ry, dV=rv, cond2=o.cond2()))
        assert ry <= 1.0 and rv <= 1.0, (ry, rv)
    # nothing was refitted for the points of G
    assert not any(j in G for _, j in o._refits)
    assert {r for r, _ in o._refits} >= {0}


def test_the_leaves_case_against_refits():
    """eps=None: every leaf loses the two ends of its list, every kept point is a member of its home leaf alone, every
    removed point of none; the closed form on the reduced leaves against refits at every point"""
    X, y, G, o = RA.leaves_case("f64")
    s2 = AC.SIGMA2["f64"]
    whole = BR.Oracle(X, y, None, RA.hyper("f64"), RA.LEAF_LEVELS)
    assert o.P == 4 and sum(len(s) for s in whole.sets) == len(X)
    for r, s in enumerate(whole.sets):
        assert s[0] in G and s[-1] in G and np.array_equal(o.sets[r], s[~np.isin(s, G)]), r
        assert 2 <= np.isin(s, G).sum() <= RC.removable(len(s)), r
        assert AR.kappa_of(o.fits[r]["K"] + s2 * np.eye(len(o.sets[r]))) <= AC.KAPPA_MAX, r
    radius = 0.6
    total, strip, _, homeless = o.counts(radius)
    assert homeless == len(G) and total - strip == len(X) - len(G)
    wth = O.kernel(O.SPLINE34, 1.0 / radius)
    Yr, Vr = o.blend_refit(wth, radius)
    Yc, Vc = o.blend_closed(wth, radius)
    ry, rv = BR.ratios(Yc, Vc, Yr, Vr, o.cond2(), 2.0 ** -53, np.abs(y).max(), o.k0() + s2)
    assert ry <= 1.0 and rv <= 1.0, (ry, rv)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_the_mixed_steps_stay_within_capacity_and_band(dtype):
    t, steps = RA.mixed_steps(dtype)
    n0 = len(t.X)
    assert [s.kind for s in steps] == ["remove", "append", "remove", "append"]
    assert [s.N for s in steps] == [n0, n0 + 18, n0 + 18, n0 + 22]
    ld = [RA.ld_of(len(s)) for s in RA.tree_lists(t, t.X)]
    assert ld == [256, 128, 256, 128]
    n = np.array([len(s) for s in RA.tree_lists(t, t.X)])
    for k, st in enumerate(steps):
        now = np.array([len(s) for s in st.sets])
        if st.kind == "remove":
            lost = n - now
            assert np.all(lost <= [RC.removable(int(v)) for v in n]) and np.all(lost <= RC.MAX_ROWS), (k, lost)
            assert lost.sum() >= len(st.points)
        else:
            assert np.all(now >= n) and np.all(now <= ld) and now.sum() > n.sum(), (k, now)
        for r, s in enumerate(st.sets):
            assert np.all(np.diff(s) > 0) and not np.isin(s, st.removed).any() and s[-1] < st.N, (k, r)
        n = now
    # the third call takes the first entry of a list, the last old entry of another, and a new point of two patches
    third = steps[2].points
    before = steps[1].sets
    assert third[0] == before[1][0] and third[1] == steps[0].sets[3][-1] and third[1] in before[3]
    mult = RA.multiplicity(before, steps[1].N)
    assert sorted(mult[third[2:]].tolist()) == [1, 1, 2] and np.all(third[2:] >= n0)
    # every patch was met by an append and by a removal
    assert np.all(np.array([len(s) for s in steps[1].sets]) > [len(s) for s in steps[0].sets])
    s2 = AC.SIGMA2[dtype]
    oth = AC.FAMILIES["spline34"][1]
    for st in steps:
        for r, s in enumerate(st.sets):
            assert AR.kappa_of(O.kernel_matrix(oth, st.X[s]) + s2 * np.eye(len(s))) <= AC.KAPPA_MAX, r


def test_the_slabs_case_holds_its_shapes():
    case = {name: c for name, c, _, _ in RC.all_cases("f64")}["slabs"]
    shapes = [(n, tuple(int(v) for v in rows)) for n, rows in case.sizes]
    full = [(n, rows) for n, rows in shapes if n % 128 == 0]
    assert any(rows[0] == 0 for n, rows in full)                            # a full patch with k0 = 0
    assert any(rows == (n - 1,) for n, rows in full)                        # ... that loses its last row only
    assert any(n - len(rows) - rows[0] > 512 and len(rows) < 8 for n, rows in shapes)          # a third chunk of the row loop
    assert any(n - len(rows) - rows[0] > 512 and len(rows) == RC.MAX_ROWS for n, rows in shapes)
    runs = [(n, rows) for n, rows in shapes if len(rows) == 32 and rows[-1] - rows[0] == 31]
    assert any(rows[0] // 128 == rows[-1] // 128 for _, rows in runs)       # one run of 32 rows inside a tile
    assert any(rows[0] // 128 < rows[-1] // 128 for _, rows in runs)        # ... and astride the tile edge
    for n, rows in shapes:
        assert len(rows) <= min(RC.removable(n), RC.MAX_ROWS) and len(set(rows)) == len(rows)
