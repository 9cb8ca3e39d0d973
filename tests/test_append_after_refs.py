"""What tests/test_gpu_append_after.py relies on, checked without a device (references in tests/_append_after_refs.py).

For the tree of tests/_append_cases.Tree in both precisions: the closed form of the blended leave-one-out of an APPENDED
model (the tree of the original points, the index lists of the extended array) agrees with brute-force refits at the 18 new
points and 18 old ones, within the bound tests/test_loo_blend_abi.py holds the closed form to (|dY| <= cond_2 u max|y|,
|dV| <= cond_2 u (k(0) + sigma2), u = 2^-53); kappa2 of every extended patch is <= 10^3; the new points include members of
one, two and three or more patches.  For the models of the other GPU tests: kappa2 <= 10^3 of every set they reach.
"""
import numpy as np
import pytest

from oracle import oracle as O

import _append_after_refs as AA
import _append_cases as AC
import _append_refs as AR
import _loo_blend_refs as BR


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_closed_form_of_an_appended_model_against_refits(dtype):
    t, o = AA.tree_oracle(dtype)
    s2, n0 = AC.SIGMA2[dtype], len(t.X)
    # the lists are those of an append: the old list of the original tree, then the new entries, ascending
    old = BR.Oracle(t.X, t.y, t.EPS, AA.hyper(dtype), t.LEVELS)
    ooff, oinds, oloff, _ = O.BSP(t.X, t.LEVELS).assign(t.Xnew, t.EPS)
    for r in range(o.P):
        assert np.array_equal(o.sets[r], np.concatenate([old.sets[r], n0 + oinds[ooff[r]:ooff[r + 1]]])), r
        assert np.all(np.diff(o.sets[r]) > 0), r
    mult = AA.multiplicity(o, n0)
    assert np.array_equal(mult, np.diff(oloff))
    assert (mult == 1).any() and (mult == 2).any() and (mult >= 3).any(), mult
    for r, f in enumerate(o.fits):
        assert AR.kappa_of(f["K"] + s2 * np.eye(len(f["K"]))) <= AC.KAPPA_MAX, r
    wth = O.kernel(O.SPLINE34, 1.0 / t.RADIUS)
    total, strip, multi, homeless = o.counts(t.RADIUS, t.DELTA)
    assert homeless == 0 and multi >= 1 and 0 < strip < total
    pts = AA.check_points(t)
    assert len(pts) == 36 and sum(j >= n0 for j in pts) == 18
    for noisy in (False, True):
        Yr, Vr = (o.blend_refit_noisy if noisy else o.blend_refit)(wth, t.RADIUS, pts, t.DELTA)
        Yc, Vc = o.blend_closed(wth, t.RADIUS, noisy, t.DELTA)
        ry, rv = BR.ratios(Yc[pts], Vc[pts], Yr, Vr, o.cond2(), 2.0 ** -53, np.abs(o.y).max(), o.k0() + s2)
        print("APPEND_AFTER_REF", dtype, noisy, dict(items=total, strip=strip, dY=ry, dV=rv))
        assert ry <= 1.0 and rv <= 1.0, (ry, rv)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_the_other_models_are_as_well_conditioned(dtype):
    oth, s2 = AC.FAMILIES["spline34"][1], AC.SIGMA2[dtype]
    case = AA.shapes(dtype)
    assert [n for n, _ in case.sizes] == list(AA.SHAPE_N)
    # patches 0 to 2 end exactly full, patch 3 keeps room
    assert [128 * ((n + 127) // 128) - n - m for n, m in case.sizes] == [0, 0, 0, 124]
    for k in range(len(AA.SHAPE_CALLS)):
        assert max(AA.kappas(AA.shape_sets(case, k)[0], oth, s2)) <= AC.KAPPA_MAX, k
    for k in range(len(AA.SHAPE_CALLS)):
        Xn, yn = AA.shape_call(case, k)
        assert tuple(len(x) for x in Xn) == AA.SHAPE_CALLS[k] == tuple(len(y) for y in yn)
    Xe, _ = AA.shape_sets(case, len(AA.SHAPE_CALLS) - 1)
    assert all(np.array_equal(a, b) for a, b in zip(Xe, case.Xe))
    trend = AA.trend_case(dtype)
    assert trend.sizes[AA.TREND_TWO] == (2, 2) and trend.D == 2 and trend.P == 8          # n = 2 <= q = 3 < n + m = 4
    assert max(AA.kappas(trend.Xe, oth, s2)) <= AC.KAPPA_MAX
    assert max(AA.kappas(trend.Xs, oth, s2)) <= AC.KAPPA_MAX
