"""The references and workloads of tests/test_gpu_loo_blend_edges.py, checked on the CPU: for every workload of
tests/_loo_blend_edge_cases.py the closed form in fp64 (blend_closed, items(..., "closed64")) against the brute-force
refits, by the rule the GPU test applies to the device, and the preconditions the workloads were chosen for (patch sizes,
item counts, homeless points, the single non-member, the growth inequality), all from the oracle.  A failure of the GPU
module is then a property of the device code, not of its inputs.
"""
import numpy as np
import pytest

from oracle import oracle as O

import _loo_blend_refs as BR
import _loo_blend_multi_refs as MR
import _loo_blend_edge_cases as EC
import _trend_refs as TR

U64 = 2.0 ** -53


def _wth(radius):
    return O.kernel(O.SPLINE34, 1.0 / radius)


def _multi_ratios(o, radius, points=None):
    """(dY, dV) of the fp64 closed form against the GPU tests' reference, in units of cond_2 u scale"""
    w = _wth(radius)
    _, MUr, Vr = o.blend(w, o.items(radius, "ref", points=points))
    _, MUc, Vc = o.blend(w, o.items(radius, "closed64", points=points))
    return MR.ratios(MUc, Vc, MUr, Vr, o.cond2(), U64, np.abs(o.Y).max(), o.k0() + BR.SIGMA2)


def _single_ratios(o, radius):
    w = _wth(radius)
    Yc, Vc = o.blend_closed(w, radius)
    Yr, Vr = o.blend_refit(w, radius)
    return BR.ratios(Yc, Vc, Yr, Vr, o.cond2(), U64, np.abs(o.y).max(), o.k0() + BR.SIGMA2)


# ------------------------------------------------------------------------------------ the helpers' arguments
def test_the_oracles_take_depth_and_dimension_from_their_arguments():
    for name, c in EC.DIMS.items():
        o = EC.dim_oracle(name)
        assert o.P == 2 ** (c["levels"] - 1) and o.D == c["D"] and o.X.shape == (c["N"], c["D"])
        assert o.k0() == 1.0
    X, y = BR.workload()
    base = BR.Oracle(X, y, 0.3, EC.UNIFORM)                 # the defaults are the base workload's
    assert base.P == 2 ** (BR.LEVELS - 1) and base.D == BR.D and base.levels == BR.LEVELS


def test_recorded_refits_serve_their_own_workload_only():
    """the file's keys name eps and the trend only: a workload with other points must compute its refits, whatever its
    (r, j) pairs are"""
    X, Y = MR.targets(MR.GOLDEN_R)
    base = MR.MultiOracle(X, Y, 0.3, EC.UNIFORM, "linear")
    assert base.is_recorded_workload() and len(base._recorded()) == sum(len(s) for s in base.sets)
    for name in ("D1", "D3", "D3_deep", "D4"):
        o = EC.dim_oracle(name, "linear")
        assert o.R == MR.GOLDEN_R and not o.is_recorded_workload() and o._recorded() == {}
    # the base points with other targets, under a deeper tree, or with other hyperparameters
    Y2 = np.asfortranarray(Y.copy())
    Y2[5, 1] += 1e-9
    assert not MR.MultiOracle(X, Y2, 0.3, EC.UNIFORM, "linear").is_recorded_workload()
    assert not MR.MultiOracle(X, Y, 0.3, EC.UNIFORM, "linear", 4).is_recorded_workload()
    assert not MR.MultiOracle(X, Y, 0.3, [(("s34", 0.7), BR.SIGMA2)], "linear").is_recorded_workload()
    assert EC.dup_oracle("linear")._recorded() == {} and EC.count_oracle(257, "linear")._recorded() == {}


# ------------------------------------------------------------------------------------ dimensions
@pytest.mark.parametrize("name", list(EC.DIMS))
def test_dimension_workloads_single_output(name):
    c = EC.DIMS[name]
    o = EC.dim_oracle(name)
    total, other, multi, homeless = o.counts(c["radius"])
    assert multi >= 1 and 0 < other < total
    assert (homeless >= 1) == c["homeless"], homeless
    ry, rv = _single_ratios(o, c["radius"])
    print(name, "sizes", [len(s) for s in o.sets], "counts", (total, other, multi, homeless), "cond2 %.4g" % o.cond2(),
          "ratios", ry, rv)
    assert ry <= 1.0 and rv <= 1.0, (ry, rv)


@pytest.mark.parametrize("name, trend, R", EC.DIM_MULTI)
def test_dimension_workloads_multi_output(name, trend, R):
    c = EC.DIMS[name]
    o = EC.dim_oracle(name, trend, R)
    assert R + EC.Q_OF[trend](c["D"]) <= 16
    if R > 3:
        assert R + EC.Q_OF[trend](c["D"]) == 16
    ry, rv = _multi_ratios(o, c["radius"])
    print(name, trend, R, "ratios", ry, rv)
    assert ry <= 1.0 and rv <= 1.0, (ry, rv)


# ------------------------------------------------------------------------------------ small patches
@pytest.mark.parametrize("N", EC.SMALL_PLAIN)
def test_small_patches_without_a_trend(N):
    """every patch has exactly N / 8 points; at one point per patch the refit has no points and the item is the prior"""
    o = EC.small_oracle(2, N, None)
    r = EC.SMALL["radius"]
    assert [len(s) for s in o.sets] == [N // 8] * 8
    total, other, multi, homeless = o.counts(r)
    assert multi >= 1 and homeless == 0 and other == total - N > 0
    fy, fv = _single_ratios(o, r)
    my, mv = _multi_ratios(o, r)
    print(N, "fp64 closed form against the refits: single", fy, fv, "multi", my, mv)
    assert all(np.isfinite(a) for a in (fy, fv, my, mv))
    if N == 8:
        for j, row in o.items(r, "ref").items():
            _, Uj, vj, mem = row
            assert mem[-1] and np.all(Uj[-1] == 0.0) and vj[-1] == o.k0()           # the prior, exactly
        for row in o.items_closed(r):
            assert row[-1][1] and abs(row[-1][2]) <= 10 * U64 * np.abs(o.y).max()
            assert abs(row[-1][3] - o.k0()) <= 10 * U64 * (o.k0() + BR.SIGMA2)


@pytest.mark.parametrize("D, N, trend", EC.SMALL_TREND)
def test_small_patches_with_a_trend_at_q_plus_one_points(D, N, trend):
    o = EC.small_oracle(D, N, trend)
    r = EC.SMALL["radius"]
    q = EC.Q_OF[trend](D)
    assert [len(s) for s in o.sets] == [q + 1] * 8
    total, other, multi, homeless = o.counts(r)
    assert multi >= 1 and homeless == 0 and other == total - N > 0
    my, mv = _multi_ratios(o, r)
    print(D, N, trend, "fp64 closed form against the refits:", my, mv)
    assert np.isfinite(my) and np.isfinite(mv)
    # the per-patch values against n refits
    for p, s in enumerate(o.sets):
        K, H = o.fits[p]["K"], MR.basis(o.X[s], trend)
        res, var = TR.brute_force_loo(K, BR.SIGMA2, o.Y[s], H)
        f = TR.gls_fp64(K, BR.SIGMA2, o.Y[s], H)
        assert np.all(np.isfinite(f["res"])) and np.all(f["var"] > 0)
        assert np.abs(f["res"] - res).max() <= 1e-6 * max(1.0, float(np.abs(res).max()))
        assert np.abs(f["var"] - var).max() <= 1e-6 * float(var.max())


@pytest.mark.parametrize("D, N, trend", EC.AT_Q)
def test_patches_of_exactly_q_points(D, N, trend):
    """n = q: the fit interpolates the trend, and Q_ii of the closed form is rounding noise around 0 (exactly 0 for one
    point and a constant): what the device must answer with NaN"""
    o = EC.small_oracle(D, N, trend)
    q = EC.Q_OF[trend](D)
    assert [len(s) for s in o.sets] == [q] * 8
    total, other, multi, homeless = o.counts(EC.SMALL["radius"])
    assert homeless == 0 and other > 0
    for p in range(o.P):
        # exactly, Q = 0; in fp64 what is left of d_i (about 1) is its rounding error amplified by cond(G): noise, nine
        # orders below d, whose reciprocal the blend would clamp into a variance of 1e-12
        f = o.fit64(p)
        d = np.diag(np.linalg.inv(f["U"]))
        assert np.abs(f["Q"]).max() <= 1e-9 * d.min(), (f["Q"], d)


def _mixed_points(o, radius):
    """(points with a member item in a patch of n <= q points, the other points)"""
    q = EC.Q_OF[o.trend](o.D)
    home, regs, _ = o.plan(radius)
    hit = [j for j in range(len(o.X))
           if any(o.row_of(int(r), j) >= 0 and len(o.sets[int(r)]) <= q for r in list(regs[j]) + [int(home[j])])]
    return hit, [j for j in range(len(o.X)) if j not in hit]


def test_the_mixed_tree_has_both_kinds_of_leaves():
    o = EC.mixed_oracle()
    q, r = EC.Q_OF[o.trend](o.D), EC.MIXED["radius"]
    sizes = [len(s) for s in o.sets]
    assert all(n == q or n >= q + 2 for n in sizes) and sizes.count(q) >= 2 and sum(n >= q + 2 for n in sizes) >= 2, sizes
    hit, clean = _mixed_points(o, r)
    home, regs, _ = o.plan(r)
    through = [j for j in clean if any(len(o.sets[int(p)]) == q for p in regs[j])]
    assert len(hit) >= 3 and len(clean) >= 3 and len(through) >= 1      # a clean point with a non-member item at n == q
    ry, rv = _multi_ratios(o, r, clean)
    print("mixed: sizes", sizes, "clean", clean, "ratios", ry, rv)
    assert ry <= 1.0 and rv <= 1.0, (ry, rv)


# ------------------------------------------------------------------------------------ item counts
def test_item_count_workloads():
    for N in EC.COUNT_NS:
        o = EC.count_oracle(N)
        r0 = EC.radius_with_no_neighbours(o)
        assert o.counts(r0) == (N, 0, 0, 0)
        assert (r0 == 0.0) == (N == 257)          # an odd split puts its plane through a point: see the helper
    o = EC.count_oracle(256)
    r1 = EC.radius_with_one_non_member(o, EC.radius_with_no_neighbours(o))
    assert o.counts(r1)[:2] == (257, 1)
    # N = 257: the two median points come at every positive radius, there is no radius with exactly one
    o = EC.count_oracle(257)
    assert EC.radius_with_one_non_member(o, 0.0) is None and o.counts(1e-9)[:2] == (259, 2)
    for N, r in ((256, r1), (257, 1e-9)):
        for trend in (None, "linear"):
            ry, rv = _multi_ratios(EC.count_oracle(N, trend), r)
            assert ry <= 1.0 and rv <= 1.0, (N, trend, ry, rv)


# ------------------------------------------------------------------------------------ buffer growth
def test_the_growth_plan_exceeds_the_reservation_slack():
    o = EC.grow_oracle()
    ts, ss = o.counts(EC.GROW["small"])[:2]
    tl, sl = o.counts(EC.GROW["large"])[:2]
    assert ts <= len(o.X) + 64                                # close to N
    assert tl > ts + EC.reserve_slack(ts) and sl - ss > EC.reserve_slack(ts), (ts, ss, tl, sl)


# ------------------------------------------------------------------------------------ duplicated points
@pytest.mark.parametrize("trend", [None, "linear"])
def test_duplicated_points(trend):
    o = EC.dup_oracle(trend)
    c = EC.DUP
    h = c["N"] // 2
    for k in range(c["pairs"]):
        assert np.array_equal(o.X[k], o.X[h + k]) and o.Y[k, 0] != o.Y[h + k, 0]
        shared = [p for p in range(o.P) if o.row_of(p, k) >= 0]
        assert shared and all(o.row_of(p, h + k) >= 0 and o.row_of(p, h + k) != o.row_of(p, k) for p in shared)
    if trend is None:
        ry, rv = _single_ratios(o, c["radius"])
        assert ry <= 1.0 and rv <= 1.0, (ry, rv)
    ry, rv = _multi_ratios(o, c["radius"])
    print("duplicates", trend, "cond2 %.4g" % o.cond2(), ry, rv)
    assert ry <= 1.0 and rv <= 1.0, (ry, rv)
