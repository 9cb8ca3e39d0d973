"""The inputs of tests/test_gpu_cov_edges.py, checked on the CPU (no device compute): every input of
tests/_cov_edge_cases.py has the property its GPU test relies on, so that a failure of the GPU module is a property of the
device code and not of its inputs.

  A. the schedule: cov_tasks_from_plan and slots = min(ntasks, ncu) restated; for chips of 64, 256 and 304 compute units
     there are at least 2 ncu + 3 tasks, and some workgroup runs a patch of nt >= 5 and then one of nt = 1, the other way
     round, a full strip and then a strip of one item, the other way round, and two patches whose nt differ in parity; a
     sub-query of the bits check has fewer tasks than the smallest chip has compute units;
  B. the block rows and last-row pairs of the eight patches, the item counts on the wave, piece and strip boundaries;
  C. the items of the blend inputs (from the oracle's plan): 12 and more per query, more neighbours than PLAN_STAGE, t == 0,
     the twins of the duplicated points;
  D. the doubled corner queries of the draws;
  and for every input with a reference: kappa2(L) <= 10^3, and a plain numpy / LAPACK evaluation of the block in the
  model's own precision stays below one error unit of tests/_cov_refs.py -- the check of tests/test_cov_refs.py.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import _cov_cases as CC
import _cov_edge_cases as CE
import _cov_refs as CR
import _grad_edge_cases as EC

_REFS = {}


def _ref(key, oth, X, sigma2):
    if key not in _REFS:
        _REFS[key] = CR.RegionRef(oth, X, sigma2)
    return _REFS[key]


def grouped_cov(ref, pts_list):
    """RegionRef.cov of several item lists of one patch (or of patches that share their points) with one substitution: the
    diagonal blocks of the covariance of all the points together -> list of dict(S, unit, clamped)"""
    out = ref.cov(np.vstack(pts_list))
    cut = np.concatenate([[0], np.cumsum([len(p) for p in pts_list])])
    return [dict(S=out["S"][a:b, a:b], unit=out["unit"][a:b, a:b], clamped=out["clamped"][a:b]) for a, b in zip(cut[:-1], cut[1:])]


def plain_worst(blocks, dtype):
    """blocks: iterable of (reference, patch points, item points) -> (worst err / unit of the plain evaluation, largest
    kappa2(L))"""
    T_, u = (np.float32, 2.0 ** -24) if dtype == "f32" else (np.float64, 2.0 ** -53)
    worst = kappa = 0.0
    for ref, X, pts in blocks:
        out = ref.cov(pts)
        assert not out["clamped"].any()
        plain = CR.plain_region_cov(ref.th, X, CC.SIGMA2[dtype], pts, T_)
        err = np.abs(plain - out["S"]).astype(np.float64)
        worst = max(worst, float((err / ((len(X) + 32) * u * out["unit"])).max()))
        kappa = max(kappa, ref.kappa)
    return worst, kappa


# ------------------------------------------------------------------------------------ A. several strips per workgroup
def test_the_restated_tasks_deal_a_regions_items_evenly():
    region, items = CE.cov_tasks([255, 1, 256, 257, 513, 0, 3, 17, 512])
    assert list(region) == [0, 1, 2, 3, 3, 4, 4, 4, 6, 7, 8, 8]
    assert list(items) == [255, 1, 256, 129, 128, 171, 171, 171, 3, 17, 256, 256]


def test_the_classes_of_the_schedule_patches():
    sizes, counts = CE.a_sizes(), CE.a_counts()
    assert len(sizes) == CE.A_P == 2 ** (CE.A_LEVELS - 1)
    assert sorted(set(sizes)) == [1, 7, 40, 90, 128, 129, 257, 300, 641]
    assert sizes.count(641) == 16 and sizes.count(90) == 112 and all(sizes.count(n) == 128 for n in (1, 7, 40, 128, 129, 257, 300))
    assert sorted({CE.block_rows(n) for n in sizes}) == [1, 2, 3, 6]
    # the regions a workgroup of 64, 256 or 304 runs one after the other differ in class and in point set
    for d in CE.A_NCU:
        assert all(CE.a_class(r) != CE.a_class(r + d) and CE.a_variant(r) != CE.a_variant(r + d) for r in range(CE.A_P - d))
    assert len({CE.a_set_key(r, sizes) for r in range(CE.A_P)}) == 9 * CE.A_VARIANTS
    assert sorted(CE.A_HEAVY.values()) == [256, 256, 256, 257, 257, 513, 513] and sum(counts) < 16384 // 4
    heavy_nt = {CE.block_rows(sizes[r]) for r in CE.A_HEAVY}
    assert heavy_nt == {1, 2, 3, 6}                                  # a full strip on six block rows among them
    assert sizes[411] == 641 and counts[411] == 256
    checked = CE.a_checked_regions()
    assert all(r in checked for r in range(CE.A_P) if CE.block_rows(sizes[r]) >= 2) and all(r in checked for r in range(0, CE.A_P, 8))


@pytest.mark.parametrize("ncu", CE.A_NCU)
def test_some_workgroup_runs_tasks_of_every_kind_one_after_the_other(ncu):
    sizes, counts = CE.a_sizes(), CE.a_counts()
    s = CE.schedule(counts, sizes, ncu)
    print("COVEDGESCHED", ncu, s)
    assert s["ntasks"] >= 2 * ncu + 3 and s["slots"] == ncu, s
    assert s["deep_to_one"] >= 1 and s["one_to_deep"] >= 1, s
    assert s["full_to_single"] >= 1 and s["single_to_full"] >= 1, s
    assert s["parity"] >= 1, s
    assert CE.schedule_ok(s, ncu)
    # a sub-query of the bits check: every workgroup of the smallest chip has one task
    region, _ = CE.cov_tasks(counts)
    for lo, hi in CE.a_pieces():
        assert ((region >= lo) & (region < hi)).sum() <= min(CE.A_NCU)
    # without the task loop: the largest case of tests/test_gpu_cov.py with explicit items stays below the smallest chip
    assert CE.schedule(CC.EDGE_COUNTS, CC.EDGE_SIZES, 64)["most_tasks"] == 1


def a_region_groups(sizes):
    """the checked regions of group A by point set: one long-double factor serves a group"""
    groups = {}
    for r in CE.a_checked_regions():
        groups.setdefault(CE.a_set_key(r, sizes), []).append(r)
    return groups


@pytest.mark.parametrize("D,dtype,mixed", CE.A_CASES)
def test_a_plain_evaluation_stays_below_one_unit_on_the_schedule_inputs(D, dtype, mixed):
    Xs, sizes = CE.a_patches(D, dtype), CE.a_sizes()
    xq, region = CE.a_items(D, dtype)
    assert [len(X) for X in Xs] == sizes and np.array_equal(np.bincount(region, minlength=CE.A_P), CE.a_counts())

    T_, u = (np.float32, 2.0 ** -24) if dtype == "f32" else (np.float64, 2.0 ** -53)
    worst = kappa = 0.0
    for key, regs in a_region_groups(sizes).items():
        ref = _ref(("A", D, dtype, mixed) + key, CC.FAMILIES[CE.a_family(key, mixed)][1], Xs[regs[0]], CC.SIGMA2[dtype])
        kappa = max(kappa, ref.kappa)
        for r, out in zip(regs, grouped_cov(ref, [xq[region == r] for r in regs])):
            assert not out["clamped"].any()
            plain = CR.plain_region_cov(ref.th, Xs[r], CC.SIGMA2[dtype], xq[region == r], T_)
            err = np.abs(plain - out["S"]).astype(np.float64)
            worst = max(worst, float((err / ((sizes[r] + 32) * u * out["unit"])).max()))
    print("COVEDGEUNIT A D=%d dtype=%s mixed=%s plain worst err/unit=%.3g kappa2(L)=%.3g" % (D, dtype, mixed, worst, kappa))
    assert worst < 1.0 and kappa <= CC.KAPPA_MAX, (worst, kappa)


# ------------------------------------------------------------------------------------ B. depth, dimension, strip counts
def test_block_rows_pairs_and_counts_of_the_deep_patches():
    assert [CE.block_rows(n) for n in CE.B_SIZES] == CE.B_NT == [5, 6, 6, 7, 7, 7, 1, 1]
    assert [CE.last_pairs(n) for n in CE.B_SIZES] == CE.B_PAIRS == [1, 1, 2, 3, 4, 4, 2, 2]
    # the first pair exactly full (672 = 5 x 128 + 32), the last pair exactly full (896 = 7 x 128), each once
    assert [n % 128 for n in CE.B_SIZES].count(32) == 1 and [n % 128 for n in CE.B_SIZES].count(0) == 1
    assert CE.B_COUNTS == [31, 32, 33, 63, 64, 65, 512, 96]
    region, items = CE.cov_tasks(CE.B_COUNTS)
    assert list(items[region == CE.B_TWO_STRIPS]) == [256, 256] and len(region) == 9
    # none of this is in the inputs of tests/test_gpu_cov.py
    assert max(CE.block_rows(n) for n in CC.EDGE_SIZES) == 3 and not set(CE.B_COUNTS[:7]) & set(CC.EDGE_COUNTS)


@pytest.mark.parametrize("D,dtype,family", CE.B_CASES)
def test_a_plain_evaluation_stays_below_one_unit_on_the_deep_patches(D, dtype, family):
    Xs = CE.b_patches(D, dtype)
    xq, region = CE.b_items(D, dtype)
    assert [len(X) for X in Xs] == CE.B_SIZES and list(np.bincount(region, minlength=8)) == CE.B_COUNTS
    oth = CC.FAMILIES[family][1]
    worst, kappa = plain_worst(((_ref(("B", D, dtype, family, r), oth, Xs[r], CC.SIGMA2[dtype]), Xs[r], xq[region == r])
                                for r in range(8)), dtype)
    print("COVEDGEUNIT B D=%d dtype=%s family=%s plain worst err/unit=%.3g kappa2(L)=%.3g" % (D, dtype, family, worst, kappa))
    assert worst < 1.0 and kappa <= CC.KAPPA_MAX, (worst, kappa)


# ------------------------------------------------------------------------------------ C. the blend
def _oracle_blocks(wl, radius=None, Xq=None):
    plan = wl.plan(radius, Xq)
    items = CE.plan_items(plan)
    pts = CC.rnd(wl.Xq if Xq is None else Xq, wl.dtype)
    return items, CC.blocks_of(items, pts)


def _plain_on(wl, blocks, key):
    return plain_worst(((_ref((key, r), wl.oth, wl.Xs[r], CC.SIGMA2[wl.dtype]), wl.Xs[r], pts) for r, (_, pts) in blocks.items()),
                       wl.dtype)


@pytest.mark.parametrize("name", ["base2"] + sorted(CE.C_INPUTS))
def test_a_plain_evaluation_stays_below_one_unit_on_the_blend_inputs(name):
    wname, radius = CE.C_INPUTS.get(name, ("base2", None))
    wl = EC.workload(wname)
    items, blocks = _oracle_blocks(wl, radius)
    per_query = np.diff(items[0])
    if name == "polygon":
        assert per_query.min() >= 12 and len(wl.Xs) == 2048 and len(wl.Xq) == 48
    if name.startswith("many"):
        assert per_query.max() - 1 > EC.PLAN_STAGE
    if name == "L7_D4":
        assert wl.D == 4 and len(wl.Xs) == 64 and (per_query > 1).sum() >= 40
    if name == "on_plane":
        assert per_query[0] == 2 and items[2][0] == 0.0              # query 0 sits on the plane: t == 0
    if name == "grid":
        assert all(any(np.array_equal(x, p) for p in wl.X) for x in wl.Xq[:8])
    if name == "radius_0":
        assert np.all(per_query == 1)
    if name == "radius_1e300":
        assert items[0][-1] - len(wl.Xq) >= 300
    if name == "base2_f32":
        assert wl.dtype == "f32"
    worst, kappa = _plain_on(wl, blocks, ("C", wname))
    print("COVEDGEUNIT C %s plain worst err/unit=%.3g kappa2(L)=%.3g regions=%d" % (name, worst, kappa, len(blocks)))
    assert worst < 1.0 and kappa <= CC.KAPPA_MAX, (worst, kappa)


def test_the_twins_among_the_duplicated_points():
    wl = EC.workload("dups")
    assert np.array_equal(wl.Xq, wl.X)                               # every training point is a query
    groups = CE.twin_groups(wl.Xq)
    assert all(np.array_equal(wl.Xq[g[0]], wl.Xq[j]) for g in groups for j in g[1:])
    pairs = {(g[0], j) for g in groups for j in g[1:]}
    assert all((i, 120 + i) in pairs for i in range(20))             # the 20 twins the workload writes first
    assert any(len(g) >= 3 for g in groups)                          # and the triplets on the planes
    twins = sorted(j for g in groups for j in g)
    assert 40 <= len(twins) < len(wl.Xq)
    # twins have the same items: home, neighbours and t
    plan = wl.plan()
    for g in groups:
        for j in g[1:]:
            assert plan[j][:3] == plan[g[0]][:3] and np.array_equal(plan[j][3], plan[g[0]][3])


def test_the_prefixes_of_the_batch_keep_their_order():
    assert CE.C_NQ_EDGES == [1, 15, 16, 17, 33] and max(CE.C_NQ_EDGES) < len(EC.workload("base2").Xq)


# ------------------------------------------------------------------------------------ D. draws
def test_the_doubled_corner_queries_share_regions_and_stay_below_one_unit():
    m = CC.Main("f64")
    X8 = CE.corner_queries(m)
    Xq = np.vstack([X8, X8])
    assert CE.twin_groups(Xq) == [[j, j + 8] for j in range(8)]
    w = SimpleNamespace(X=m.X, LEVELS=m.LEVELS, Xq=Xq, RADIUS=m.RADIUS, DELTA=m.DELTA)
    items = CC.oracle_items(w)
    shared = CR.shared_region_mask(items[:2])
    assert (shared & ~np.eye(16, dtype=bool)).sum() >= 2 * 20 + 16
    oth = CC.FAMILIES["spline34"][1]
    worst, kappa = plain_worst(((_ref(("D", r), oth, m.Xs[r], CC.SIGMA2["f64"]), m.Xs[r], pts)
                                for r, (_, pts) in CC.blocks_of(items, Xq).items()), "f64")
    print("COVEDGEUNIT D plain worst err/unit=%.3g kappa2(L)=%.3g" % (worst, kappa))
    assert worst < 1.0 and kappa <= CC.KAPPA_MAX, (worst, kappa)


def test_the_jitter_ladder():
    lad = CE.jitter_ladder(3.0)
    assert lad[0] == 0.0 and lad[1] == 2.0 ** -52 * 3.0 and all(b == 10.0 * a for a, b in zip(lad[1:-1], lad[2:]))
    assert lad[-1] <= 2.0 ** -26 * 3.0 < 10.0 * lad[-1] and len(lad) == 9
