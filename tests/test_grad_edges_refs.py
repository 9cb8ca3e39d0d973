"""The workloads of tests/test_gpu_grad_edges.py, checked on the CPU (no device compute): every workload of
tests/_grad_edge_cases.py has, by the oracle, the property its GPU test relies on, so that a failure of the GPU module is a
property of the device code and not of its inputs.  And tests/_grad_refs.py (mix_grad_ref) is pinned for the seven blending
profiles of group A, by the central-difference test of tests/test_grad_refs.py, before it judges the device.

What the tree allows.  A neighbour item is accepted at a hyperplane only if a step of delta across the plane, from the
projection of the query onto it, leaves or enters the home leaf: the plane bounds the home leaf.  On scattered points these
are ancestor planes of the leaf whose foot point happens to lie on the leaf's own face, so a query of the random workloads
has at most levels - 1 neighbours (asserted below) and far fewer in practice: D = 3 at levels 5 cannot exceed 4, and group C
uses levels 7, where the wide radius gives 6 (m = 7), more than the PLAN_STAGE = 4 the fill pass copies.  Queries of m >= 12
items come from a point set built so that all 11 ancestor planes of one leaf form a polygon round it (polygon_points).
"""
import numpy as np
import pytest

from oracle import oracle as O

import _grad_refs as GR
import _grad_edge_cases as EC
import test_grad_refs as TGR


# ------------------------------------------------------------------------------------ A. weight families
@pytest.mark.parametrize("name", ["base2", "base3"])
def test_weight_family_workloads(name):
    wl = EC.workload(name)
    r = EC.A_RADIUS[wl.D]
    plan = wl.plan()
    ts = np.concatenate([s[3] for s in plan])
    assert len(ts) >= 40                                            # neighbour items
    assert np.all(np.abs(ts) < r)
    for wname, (_, owth) in EC.weight_kernels(r).items():
        w = np.array([O.profile(owth, abs(t)) for t in ts])
        assert np.all(w >= 0.0), wname                              # no negative weight: S >= 1 (the home weight) ...
        for s in plan:
            assert 1.0 + sum(O.profile(owth, abs(t)) for t in s[3]) >= 1.0, wname
        if wname == "modsqexp":
            assert np.all(np.cos(owth.p[1] * np.abs(ts)) > 0)       # ... for ModSqExp because cos(p1 |t|) > 0 on |t| < r
        if wname == "spline34_narrow":
            assert np.any(w == 0.0) and np.any(w > 0.0)             # an accepted neighbour with a weight of exactly 0
        if wname == "trq":
            assert abs(O.profile(owth, 0.0) - 0.7) <= 1e-15             # w(0) = p1 != 1, the home weight stays 1
    pick, with_nb = wl.stable_pick(EC.has_neighbours)
    assert len(pick) == 16 and with_nb >= 4


@pytest.mark.parametrize("wname", list(EC.weight_kernels(1.0)))
def test_mix_grad_ref_equals_central_differences_of_the_oracle_for_every_weight_family(wname):
    """tests/test_grad_refs.py::test_analytic_gradient_equals_central_differences_of_the_oracle with the blending profile
    replaced (its workload's radius is 1): one model family, the linear trend for every second profile"""
    wl = TGR.Workload()
    wl.wth = EC.weight_kernels(TGR.RADIUS)[wname][1]
    trend = list(EC.weight_kernels(1.0)).index(wname) % 2 == 1      # the trend changes the items, not the weights
    TGR.test_analytic_gradient_equals_central_differences_of_the_oracle(wl, "spline34", trend)


def test_psi_of_the_weight_kernels_is_the_derivative_of_the_oracle_profile():
    for r in EC.A_RADIUS.values():
        for wname, (_, owth) in EC.weight_kernels(r).items():
            lip = max(1.0, GR.lip(owth))
            for tau in np.linspace(0.02 * r, 0.98 * r, 25):
                h = 1e-6 * r
                fd = (O.profile(owth, tau + h) - O.profile(owth, tau - h)) / (2 * h)
                assert abs(fd - float(GR.psi(owth, np.float64(tau))) * tau) <= 2e-8 * lip, (wname, tau)


# ------------------------------------------------------------------------------------ B. larger trees
@pytest.mark.parametrize("name", list(EC.DEEP))
def test_deep_tree_workloads(name):
    wl = EC.workload(name)
    D, levels, _ = EC.DEEP[name]
    assert wl.ob.P == wl.P == 2 ** (levels - 1) and len(wl.hp_c) == wl.P - 1
    plan = wl.plan()
    planes = np.concatenate([np.array(s[2], dtype=np.int64) for s in plan])
    assert len(planes) >= 40
    assert planes.max() >= 32                                       # a mask word beyond the first (w >= 1)
    if levels >= 10:
        assert planes.max() >= 256                                  # a chunk beyond the first (c0 = 256)
    if levels == 12:
        assert wl.P - 1 == EC.PLAN_LDS_NODES                        # the largest tree staged in LDS
    if levels == 13:
        assert wl.P - 1 > EC.PLAN_LDS_NODES                         # plan_kernel<D, *, LDS = false>
    for s in plan:                                                  # neighbours in hyperplane order, one region each
        assert list(s[2]) == sorted(s[2]) and len(s[1]) == len(s[2]) <= levels - 1
    if name in ("L7", "L7_D4"):
        pick, deep = wl.stable_pick(EC.has_deep_plane)
        assert len(pick) == 16 and deep >= 4                        # the numeric gradient depends on a plane of index >= 32


def test_the_oracles_hyperplanes_are_the_hosts():
    for name in ("base2", "L7", "L10", "many"):
        wl = EC.workload(name)
        v, c = wl.ob.hyperplanes()
        assert np.array_equal(v, wl.hp_v) and np.array_equal(c, wl.hp_c)


# ------------------------------------------------------------------------------------ C. many neighbours
def test_many_neighbour_workload():
    wl = EC.workload("many")
    mid, wide = wl.counts(EC.C_RADII["mid"]), wl.counts(EC.C_RADII["wide"])
    assert EC.C_RADII["wide"] > wl.width
    assert mid.max() > EC.PLAN_STAGE and wide.max() > EC.PLAN_STAGE
    assert wide.max() + 1 >= 7 and wide.max() <= wl.levels - 1      # the most items a query of this tree gets (see above)
    # and the queries of 12 and more items: a radius wider than the box, every query accepted at 11 planes or more
    poly = EC.workload("polygon")
    assert poly.radius > poly.width and poly.levels == 12 and all(len(x) == 4 for x in poly.Xs)
    m = poly.counts() + 1
    assert m.max() >= 12 and m.min() >= 12, (m.min(), m.max())
    assert all(set(range(11)) <= set(s[2]) for s in poly.plan())    # the 11 ancestors of the home leaf, pre-order 0..10
    ts = np.concatenate([s[3] for s in poly.plan()])
    assert np.all(np.abs(ts) < 1.1) and O.profile(EC.spline34_weight(poly.radius)[1], 1.1) > 0.5
    assert np.mean(wide) > 3
    a, b, heavy, light = EC.reorderings(wl)
    assert len(heavy) >= 1 and len(light) >= 256
    assert mid[a[:256]].max() > EC.PLAN_STAGE                       # order A: block 0 walks the planes again
    assert mid[b[:256]].max() <= EC.PLAN_STAGE                      # order B: block 0 copies its staged hits
    assert len(set(a[:256]) & set(b[:256])) >= 100                  # the queries both block 0s share
    assert sorted(a) == sorted(b) == list(range(len(wl.Xq)))


# ------------------------------------------------------------------------------------ D. exact t
def test_query_on_the_plane():
    wl = EC.workload("on_plane")
    assert len(wl.X) % 2 == 1 and wl.P == 2
    x0 = wl.Xq[0]
    assert np.any(np.all(wl.X == x0, axis=1))                       # the median training point
    home, reg, planes, ts = wl.signature(x0)
    assert planes == (0,) and len(reg) == 1 and reg[0] != home
    assert ts[0] == 0.0 and wl.hp_c[0] - wl.hp_v[0, 0] * x0[0] == 0.0
    assert O.profile(EC.spline34_weight(wl.radius)[1], 0.0) == 1.0
    assert abs(O.profile(EC.weight_kernels(wl.radius)["trq"][1], 0.0) - 0.7) <= 1e-15


def test_training_points_as_queries():
    grid, dups = EC.workload("grid"), EC.workload("dups")
    for wl in (grid, dups):
        assert all(np.any(np.all(wl.X == x, axis=1)) for x in wl.Xq[:50])
        assert wl.counts().sum() >= 40
    exact = lambda wl: sum(1 for s in wl.plan() if len(s[3]) and np.abs(s[3]).min() < 1e-12)
    assert exact(grid) >= 10
    # the duplicated set: twins, and triplets of the points that the planes pass through
    assert exact(dups) >= 10
    _, cnt = np.unique(dups.X, axis=0, return_counts=True)
    assert (cnt == 2).sum() >= 15 and (cnt == 3).sum() >= 3
    copies = [i for i in range(len(dups.X)) if np.sum(np.all(dups.X == dups.X[i], axis=1)) >= 2]
    assert sum(1 for i in copies if len(dups.plan()[i][1])) >= 10   # duplicated points with neighbour items


def test_extreme_radii():
    wl = EC.workload("base2")
    assert np.all(wl.counts(0.0) == 0)
    huge = wl.counts(EC.HUGE_RADII[0])
    assert huge.sum() > wl.counts().sum() and huge.sum() >= 300    # every ancestor plane passes the distance test
    for r in EC.HUGE_RADII[1:]:
        assert np.array_equal(wl.counts(r), huge)


# ------------------------------------------------------------------------------------ E, F
def test_ranges_and_buffer_workloads():
    assert [EC.range_chain(n) for n in EC.E_NQ] == [[(0, 1)], [(0, 100), (100, 255)], [(0, 100), (100, 256)],
                                                    [(0, 100), (100, 257)], [(0, 100), (100, 257), (257, 513)]]
    wl = EC.workload("base2")
    for n in EC.E_NQ:
        Xq = wl.queries(n)
        assert Xq.shape == (n, 2)
    assert sum(len(s[1]) for s in wl.plan(Xq=wl.queries(513))) >= 100
    small, large = wl.counts(EC.F_RADII["small"]).sum(), wl.counts(EC.F_RADII["large"]).sum()
    # the plan of the large radius outgrows the gradient buffer of the small one at R = 1, and R = 16 outgrows both
    assert (len(wl.Xq) + large) > (len(wl.Xq) + small) and large >= 10 * max(small, 1)


def test_fp32_stencil_at_the_wider_spacing():
    """h = 2^-10 of the width: the stencil of a float32 query consists of float32 numbers, and 16 queries are stable"""
    wl = EC.workload("base2_f32")
    Xq32 = Xq = wl.Xq.astype(np.float32).astype(np.float64)
    h = wl.width * 2.0 ** -10
    pick, with_nb = wl.stable_pick(EC.has_neighbours, Xq=Xq32, h=h)
    assert len(pick) == 16 and with_nb >= 4
    for x in Xq32[pick]:
        for p in wl.stencil(x, h):
            assert np.array_equal(p, p.astype(np.float32).astype(np.float64))
