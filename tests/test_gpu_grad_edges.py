"""The gradient of the blended mean on the GPU at its edges (mix_grad_kernel of pmk_grad.hip, the item_plane output of
plan_kernel, the capacity-grown buffers of pmk_query_items_grad / pmk_query_mix_grad), on the workloads of
tests/_grad_edge_cases.py; tests/test_grad_edges_refs.py asserts on the CPU what each workload was chosen for.

  A. every stationary family as the BLENDING profile (Spline12, Spline32, Gaussian, RQ, TRQ with w(0) = 0.7, ModSqExp also
     at D = 3, a Spline34 narrower than the plan radius: accepted neighbours of weight exactly 0);
  B. item_plane on trees of 63, 511, 2047 and 4095 planes (mask words beyond the first, chunks beyond the first, the largest
     tree staged in LDS, the tree read from global memory), D = 2 and D = 4;
  C. queries with more than PLAN_STAGE neighbours (the fill pass walks the planes again) and the O(m^2) loop of the blend,
     up to queries of 12 and 14 items on a point set built for it;
  D. t == 0 exactly, training points of gridded and duplicated sets as queries, plan radii 0, 1e150 and 1e300;
  E. query ranges that tile [0, Nq) off the 256-thread blocks, empty ranges, rows outside a range;
  F. re-plans and a change of R on one query (d_gm and d_dyq grow by capacity);
  G. variance=True before the gradient, per-patch mixed families and sigma2 in a planned blend (fp64 and fp32), an fp32 model.

Bounds, all those of tests/test_gpu_grad.py, through its helpers (_item_ratios, _worst_ratio, _fd_ratio):
  items    |err| <= (n + 32) u lip(theta) sum_k |C[k, c]| against item_grad_ref with the device's own weights;
  blend    |err| <= 16 m 2^-53 mag against mix_grad_ref fed with the device's own items and the case's weight kernel;
  fd       central differences of pmk_predict_mixture_multi_fitted, h = 2^-17 of the domain width, tolerance
           |fd_2h - fd_h| + 2 eps_f / h, on 16 queries whose item signature is constant over the stencil;
  bits     np.array_equal on the uint64 views wherever a test says "bit for bit".
The fp32 model takes the fd rule with u = 2^-24 at h = 2^-10 of the width.  2 eps_f / h falls as 1 / h: at 2^-17 it is 1.2
times the gradient itself (recorded as fd_tolerance_over_gradient_at_2^-17) and nothing could fail; 2^7 times the spacing
brings it to about a hundredth of the gradient, the truncation term |fd_2h - fd_h| of the rule grows with h^2 by itself, and
h is still a power of two, so that the stencil of a float32 query consists of float32 numbers.  The test asserts that the
tolerance is below a tenth of the gradient before it applies it.

Every measured ratio err / bound is printed ("GRADEDGE {json}", run with -s); a run of the whole module writes them to
profiles/grad_edges_accuracy.json.
"""
import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import mixture as M

import _grad_refs as GR
import _grad_edge_cases as EC
from test_gpu_grad import FAMILIES, SIGMA2, U_OF, Blend, _fd_ratio, _item_ratios, _plane_t, _round, _worst_ratio

pytestmark = pytest.mark.gpu

_RECORDS = []
TESTS = {"weight_family", "planes", "deep_tree", "many_items", "twelve_items", "staged_vs_walk", "on_plane", "training_points", "huge_radius",
         "ranges", "buffer_lifetime", "mixed_families", "fp32_model"}
ACCURACY_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "grad_edges_accuracy.json")


def _record(**kw):
    _RECORDS.append(kw)
    print("GRADEDGE " + json.dumps(kw, sort_keys=True))


@pytest.fixture(scope="module", autouse=True)
def _write_accuracy_file():
    """only a run of the whole module replaces the file"""
    yield
    if {r["test"] for r in _RECORDS} >= TESTS:
        with open(ACCURACY_JSON, "w") as f:
            f.write("[\n" + ",\n".join(" " + json.dumps(r, sort_keys=True) for r in _RECORDS) + "\n]\n")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------ the device side of a workload
class Dev:
    """a multi-output model of a workload, fitted as test_gpu_grad.Blend fits its own (fit=False: the tree alone);
    thetas / sigma2s: per-patch kernels and noise through fit_patches"""

    def __init__(self, wl, R=None, dtype=None, thetas=None, sigma2s=None, fit=True):
        self.wl, self.R, self.dtype = wl, wl.R if R is None else R, dtype or wl.dtype
        Ys = wl.Ys(self.R)
        self.model = M.DeviceModel(wl.Xs, [np.ascontiguousarray(y[:, 0]) for y in Ys], dtype=self.dtype)
        self.own = thetas is not None
        self.oths = [FAMILIES[n][1] for n in thetas] if self.own else [wl.oth] * len(wl.Xs)
        if fit:
            if self.own:
                self.model.fit_patches([FAMILIES[n][0] for n in thetas], sigma2s)
            else:
                self.model.fit(wl.th, SIGMA2[self.dtype])
            self.solve(Ys)
            assert np.all(self.model.info() == 0)
        self.model.set_bsp(wl.root, 0)

    def solve(self, Ys):
        self.model.set_targets_multi(Ys)
        self.model.set_trend(self.wl.trend)
        self.model.solve_multi()

    def items(self, q, variance=False):
        if self.own:
            q.items_multi_fitted(variance)
            q.items_grad()
        else:
            q.items_multi(self.wl.th, variance)
            q.items_grad(self.wl.th)

    def run(self, wth, Xq=None, radius=None, variance=False):
        q = M.DeviceQuery(self.model, self.wl.Xq if Xq is None else Xq)
        q.plan(self.wl.radius if radius is None else radius, self.wl.delta)
        self.items(q, variance)
        q.mix_multi(wth)
        q.mix_grad(wth)
        return q


_DEVS = {}


def _dev(name, **kw):
    key = (name, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _DEVS:
        _DEVS[key] = Dev(EC.workload(name), **kw)
    return _DEVS[key]


def check_planes(wl, q, Xq, plan):
    """homes, regions, planes and t of every query against the oracle's plan: the planes np.nonzero(keep) in order, the home
    item last with plane -1, t equal to the oracle's and to c - v . x of the plane, bit for bit -> (plane, debug())"""
    dbg = q.debug()
    plane = q.item_grads()[1]
    off, t, reg = dbg["item_offsets"], dbg["item_t"], dbg["item_region"]
    assert len(plan) == len(Xq) == q.Nq and off[-1] == q.total == len(plane)
    dot_mode = pmk.lib().pmk_bsp_dot_mode(M._native(wl.root).h)
    for j, (home, regs, planes, ts) in enumerate(plan):
        b, e = off[j], off[j + 1]
        assert dbg["home"][j] == home, j
        assert list(plane[b:e]) == list(planes) + [-1], (j, plane[b:e], planes)
        assert list(reg[b:e]) == list(regs) + [home], j
        assert same_bits(t[b:e - 1], ts) and t[e - 1] == 0.0, j
        for k, p in enumerate(planes):
            assert _plane_t(wl.hp_v[p], wl.hp_c[p], Xq[j], dot_mode) == t[b + k], (j, p)
    return plane, dbg


def blend_ratio(q, hp_v, owth):
    """worst err / bound of fetch_grad against mix_grad_ref fed with the device's own items -> (ratio, largest m, neighbour
    items)"""
    dY = q.fetch_grad()
    U, _ = q.item_values_multi()
    G, plane = q.item_grads()
    dbg = q.debug()
    off, t = dbg["item_offsets"], dbg["item_t"]
    assert np.all(np.isfinite(dY))
    worst = 0.0
    for j in range(q.Nq):
        items = range(off[j], off[j + 1])
        ref, mag = GR.mix_grad_ref(items, G, U, t, plane, hp_v, owth)
        bound = 16 * len(items) * 2.0 ** -53 * mag.astype(np.float64)
        err = np.abs(np.asarray(dY[j], dtype=GR.LD) - ref).astype(np.float64)
        worst = max(worst, _worst_ratio(err, bound))
    return worst, int(np.diff(off).max()), int(off[-1] - q.Nq)


def item_ratio(dev, q, Xq):
    """worst err / bound of item_grads against item_grad_ref with the device's own weights"""
    wl, model = dev.wl, dev.model
    G, _ = q.item_grads()
    dbg = q.debug()
    item_q = np.repeat(np.arange(q.Nq), np.diff(dbg["item_offsets"]))
    P = len(wl.Xs)
    tinfo = model.trend_info() if wl.trend else np.zeros(P, dtype=np.int32)
    betas = model.trend()[0] if wl.trend == "linear" else [None] * P
    return _item_ratios(G, _round(np.asarray(Xq), dev.dtype)[item_q], dbg["item_region"], wl.Xs, model.weights_multi(), dev.oths,
                        betas, tinfo, U_OF[dev.dtype])


def fd_ratio(dev, wth, Xc, dY, radius=None, u=2.0 ** -53, h=None, check=True):
    """test_gpu_grad._fd_ratio on the queries Xc of a workload (stable over the stencil by the caller's choice), with the
    kernel of each patch in eps_f -> (worst err / tol, median tol / max |dY| per query)"""
    wl = dev.wl
    radius = wl.radius if radius is None else radius
    h = wl.width * 2.0 ** -17 if h is None else h
    b = SimpleNamespace(wth=wth, model=dev.model, radius=radius, delta=wl.delta, R=dev.R)
    return _fd_ratio(b, wl.trend, Xc, lambda x: wl.stencil(x, h), [wl.signature(x, radius)[:2] for x in Xc], dY, h, dev.oths,
                     wl.Xs, u, check)


def fd_on_stable_queries(dev, wth, pred, radius=None):
    """16 stencil-stable queries of the workload, at least 4 of which satisfy pred -> (ratio, how many do); the ratio is
    returned unasserted so that the caller records it first"""
    pick, n_pred = dev.wl.stable_pick(pred, radius)
    assert len(pick) == 16 and n_pred >= 4
    Xc = dev.wl.Xq[pick]
    q = dev.run(wth, Xc, radius)
    return fd_ratio(dev, wth, Xc, q.fetch_grad(), radius, check=False)[0], n_pred


def same_nan_pattern(q, R):
    """per (query, column): the gradient is NaN exactly where the mean is"""
    Y, dY = q.fetch_multi(R)[0], q.fetch_grad()
    nan = np.isnan(dY)
    assert np.array_equal(nan.all(2), nan.any(2))
    return np.array_equal(nan.any(2), np.isnan(Y))


# ------------------------------------------------------------------------------------------ A. weight families
def test_the_base_workloads_are_those_of_the_blend_tests():
    for name in ("base2", "base3"):
        wl = EC.workload(name)
        b = Blend(wl.D, wl.R, "spline34", None, radius=wl.radius)
        assert np.array_equal(b.X, wl.X) and np.array_equal(b.Xq, wl.Xq) and b.delta == wl.delta and b.levels == wl.levels
        assert len(b.Xs) == len(wl.Xs) and all(np.array_equal(x, y) for x, y in zip(b.Xs, wl.Xs))
        assert np.array_equal(b.hp_v, wl.hp_v) and np.array_equal(b.hp_c, wl.hp_c)
        wth, _ = EC.spline34_weight(wl.radius)
        assert same_bits(b.staged().fetch_grad(), _dev(name).run(wth).fetch_grad())


@pytest.mark.parametrize("name,wname", [("base2", w) for w in EC.weight_kernels(1.0)] + [("base3", "modsqexp")])
def test_every_family_as_the_blending_profile(name, wname):
    wl, dev = EC.workload(name), _dev(name)
    wth, owth = EC.weight_kernels(wl.radius)[wname]
    q = dev.run(wth)
    plane, dbg = check_planes(wl, q, wl.Xq, wl.plan())
    nb = plane >= 0
    w_ref = GR.phi(owth, np.abs(dbg["item_t"][nb]))
    if wname == "spline34_narrow":
        assert np.any(w_ref == 0.0) and np.any(w_ref > 0.0)          # accepted neighbours of weight exactly 0
    ratio, m, n_nb = blend_ratio(q, wl.hp_v, owth)
    assert n_nb >= 40
    assert same_nan_pattern(q, dev.R)
    fd, with_nb = fd_on_stable_queries(dev, wth, EC.has_neighbours)
    _record(group="A", test="weight_family", D=wl.D, weight=wname, ratio=ratio, fd_ratio=fd, neighbour_items=n_nb,
            fd_with_neighbours=with_nb)
    assert ratio <= 1.0 and fd <= 1.0, (ratio, fd)


def test_failed_patch_gives_nan_even_at_weight_zero_and_the_rest_keep_their_bits():
    """test_failed_patch_gives_nan_and_the_rest_keep_their_bits of tests/test_gpu_grad.py with the narrow profile: an item
    of the failed patch makes its query NaN in the gradient as in the mean, also where its weight is exactly 0"""
    r = EC.A_RADIUS[2]
    wth, owth = EC.weight_kernels(r)["spline34_narrow"]
    sound, broken = Blend(2, 3, "spline34", "constant", radius=r), Blend(2, 3, "spline34", "constant", diag_patch=2, radius=r)
    assert broken.model.info()[2] != 0 and np.all(np.delete(broken.model.info(), 2) == 0)
    sound.wth = broken.wth = wth
    qs, qb = sound.staged(), broken.staged()
    Gs, _ = qs.item_grads()
    Gb, plane = qb.item_grads()
    dbg = qb.debug()
    reg, off, t = dbg["item_region"], dbg["item_offsets"], dbg["item_t"]
    bad_item = reg == 2
    assert bad_item.any() and not bad_item.all()
    assert np.all(np.isnan(Gb[bad_item])) and np.array_equal(Gb[~bad_item], Gs[~bad_item])
    w = np.where(plane >= 0, GR.phi(owth, np.abs(t)), 1.0)
    bad_q = np.array([bad_item[off[j]:off[j + 1]].any() for j in range(len(sound.Xq))])
    weightless = np.array([np.all(w[off[j]:off[j + 1]][bad_item[off[j]:off[j + 1]]] == 0.0) for j in range(len(sound.Xq))])
    assert np.any(bad_q & weightless)                               # a query whose only failed items have weight 0
    dYs, dYb = qs.fetch_grad(), qb.fetch_grad()
    assert bad_q.any() and not bad_q.all()
    assert np.all(np.isnan(dYb[bad_q])) and np.array_equal(dYb[~bad_q], dYs[~bad_q])
    assert same_nan_pattern(qb, 3) and same_nan_pattern(qs, 3)
    assert np.array_equal(np.isnan(qb.fetch_multi(3)[0]).any(1), bad_q)


# ------------------------------------------------------------------------------------------ B. larger trees
@pytest.mark.parametrize("name", list(EC.DEEP))
def test_item_plane_on_larger_trees(name):
    wl = EC.workload(name)
    fitted = name in EC.DEEP_FITTED
    dev = _dev(name) if fitted else Dev(wl, fit=False)
    q = M.DeviceQuery(dev.model, wl.Xq)
    q.plan(wl.radius, wl.delta)
    assert pmk.lib().pmk_query_get_items_grad(q.h, None, 0, None) == 0          # the planes need only the plan
    plane, _ = check_planes(wl, q, wl.Xq, wl.plan())
    assert plane.max() >= (256 if wl.levels >= 10 else 32)
    if not fitted:
        _record(group="B", test="planes", case=name, planes=int(wl.P - 1), items=int(q.total), max_plane=int(plane.max()))
        return
    wth, owth = EC.spline34_weight(wl.radius)
    q = dev.run(wth)
    items = item_ratio(dev, q, wl.Xq)
    ratio, m, n_nb = blend_ratio(q, wl.hp_v, owth)
    rec = dict(group="B", test="deep_tree", case=name, planes=int(wl.P - 1), max_plane=int(plane.max()), item_ratio=items,
               ratio=ratio, neighbour_items=n_nb)
    fd = 0.0
    if wl.levels == 7:
        fd, deep = fd_on_stable_queries(dev, wth, EC.has_deep_plane)
        rec.update(fd_ratio=fd, fd_with_plane_ge_32=deep)
    _record(**rec)
    assert items <= 1.0 and ratio <= 1.0 and fd <= 1.0, rec


# ------------------------------------------------------------------------------------------ C. many neighbours
@pytest.mark.parametrize("which", list(EC.C_RADII))
def test_more_neighbours_than_the_stage_holds(which):
    wl, dev = EC.workload("many"), _dev("many")
    radius = EC.C_RADII[which]
    wth, owth = EC.spline34_weight(radius)
    q = dev.run(wth, radius=radius)
    _, dbg = check_planes(wl, q, wl.Xq, wl.plan(radius))
    cnt = np.diff(dbg["item_offsets"]) - 1
    assert cnt.max() > EC.PLAN_STAGE
    ratio, m, n_nb = blend_ratio(q, wl.hp_v, owth)
    _record(group="C", test="many_items", radius=radius, ratio=ratio, largest_m=m, neighbour_items=n_nb)
    assert m == cnt.max() + 1 and ratio <= 1.0, (m, ratio)


def test_the_staged_copy_and_the_second_walk_give_the_same_bits():
    wl, dev = EC.workload("many"), _dev("many")
    wth, _ = EC.spline34_weight(wl.radius)
    a, b, heavy, light = EC.reorderings(wl)
    out = []
    for order in (a, b):
        q = dev.run(wth, wl.Xq[order])
        dbg = q.debug()
        G, plane = q.item_grads()
        U, _ = q.item_values_multi()
        off = dbg["item_offsets"]
        cnt = np.diff(off) - 1
        out.append((order, off, cnt, dbg, G, plane, U, q.fetch_grad()))
    assert out[0][2][:256].max() > EC.PLAN_STAGE and out[1][2][:256].max() <= EC.PLAN_STAGE
    where_b = np.argsort(b)                                          # position of query j in order B
    shared = 0
    (_, offa, _, da, Ga, pla, Ua, dYa), (_, offb, _, db, Gb, plb, Ub, dYb) = out
    for pa, j in enumerate(a):
        pb = where_b[j]
        sa, sb = slice(offa[pa], offa[pa + 1]), slice(offb[pb], offb[pb + 1])
        assert np.array_equal(da["item_region"][sa], db["item_region"][sb]) and np.array_equal(pla[sa], plb[sb]), j
        assert same_bits(da["item_t"][sa], db["item_t"][sb]) and same_bits(Ga[sa], Gb[sb]) and same_bits(Ua[sa], Ub[sb]), j
        assert same_bits(dYa[pa], dYb[pb]), j
        shared += int(pa < 256 and pb < 256)
    assert shared >= 100                                             # queries that sat in block 0 both times
    _record(group="C", test="staged_vs_walk", queries=len(a), heavy=len(heavy), shared_block0=shared)


def test_twelve_and_more_items_per_query():
    """the polygon workload: every query is accepted at the 11 ancestor planes of its leaf (some at more), so the O(m^2) loop
    of mix_grad_kernel and the 16 m u bound run at m = 12 and above, with weights near 1 on every item"""
    wl, dev = EC.workload("polygon"), _dev("polygon")
    wth, owth = EC.spline34_weight(wl.radius)
    q = dev.run(wth)
    _, dbg = check_planes(wl, q, wl.Xq, wl.plan())
    m_all = np.diff(dbg["item_offsets"])
    assert m_all.min() >= 12
    assert GR.phi(owth, np.abs(dbg["item_t"])).min() > 0.5
    items = item_ratio(dev, q, wl.Xq)
    ratio, m, n_nb = blend_ratio(q, wl.hp_v, owth)
    _record(group="C", test="twelve_items", ratio=ratio, item_ratio=items, largest_m=m, smallest_m=int(m_all.min()), neighbour_items=n_nb)
    assert m >= 12 and items <= 1.0 and ratio <= 1.0, (m, items, ratio)


# ------------------------------------------------------------------------------------------ D. exact t
def test_query_on_a_plane():
    wl, dev = EC.workload("on_plane"), _dev("on_plane")
    wth, owth = EC.spline34_weight(wl.radius)
    q = dev.run(wth)
    _, dbg = check_planes(wl, q, wl.Xq, wl.plan())
    off, t = dbg["item_offsets"], dbg["item_t"]
    assert off[1] == 2 and t[0] == 0.0 and t[1] == 0.0
    G, _ = q.item_grads()
    assert np.all(np.isfinite(G[:2])) and not np.array_equal(G[0], G[1])
    dY = q.fetch_grad()
    assert same_bits(dY[0], (G[0] + G[1]) / 2)                       # w(0) = 1 and dw = 0: the mean of the two, bit for bit
    ratio, _, _ = blend_ratio(q, wl.hp_v, owth)
    # w(0) = 0.7 against the home weight 1
    wth, owth = EC.weight_kernels(wl.radius)["trq"]
    q = dev.run(wth)
    G, plane = q.item_grads()
    U, _ = q.item_values_multi()
    dY = q.fetch_grad()
    want = (GR.LD(7) / GR.LD(10) * np.asarray(G[0], dtype=GR.LD) + np.asarray(G[1], dtype=GR.LD)) / (GR.LD(17) / GR.LD(10))
    _, mag = GR.mix_grad_ref(range(2), G, U, q.debug()["item_t"], plane, wl.hp_v, owth)
    bound = 16 * 2 * 2.0 ** -53 * mag.astype(np.float64)
    r07 = _worst_ratio(np.abs(np.asarray(dY[0], dtype=GR.LD) - want).astype(np.float64), bound)
    ratio_trq, _, _ = blend_ratio(q, wl.hp_v, owth)
    _record(group="D", test="on_plane", ratio=ratio, ratio_trq=ratio_trq, ratio_trq_closed_form=r07)
    assert ratio <= 1.0 and ratio_trq <= 1.0 and r07 <= 1.0


@pytest.mark.parametrize("name", ["grid", "dups"])
def test_training_points_as_queries(name):
    wl, dev = EC.workload(name), _dev(name)
    wth, owth = EC.spline34_weight(wl.radius)
    q = dev.run(wth)
    _, dbg = check_planes(wl, q, wl.Xq, wl.plan())
    G, plane = q.item_grads()
    assert np.all(np.isfinite(G)) and np.all(np.isfinite(q.fetch_grad()))
    exact = int(np.sum((plane >= 0) & (np.abs(dbg["item_t"]) < 1e-12)))
    items = item_ratio(dev, q, wl.Xq)
    ratio, m, n_nb = blend_ratio(q, wl.hp_v, owth)
    _record(group="D", test="training_points", case=name, item_ratio=items, ratio=ratio, neighbour_items=n_nb, items_on_a_plane=exact)
    assert exact >= 10
    assert items <= 1.0 and ratio <= 1.0, (items, ratio)


@pytest.mark.parametrize("radius", [0.0] + EC.HUGE_RADII)
def test_plan_radius_zero_and_huge(radius):
    wl, dev = EC.workload("base2"), _dev("base2")
    wth, owth = EC.weight_kernels(0.8)["gaussian"]                  # not compact: every accepted neighbour has a weight,
    q = dev.run(wth, radius=radius)                                  # which may underflow to 0
    plane, dbg = check_planes(wl, q, wl.Xq, wl.plan(radius))
    if radius == 0.0:
        assert q.total == q.Nq and np.all(plane == -1)
        assert same_bits(q.fetch_grad(), q.item_grads()[0])          # the home item's gradient, bit for bit
        return
    ratio, m, n_nb = blend_ratio(q, wl.hp_v, owth)
    _record(group="D", test="huge_radius", radius=radius, ratio=ratio, neighbour_items=n_nb, largest_abs_t=float(np.abs(dbg["item_t"]).max()))
    assert n_nb >= 300 and ratio <= 1.0, (n_nb, ratio)


# ------------------------------------------------------------------------------------------ E. ranges and blocks
def _range_query(nq):
    wl, dev = EC.workload("base2"), _dev("base2")
    q = M.DeviceQuery(dev.model, wl.queries(nq))
    q.plan(wl.radius, wl.delta)
    dev.items(q)
    wa, wb = EC.spline34_weight(wl.radius)[0], EC.weight_kernels(wl.radius)["gaussian"][0]
    q.mix_multi(wa)
    return q, wa, wb


@pytest.mark.parametrize("nq", EC.E_NQ)
def test_ranges_that_tile_the_queries_equal_the_full_range(nq):
    q, wa, wb = _range_query(nq)
    q.mix_grad(wa)
    A = q.fetch_grad()
    q.mix_grad(wb)
    B = q.fetch_grad()
    has_nb = np.diff(q.debug()["item_offsets"]) > 1
    assert np.all(np.isfinite(A)) and (nq == 1 or not np.array_equal(A[has_nb], B[has_nb]))
    for q0, q1 in EC.range_chain(nq):                                # over the rows of B: every row is written again
        q.mix_grad(wa, q0, q1)
    assert same_bits(q.fetch_grad(), A)
    for at in sorted({0, nq // 2, nq}):                              # q0 == q1 is accepted and changes nothing
        q.mix_grad(wb, at, at)
    assert same_bits(q.fetch_grad(), A)
    L, d = pmk.lib(), wa.desc()
    for q0, q1 in ((-1, nq), (0, nq + 1), (nq, nq - 1), (1, 0)):
        assert L.pmk_query_mix_grad(q.h, C.byref(d), q0, q1) == -3, (q0, q1)
    assert same_bits(q.fetch_grad(), A)
    _record(group="E", test="ranges", Nq=nq, chain=EC.range_chain(nq), with_neighbours=int(has_nb.sum()))


def test_rows_outside_a_range_keep_their_bits():
    q, wa, wb = _range_query(513)
    q.mix_grad(wb)
    B = q.fetch_grad()
    q.mix_grad(wa)
    A = q.fetch_grad()
    q.mix_grad(wb, 100, 300)
    got = q.fetch_grad()
    inside = np.zeros(513, dtype=bool)
    inside[100:300] = True
    assert same_bits(got[~inside], A[~inside]) and same_bits(got[inside], B[inside])
    has_nb = np.diff(q.debug()["item_offsets"]) > 1
    assert not np.array_equal(A[inside & has_nb], B[inside & has_nb]) and (has_nb & ~inside).sum() >= 20


# ------------------------------------------------------------------------------------------ F. buffer lifetime
def test_replans_and_a_change_of_R_on_one_query():
    wl = EC.workload("base2")
    wth, _ = EC.spline34_weight(wl.radius)

    def results(dev, q):
        dev.items(q)
        q.mix_multi(wth)
        q.mix_grad(wth)
        return q.fetch_grad(), q.item_grads()[0], q.fetch_multi(dev.R)[0]

    def fresh(R, radius):
        dev = Dev(wl, R=R)
        q = M.DeviceQuery(dev.model, wl.Xq)
        q.plan(radius, wl.delta)
        return results(dev, q), q.total

    small, large = EC.F_RADII["small"], EC.F_RADII["large"]
    dev = Dev(wl, R=1)
    q = M.DeviceQuery(dev.model, wl.Xq)
    totals = []
    for stage, (R, radius, replan) in enumerate([(1, small, True), (1, large, True), (16, large, False), (1, small, True)]):
        if R != dev.R:
            dev.R = R
            dev.solve(wl.Ys(R))
        if replan:
            q.plan(radius, wl.delta)
        got = results(dev, q)
        want, total = fresh(R, radius)
        assert q.total == total
        totals.append(total * R)
        for g, w, what in zip(got, want, ("fetch_grad", "item_grads", "fetch_multi")):
            assert same_bits(g, w), (stage, what)
    assert totals[0] < totals[1] < totals[2] and totals[3] == totals[0]          # grows twice, then capacity exceeds need
    _record(group="F", test="buffer_lifetime", item_values=totals)


# ------------------------------------------------------------------------------------------ G. paths that must not matter
def test_the_variance_strip_before_the_gradient_changes_no_bit():
    wl, dev = EC.workload("base2"), _dev("base2")
    wth, _ = EC.spline34_weight(wl.radius)
    qv, qm = dev.run(wth, variance=True), dev.run(wth, variance=False)
    assert qv.fetch_multi(dev.R)[1] is not None and qm.fetch_multi(dev.R)[1] is None
    assert same_bits(qv.item_grads()[0], qm.item_grads()[0]) and same_bits(qv.fetch_grad(), qm.fetch_grad())
    assert same_bits(qv.fetch_multi(dev.R)[0], qm.fetch_multi(dev.R)[0])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_planned_blend_over_mixed_families_and_noise_per_patch(dtype):
    name = "base2" if dtype == "f64" else "base2_f32"
    wl = EC.workload(name)
    dev = _dev(name, thetas=EC.MIXED_NAMES, sigma2s=EC.MIXED_SIGMA2[dtype])
    assert len(wl.Xs) == len(EC.MIXED_NAMES)
    wth, owth = EC.spline34_weight(wl.radius)
    q = dev.run(wth)
    check_planes(wl, q, wl.Xq, wl.plan())
    items = item_ratio(dev, q, wl.Xq)
    ratio, m, n_nb = blend_ratio(q, wl.hp_v, owth)
    rec = dict(group="G", test="mixed_families", dtype=dtype, item_ratio=items, ratio=ratio, neighbour_items=n_nb)
    fd = 0.0
    if dtype == "f64":
        fd, with_nb = fd_on_stable_queries(dev, wth, EC.has_neighbours)
        rec.update(fd_ratio=fd, fd_with_neighbours=with_nb)
    _record(**rec)
    assert n_nb >= 40 and items <= 1.0 and ratio <= 1.0 and fd <= 1.0, rec


def test_fp32_model_with_a_uniform_theta():
    """the blend of an fp32 model's items against the reference, and the central-difference rule with u = 2^-24 on queries
    and stencil points that are float32 numbers, at h = 2^-10 of the width (see the module's docstring)"""
    wl, dev = EC.workload("base2_f32"), _dev("base2_f32")
    wth, owth = EC.spline34_weight(wl.radius)
    q = dev.run(wth)
    items = item_ratio(dev, q, wl.Xq)
    ratio, m, n_nb = blend_ratio(q, wl.hp_v, owth)
    Xq32 = _round(wl.Xq, "f32")
    out = {}
    for e in (17, 10):
        h = wl.width * 2.0 ** -e
        pick, with_nb = wl.stable_pick(EC.has_neighbours, Xq=Xq32, h=h)
        assert len(pick) == 16 and with_nb >= 4
        Xc = Xq32[pick]
        assert all(np.array_equal(p, _round(p, "f32")) for x in Xc for p in wl.stencil(x, h))      # h is a power of two: exact
        out[e] = fd_ratio(dev, wth, Xc, dev.run(wth, Xc).fetch_grad(), u=2.0 ** -24, h=h, check=False)
    _record(group="G", test="fp32_model", item_ratio=items, ratio=ratio, neighbour_items=n_nb, fd_ratio=out[10][0],
            fd_tolerance_over_gradient=out[10][1], **{"fd_ratio_at_2^-17": out[17][0], "fd_tolerance_over_gradient_at_2^-17": out[17][1]})
    assert n_nb >= 40 and items <= 1.0 and ratio <= 1.0, (items, ratio)
    assert out[10][1] <= 0.1 and out[10][0] <= 1.0, out
