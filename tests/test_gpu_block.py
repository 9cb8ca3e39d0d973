"""Block kriging on the GPU (pmk_query_items_block, pmk_predict_mixture_block_fitted; the kernels of pmk_block.hip): mean
and kriging variance of weighted sums of the blended field over groups of queries.

Reference: tests/_block_refs.py, the numpy.longdouble restatement that tests/test_block_refs.py pins to a^T Cov a of the
joint covariance, to the textbook form and to the singleton identity.  Unit of a group:
    E_f = sum_r sum_{i,i' in (r,f)} |w_i| |w_i'| e_r(i,i'),   e_r the unit of a block entry of tests/test_gpu_cov.py (with the
    trend part of tests/test_gpu_cov_multi.py), (n_r + 32) u included, u = 2^-53 (fp64) or 2^-24 (fp32),
and every ratio err / E_f must stay <= 10.  Means: the per-item bound of tests/test_gpu_multi_edges.py (fp64:
2 (n + 4 + q) u S + 1e-18 sum |C|; fp32: 50 sqrt(kappa(U)) eps32 (S + 1)) summed with |w_i|.  tests/test_block_refs.py checks
on the same inputs (tests/_block_cases.py, where sigma2 of the fp32 cases is explained) that a plain numpy evaluation stays
below one unit and that every aggregate lies 100 units above its floor.  No accuracy case may sit on
its floor: asserted here on the device's own pieces (kappa - |Vbar|^2 > min_v sum w^2 for every aggregate).

Every measured ratio is printed ("BLOCK {json}", run with -s); with PMK_WRITE_PROFILES=1 a run of the whole module writes
them to profiles/block_accuracy.json, each with `plain`, the figure of a plain numpy / LAPACK evaluation of the same case in
the model's precision against the same reference and unit.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
from patchmixturekriging_amd import mixture as M
import _block_cases as BC
import _block_refs as BR
import _cov_cases as CC
import _cov_multi_cases as CMC
import _cov_multi_refs as CMR
import _cov_refs as CR
import _grad_edge_cases as GE
import _multi_refs as R_
import _trend_refs as T
from oracle import oracle as O
from test_block_refs import main_case
from test_gpu_cov_multi import _bits
from test_gpu_grad import _worst_ratio

pytestmark = pytest.mark.gpu

U_OF, SIGMA2, RATIO_MAX, LD = CC.U_OF, BC.SIGMA2, CC.RATIO_MAX, CR.LD
MIN_V = 1e-12
_RECORDS = []
ACCURACY_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "block_accuracy.json")


def _record(**kw):
    _RECORDS.append(kw)
    print("BLOCK " + json.dumps(kw, sort_keys=True))


@pytest.fixture(scope="module", autouse=True)
def _write_accuracy_file():
    yield
    if os.environ.get("PMK_WRITE_PROFILES") == "1" and {"main", "edges", "profiles", "singletons", "large"} <= {r["test"] for r in _RECORDS}:
        with open(ACCURACY_JSON, "w") as f:
            f.write("[\n" + ",\n".join(" " + json.dumps(r, sort_keys=True) for r in _RECORDS) + "\n]\n")


def _model(Xs, Ys, th, dtype, root, trend, diag=None):
    """fit with the sigma2 of tests/_block_cases.py, attach the tree, R target columns, the trend, the multi-output solve"""
    model = M.DeviceModel(Xs, [np.ascontiguousarray(y[:, 0]) for y in Ys], dtype=dtype)
    if diag is not None:
        model.set_diag(diag)
    if isinstance(th, list):
        model.fit_patches(th, [SIGMA2[dtype]] * len(Xs))
    else:
        model.fit(th, SIGMA2[dtype])
    model.set_bsp(root, 0)
    model.set_targets_multi(Ys)
    model.set_trend(trend)
    model.solve_multi()
    return model


def _block(model, Xq, radius, delta, group, a, wth, F=None, th=None, variance=True, addend=None):
    q = M.DeviceQuery(model, Xq)
    q.plan(radius, delta)
    if addend is not None:
        q.set_diag(addend)
    q.items_multi_fitted(False) if th is None else q.items_multi(th, False)
    q.items_block(group, a, wth, F=F, theta=th, variance=variance)
    return q


def _device_items(q):
    dbg = q.debug()
    return dbg["item_offsets"], dbg["item_region"], dbg["item_t"]


def _mean_bound(model, q, items, oths, Xs, Xq, trend, dtype, refs):
    """(reference item means [total, R] in long double, per-item bound [total, R]) from the model's own weights"""
    Cs = model.weights_multi()
    qt = CMC.Q_OF[trend](Xq.shape[1])
    betas = model.trend()[0] if qt else None
    off, reg = items[0], items[1]
    query_of = np.repeat(np.arange(len(off) - 1), np.diff(off))
    R = Cs[0].shape[1] if Cs[0].ndim == 2 else 1
    ref, bound = np.zeros((len(reg), R), dtype=LD), np.zeros((len(reg), R))
    for r in sorted(set(int(v) for v in reg)):
        sel = np.nonzero(reg == r)[0]
        x = Xq[query_of[sel]]
        mu, S, _ = R_.item_means_reference(oths[r], Xs[r], Cs[r], x)
        terms = len(Xs[r]) + 4
        if qt:
            Hq = T.basis(x, trend)
            mu = mu + np.asarray(Hq, dtype=LD) @ np.asarray(betas[r], dtype=LD)
            S = S + np.abs(Hq) @ np.abs(betas[r])
            terms += qt
        if dtype == "f64":
            b = 2 * terms * U_OF["f64"] * S + 1e-18 * np.abs(np.asarray(Cs[r]).reshape(len(Xs[r]), -1)).sum(0)[None, :]
        else:
            b = 50 * refs[r].kappa * 2.0 ** -23 * (S + 1)            # sqrt(kappa(U)) = kappa2(L); eps32 = 2^-23
        ref[sel], bound[sel] = mu, b
    return ref, bound


def _check(q, model, items, group, a, F, refs, oths, Xs, Xq, wth_o, trend, dtype, addend=None, sigma2=None):
    """-> dict of worst ratios: variance, mean, the pieces against the reference, and `plain`, the ratio of a plain numpy
    evaluation of the same case in the model's precision; asserts the aggregate list and that no aggregate sits on its floor"""
    Yb, Vb = q.fetch_block()
    out = BR.block_ref(items[:2], items[2], wth_o, group, a, F, refs, Xq, U_OF[dtype], addend, MIN_V)
    pieces = q.item_blocks()
    assert [(x["region"], x["group"], x["count"]) for x in out["aggs"]] == \
        list(zip(pieces["region"].tolist(), pieces["group"].tolist(), pieces["count"].tolist()))
    # nothing hides behind the clamp; an aggregate whose weights are all zero (a profile that vanishes at its items'
    # distances) has no floor to sit on and contributes exactly nothing
    live = pieces["sw2"] > 0
    assert np.array_equal(live, np.array([float(x["sw2"]) > 0 for x in out["aggs"]]))
    assert np.all((pieces["kappa"] - pieces["vnorm2"])[live] > MIN_V * pieces["sw2"][live])
    assert np.all(pieces["kappa"][~live] == 0) and np.all(pieces["vnorm2"][~live] == 0) and np.all(pieces["znorm2"][~live] == 0)
    var = _worst_ratio(np.abs(np.asarray(np.asarray(Vb, dtype=LD) - out["Var"], dtype=np.float64)), out["unit"])
    au = np.array([x["unit"] for x in out["aggs"]])
    kv = np.array([float(x["kappa"] - x["vn2"]) for x in out["aggs"]])
    piece = _worst_ratio(np.abs((pieces["kappa"] - pieces["vnorm2"]) - kv), au)
    ref_u, bound_u = _mean_bound(model, q, items, oths, Xs, Xq, trend, dtype, refs)
    aw = np.abs(np.asarray(out["w"], dtype=np.float64))
    gi = np.asarray(group, dtype=np.int64)[out["query_of"]]
    want = np.zeros((F, ref_u.shape[1]), dtype=LD)
    np.add.at(want, gi, out["w"][:, None] * ref_u)
    mb = np.zeros((F, ref_u.shape[1]))
    np.add.at(mb, gi, aw[:, None] * bound_u)
    mean = _worst_ratio(np.abs(np.asarray(np.asarray(Yb, dtype=LD) - want, dtype=np.float64)), mb)
    T_ = np.float64 if dtype == "f64" else np.float32
    pv = BR.plain_block_var(items[:2], items[2], wth_o, group, a, F, oths, Xs, SIGMA2[dtype] if sigma2 is None else sigma2, trend,
                            Xq, T_, addend, MIN_V)
    plain = _worst_ratio(np.abs(pv - np.asarray(out["Var"], dtype=np.float64)), out["unit"])
    return dict(var=var, mean=mean, pieces=piece, plain=plain, naggs=len(au)), out, Yb, Vb


# ------------------------------------------------------------------------------------------ the main workload
@pytest.mark.parametrize("dtype,family,trend,R", [(d, f, t, R) for d in ("f64", "f32") for f in ("spline34", "gaussian")
                                                  for t, R in BC.TREND_R])
def test_mean_and_variance_of_group_sums(dtype, family, trend, R):
    m, items, refs, _ = main_case(dtype, family, trend)
    th, oth = CC.FAMILIES[family]
    model = _model(m.Xs, m.Ys(R), th, dtype, m.root, trend)
    assert np.all(model.info() == 0) and np.all(model.trend_info() == 0)
    q = _block(model, m.Xq, m.RADIUS, m.DELTA, m.group, m.a, m.wth, th=th)
    dev = _device_items(q)
    assert np.array_equal(dev[0], items[0]) and np.array_equal(dev[1], items[1])
    res, out, Yb, Vb = _check(q, model, dev, m.group, m.a, m.F, refs, [oth] * 4, m.Xs, m.Xq, m.owth, trend, dtype)
    assert Yb.shape == (m.F, R) and Vb.shape == (m.F,)
    # one wave holds columns of 1 and of 65 members: region 0 has fewer than 256 aggregates (one strip), columns k and k + 1
    p = q.item_blocks()
    pairs = [k for k in range(len(p["count"]) - 1) if p["region"][k] == p["region"][k + 1] and
             {int(p["count"][k]), int(p["count"][k + 1])} == {1, 65}]
    first = {r: int(np.nonzero(p["region"] == r)[0][0]) for r in set(p["region"].tolist())}
    assert any((k - first[int(p["region"][k])]) // 32 == (k + 1 - first[int(p["region"][k])]) // 32 for k in pairs), pairs
    # against the device's own dense covariance: a^T Cov a, within the sum of both bounds
    q.mix_multi(m.wth)
    q.items_cov_multi(th)
    q.mix_cov(m.wth)
    Cov = np.asarray(q.fetch_cov(), dtype=LD)
    A = np.zeros((m.F, len(m.Xq)), dtype=LD)
    A[m.group, np.arange(len(m.Xq))] = np.asarray(m.a, dtype=LD)
    dense = np.einsum("fj,jk,fk->f", A, Cov, A)
    res["dense"] = _worst_ratio(np.abs(np.asarray(np.asarray(Vb, dtype=LD) - dense, dtype=np.float64)), 2 * out["unit"])
    _record(test="main", dtype=dtype, family=family, trend=trend, R=R, **res)
    assert res["var"] <= RATIO_MAX and res["pieces"] <= RATIO_MAX and res["dense"] <= RATIO_MAX and res["mean"] <= 1.0, res


# ------------------------------------------------------------------------------------------ strip and patch edges
def _edge_run(D, dtype, names=None, addend=False):
    root, Xs, Xq, group, a, home = BC.edge_queries(D, dtype)
    names = names or ["spline34"] * 8
    ths, oths = [CC.FAMILIES[n][0] for n in names], [CC.FAMILIES[n][1] for n in names]
    uniform = len(set(names)) == 1
    model = _model(Xs, [CMC.targets(X, 2) for X in Xs], ths[0] if uniform else ths, dtype, root, None)
    assert np.all(model.info() == 0)
    ad = np.random.default_rng(5).uniform(0.0, 0.5, len(Xq)) if addend else None
    wth, owth = pmk.Spline34KernelType(1.0), O.kernel(O.SPLINE34, 1.0)
    q = _block(model, Xq, BC.EDGE_RADIUS, BC.EDGE_DELTA, group, a, wth, th=ths[0] if uniform else None, addend=ad)
    dev = _device_items(q)
    assert np.array_equal(dev[1], home) and np.all(np.diff(dev[0]) == 1)               # the home item alone
    refs = {r: CMR.TrendRegionRef(oths[r], Xs[r], SIGMA2[dtype], None) for r in sorted(set(home.tolist()))}
    F = int(group[-1]) + 1
    res, out, Yb, Vb = _check(q, model, dev, group, a, F, refs, oths, Xs, Xq, owth, None, dtype, ad)
    p = q.item_blocks()
    assert [int(np.sum(p["region"] == r)) for r in range(8)] == list(BC.EDGE_AGGS)
    return res, max(r.kappa for r in refs.values()), Vb, q


@pytest.mark.parametrize("D,dtype", [(1, "f64"), (2, "f64"), (4, "f64"), (2, "f32")])
def test_strip_and_patch_edges(D, dtype):
    """1, 255, 256, 257 and 513 aggregates in a region; patches of 1, 127, 128, 129 and 300 points"""
    res, kappa, _, _ = _edge_run(D, dtype)
    _record(test="edges", D=D, dtype=dtype, kappa=kappa, **res)
    assert kappa <= CC.KAPPA_MAX and res["var"] <= RATIO_MAX and res["pieces"] <= RATIO_MAX and res["mean"] <= 1.0, res


def test_mixed_families_per_patch_and_set_diag_addends():
    res, kappa, _, _ = _edge_run(2, "f64", CC.MIXED_NAMES)
    _record(test="mixed", kappa=kappa, **res)
    assert kappa <= CC.KAPPA_MAX and res["var"] <= RATIO_MAX and res["pieces"] <= RATIO_MAX and res["mean"] <= 1.0, res
    res, _, with_addend, _ = _edge_run(2, "f64", addend=True)
    _, _, plain, _ = _edge_run(2, "f64")
    _record(test="diag", **res)
    assert res["var"] <= RATIO_MAX and np.all(with_addend > plain), res


# ------------------------------------------------------------------------------------------ weights
def _main_f64(trend="linear", R=2):
    m, items, refs, _ = main_case("f64", "spline34", trend)
    th, oth = CC.FAMILIES["spline34"]
    return m, items, refs, th, oth, _model(m.Xs, m.Ys(R), th, "f64", m.root, trend)


def test_contrasts_zero_weights_an_empty_group_and_no_query():
    m, items, refs, th, oth, model = _main_f64()
    Nq = len(m.Xq)
    # groups of 40; group 3 is left out (F counts it): an empty group in the middle; a contrast in group 0, zeros in group 1
    group = (np.arange(Nq) // 40).astype(np.int32)
    group[group >= 3] += 1
    F = int(group[-1]) + 1
    a = BC.averages(group)
    a[20:40] *= -1.0
    a[40:80:2] = 0.0
    q = _block(model, m.Xq, m.RADIUS, m.DELTA, group, a, m.wth, F=F, th=th)
    res, out, Yb, Vb = _check(q, model, items, group, a, F, refs, [oth] * 4, m.Xs, m.Xq, m.owth, "linear", "f64")
    _record(test="weights", **res)
    assert res["var"] <= RATIO_MAX and res["mean"] <= 1.0, res
    assert np.all(Yb[3] == 0) and Vb[3] == 0 and not np.signbit(Vb[3]) and np.all(Vb[np.arange(F) != 3] > 0)
    # the contrast of two halves is far less uncertain than their mean
    q.items_block(group, np.abs(a), m.wth, F=F, theta=th)
    assert q.fetch_block()[1][0] > Vb[0]
    # no query at all
    q0 = M.DeviceQuery(model, np.zeros((0, 2)))
    assert q0.plan(m.RADIUS, m.DELTA) == 0
    q0.items_multi(th, False)
    q0.items_block(np.zeros(0, dtype=np.int32), np.zeros(0), m.wth, F=2, theta=th)
    Y0, V0 = q0.fetch_block()
    assert Y0.shape == (2, 2) and np.all(Y0 == 0) and np.all(V0 == 0)
    assert q0.item_blocks()["count"].shape == (0,)


@pytest.mark.parametrize("name", sorted(GE.weight_kernels(1.0)))
def test_seven_blending_profiles(name):
    """the weights are those of the mix for every stationary profile; groups of up to 65 queries with several items each"""
    m, items, refs, th, oth, model = _main_f64()
    wth, owth = GE.weight_kernels(m.RADIUS)[name]
    q = _block(model, m.Xq, m.RADIUS, m.DELTA, m.group, m.a, wth, th=th)
    assert np.diff(items[0]).max() >= 2
    if name == "spline34_narrow":                                # vanishes at half the plan radius: items of weight exactly zero
        assert any(float(x["sw2"]) == 0 for x in BR.block_ref(items[:2], items[2], owth, m.group, m.a, m.F, refs, m.Xq, U_OF["f64"])["aggs"])
    res, _, _, _ = _check(q, model, items, m.group, m.a, m.F, refs, [oth] * 4, m.Xs, m.Xq, owth, "linear", "f64")
    _record(test="profiles", profile=name, **res)
    assert res["var"] <= RATIO_MAX and res["pieces"] <= RATIO_MAX and res["mean"] <= 1.0, res
    # a Brownian-bridge profile is no profile
    bb, d = pmk.BrownianBridge10(1.0).desc(), th.desc()
    g, a = np.ascontiguousarray(m.group), np.ascontiguousarray(m.a)
    assert pmk.lib().pmk_query_items_block(q.h, C.byref(d), C.byref(bb), m.F, g.ctypes.data_as(C.POINTER(C.c_int32)), M._d(a), 1) == -2


def test_fp32_pieces_on_an_ill_conditioned_factor():
    """sigma2 = 0.05, the setting of the covariance tests (kappa2(L) 23 to 29): there kappa - |Vbar|^2 is a fraction of one
    fp32 unit, so the two pieces are checked one by one, each within 10 units, and no variance is asserted"""
    dtype, s2 = "f32", CC.SIGMA2["f32"]
    m, items, _, _ = main_case(dtype, "spline34", None)
    th, oth = CC.FAMILIES["spline34"]
    refs = {r: CMR.TrendRegionRef(oth, m.Xs[r], s2, None) for r in range(4)}
    model = M.DeviceModel(m.Xs, [np.ascontiguousarray(y[:, 0]) for y in m.Ys(1)], dtype=dtype)
    model.fit(th, s2)
    model.set_bsp(m.root, 0)
    model.set_targets_multi(m.Ys(1))
    model.set_trend(None)
    model.solve_multi()
    assert np.all(model.info() == 0)
    q = _block(model, m.Xq, m.RADIUS, m.DELTA, m.group, m.a, m.wth, th=th)
    out = BR.block_ref(items[:2], items[2], m.owth, m.group, m.a, m.F, refs, m.Xq, U_OF[dtype])
    p = q.item_blocks()
    au = np.array([x["unit"] for x in out["aggs"]])
    kap = _worst_ratio(np.abs(p["kappa"] - np.array([float(x["kappa"]) for x in out["aggs"]])), au)
    vn2 = _worst_ratio(np.abs(p["vnorm2"] - np.array([float(x["vn2"]) for x in out["aggs"]])), au)
    _record(test="fp32_pieces", kappa2_L=max(r.kappa for r in refs.values()), kappa=kap, vnorm2=vn2)
    assert max(r.kappa for r in refs.values()) > 20 and kap <= RATIO_MAX and vn2 <= RATIO_MAX, (kap, vn2)


def test_a_query_with_two_items_of_one_region():
    mm = CC.Many()
    th, oth = CC.FAMILIES["spline34"]
    model = _model(mm.Xs, [np.ascontiguousarray(mm.y[i])[:, None] for i in mm.inds], th, "f64", mm.root, "constant")
    group = (np.arange(len(mm.Xq)) // 4).astype(np.int32)
    a = BC.averages(group)
    q = _block(model, mm.Xq, mm.RADIUS, mm.DELTA, group, a, mm.wth, th=th)
    dev = _device_items(q)
    off, reg = dev[0], dev[1]
    assert any(len(set(reg[off[j]:off[j + 1]])) < off[j + 1] - off[j] for j in range(len(mm.Xq)))
    refs = {r: CMR.TrendRegionRef(oth, mm.Xs[r], SIGMA2["f64"], "constant") for r in sorted(set(reg.tolist()))}
    res, _, _, _ = _check(q, model, dev, group, a, int(group[-1]) + 1, refs, [oth] * len(mm.Xs), mm.Xs, mm.Xq, mm.owth,
                          "constant", "f64")
    _record(test="many", **res)
    assert res["var"] <= RATIO_MAX and res["pieces"] <= RATIO_MAX and res["mean"] <= 1.0, res


# ------------------------------------------------------------------------------------------ singletons and the floor
@pytest.mark.parametrize("dtype,trend", [("f64", None), ("f64", "linear"), ("f32", "linear")])
def test_singleton_groups_answer_vq_and_yq(dtype, trend):
    m, items, refs, _ = main_case(dtype, "spline34", trend)
    th, oth = CC.FAMILIES["spline34"]
    model = _model(m.Xs, m.Ys(3), th, dtype, m.root, trend)
    Nq = len(m.Xq)
    q = M.DeviceQuery(model, m.Xq)
    q.plan(m.RADIUS, m.DELTA)
    q.items_multi(th, True)
    q.mix_multi(m.wth)
    Yq, Vq = q.fetch_multi(3)
    q.items_block(np.arange(Nq, dtype=np.int32), np.ones(Nq), m.wth, theta=th)
    Yb, Vb = q.fetch_block()
    out = BR.block_ref(items[:2], items[2], m.owth, np.arange(Nq), np.ones(Nq), Nq, refs, m.Xq, U_OF[dtype])
    off, reg = items[0], items[1]
    single = np.array([len(set(reg[off[j]:off[j + 1]])) == off[j + 1] - off[j] for j in range(Nq)])
    var = _worst_ratio(np.abs(Vb - Vq)[single], out["unit"][single])
    # the means are the same sums of the same products up to the order of the two roundings of a w / sw
    mean = float(np.max(np.abs(Yb - Yq) / (np.abs(Yq) + 1e-300)))
    T_ = np.float64 if dtype == "f64" else np.float32
    pv = BR.plain_block_var(items[:2], items[2], m.owth, np.arange(Nq), np.ones(Nq), Nq, [oth] * 4, m.Xs, SIGMA2[dtype], trend,
                            m.Xq, T_)
    plain = _worst_ratio(np.abs(pv - np.asarray(out["Var"], dtype=np.float64))[single], out["unit"][single])
    _record(test="singletons", dtype=dtype, trend=trend, var=var, plain=plain, mean_rel=mean)
    assert var <= RATIO_MAX and mean <= 8 * 2.0 ** -53, (var, mean)


def test_the_floor():
    """NOT the clamp workload of tests/test_gpu_vgrad_edges.py: that one is made of explicit (point, region) items, which
    belong to no blend and are refused here; this is the same kind of input under a tree.
    Separated points (K = I exactly) with a tiny sigma2, queries on training points: every item's kappa - |Vbar|^2 =
    w^2 sigma2 / (1 + sigma2) is below its floor, and a singleton group answers min_v w^2 per item (a query on a hyperplane
    holds two items of weight 1 / 2)"""
    g = np.arange(12.0)
    X = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2) - 5.5                            # 144 points a unit apart
    root, _, _ = pmk.setuppartition(X, 3)
    Xs, inds, _, _ = pmk.organizetrainingsets(root, 3, X, 0.1)
    th = pmk.Spline34KernelType(2.0)                                                   # support radius 1 / 2
    model = M.DeviceModel(Xs, [np.zeros(len(x)) for x in Xs])
    model.fit(th, 1e-14)
    model.set_bsp(root, 0)
    model.set_targets_multi([CMC.targets(x, 1) for x in Xs])
    model.set_trend(None)
    model.solve_multi()
    assert np.all(model.info() == 0)
    Xq = np.ascontiguousarray(np.vstack([x[:5] for x in Xs]))
    wth = pmk.Spline34KernelType(1.0)
    q = _block(model, Xq, 1e-9, 1e-12, np.arange(len(Xq), dtype=np.int32), np.ones(len(Xq)), wth, th=th)
    _, Vb = q.fetch_block()
    p = q.item_blocks()
    assert np.all(p["count"] == 1) and np.all(np.isin(p["sw2"], (1.0, 0.25))) and np.any(p["sw2"] == 1.0)
    assert np.all(p["kappa"] - p["vnorm2"] < MIN_V * p["sw2"]) and np.all(p["kappa"] - p["vnorm2"] > 0)
    want = np.zeros(len(Xq))
    np.add.at(want, p["group"], MIN_V * p["sw2"])
    assert np.array_equal(Vb, want) and np.all(Vb <= MIN_V)
    # two queries with a = 1 / 2 each: the floor of every aggregate is min_v sum w^2
    group = (np.arange(len(Xq)) // 2).astype(np.int32)
    q.items_block(group, np.full(len(Xq), 0.5), wth, theta=th)
    p = q.item_blocks()
    want = np.zeros(int(group[-1]) + 1)
    np.add.at(want, p["group"], MIN_V * p["sw2"])
    assert np.all(p["kappa"] - p["vnorm2"] < MIN_V * p["sw2"]) and np.allclose(q.fetch_block()[1], want, rtol=1e-15, atol=0)
    _record(test="floor", groups=int(len(Xq)))


# ------------------------------------------------------------------------------------------ bits
def test_bits_sub_batches_reruns_and_neighbours_in_the_wave():
    m, items, refs, th, oth, model = _main_f64()
    q = _block(model, m.Xq, m.RADIUS, m.DELTA, m.group, m.a, m.wth, th=th)
    Yb, Vb = q.fetch_block()
    p = q.item_blocks()
    # a second run
    q.items_block(m.group, m.a, m.wth, theta=th)
    Y2, V2 = q.fetch_block()
    p2 = q.item_blocks()
    assert _bits(Yb, Y2) and _bits(Vb, V2) and all(_bits(p[k].astype(np.float64), p2[k].astype(np.float64)) for k in p)
    # a sub-batch of groups: other neighbours in the wave, other strips, the same bits
    for keep in ([5], [0, 7, 8], list(range(3, m.F, 2))):
        sel = np.nonzero(np.isin(m.group, keep))[0]
        sub_group = np.searchsorted(np.array(keep), m.group[sel]).astype(np.int32)
        qs = _block(model, m.Xq[sel], m.RADIUS, m.DELTA, sub_group, m.a[sel], m.wth, th=th)
        Ys, Vs = qs.fetch_block()
        assert _bits(Ys, Yb[keep]) and _bits(Vs, Vb[keep]), keep
        ps = qs.item_blocks()
        mask = np.isin(p["group"], keep)
        for k in ("kappa", "vnorm2", "znorm2", "sw2"):
            assert _bits(ps[k], p[k][mask]), (keep, k)
    _record(test="bits", groups=int(m.F))


def test_more_tasks_than_workgroups_and_every_group_in_a_strip_of_its_own():
    mm = CC.Many()
    th, oth = CC.FAMILIES["spline34"]
    model = _model(mm.Xs, [np.ascontiguousarray(mm.y[i])[:, None] for i in mm.inds], th, "f64", mm.root, "constant")
    Nq = len(mm.Xq)
    group = np.arange(Nq, dtype=np.int32)                          # one query per leaf centre: a strip holds one or a few columns
    a = np.ones(Nq)
    q = _block(model, mm.Xq, mm.RADIUS, mm.DELTA, group, a, mm.wth, th=th)
    Yb, Vb = q.fetch_block()
    p = q.item_blocks()
    assert len(set(p["region"].tolist())) > 256                    # more tasks than compute units
    for j in (0, 88, 89, 300, 511):
        q1 = _block(model, mm.Xq[j:j + 1], mm.RADIUS, mm.DELTA, np.zeros(1, dtype=np.int32), np.ones(1), mm.wth, th=th)
        Y1, V1 = q1.fetch_block()
        assert _bits(Y1[0], Yb[j]) and V1[0] == Vb[j], j
    _record(test="tasks", tasks=len(set(p["region"].tolist())))


# ------------------------------------------------------------------------------------------ past the dense limit
def test_past_the_limit_of_the_dense_covariance():
    mm = CC.Many()
    th, oth = CC.FAMILIES["spline34"]
    model = _model(mm.Xs, [np.ascontiguousarray(mm.y[i])[:, None] for i in mm.inds], th, "f64", mm.root, "constant")
    rng = np.random.default_rng(77)
    centres = mm.Xq[rng.integers(0, len(mm.Xq), 4096)]
    Xq = (centres[:, None, :] + rng.uniform(-0.05, 0.05, (4096, 16, 2))).reshape(-1, 2)
    group = np.repeat(np.arange(4096, dtype=np.int32), 16)
    a = np.full(len(Xq), 1 / 16.0)
    import torch
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.mem_get_info()[0]
    q = _block(model, Xq, mm.RADIUS, mm.DELTA, group, a, mm.wth, th=th)
    Yb, Vb = q.fetch_block()
    owned = before - torch.cuda.mem_get_info()[0]
    assert len(Xq) == 65536 and np.all(np.isfinite(Vb)) and np.all(Vb > 0)
    # the dense route refuses this batch
    d, w = th.desc(), mm.wth.desc()
    L = pmk.lib()
    assert L.pmk_query_items_cov_multi(q.h, C.byref(d)) == -5
    # a sample of 64 groups against long double, on the device's item lists
    off, reg, t = _device_items(q)
    keep = np.sort(rng.choice(4096, 64, replace=False))
    qs = np.nonzero(np.isin(group, keep))[0]
    sub_off = np.concatenate([[0], np.cumsum(np.diff(off)[qs])])
    it = np.concatenate([np.arange(off[j], off[j + 1]) for j in qs])
    sub_group = np.searchsorted(keep, group[qs])
    refs = {r: CMR.TrendRegionRef(oth, mm.Xs[r], SIGMA2["f64"], "constant") for r in sorted(set(reg[it].tolist()))}
    out = BR.block_ref((sub_off, reg[it]), t[it], mm.owth, sub_group, a[qs], 64, refs, Xq[qs], U_OF["f64"])
    var = _worst_ratio(np.abs(np.asarray(np.asarray(Vb[keep], dtype=LD) - out["Var"], dtype=np.float64)), out["unit"])
    pv = BR.plain_block_var((sub_off, reg[it]), t[it], mm.owth, sub_group, a[qs], 64, [oth] * len(mm.Xs), mm.Xs, SIGMA2["f64"],
                            "constant", Xq[qs], np.float64)
    plain = _worst_ratio(np.abs(pv - np.asarray(out["Var"], dtype=np.float64)), out["unit"])
    _record(test="large", queries=int(len(Xq)), groups=4096, var=var, plain=plain, device_bytes_taken_by_the_query=int(owned),
            items=int(off[-1]))
    assert var <= RATIO_MAX, var


# ------------------------------------------------------------------------------------------ failed and flagged patches
def test_a_failed_and_a_flagged_patch_mark_exactly_the_groups_that_blend_them():
    m, items, refs, th, oth, sound = _main_f64()
    Yb, Vb = _block(sound, m.Xq, m.RADIUS, m.DELTA, m.group, m.a, m.wth, th=th).fetch_block()
    diag = [np.zeros(len(x)) for x in m.Xs]
    diag[2][3] = -3.0                                            # the factorisation of this patch fails
    broken = _model(m.Xs, m.Ys(2), th, "f64", m.root, "linear", diag=diag)
    Xs = list(m.Xs)
    Xs[2] = np.ascontiguousarray(Xs[2][:2])                      # n = 2 < q = 3: the trend of this patch is flagged
    flagged = _model(Xs, [CMC.targets(x, 2) for x in Xs], th, "f64", m.root, "linear")
    assert broken.info()[2] != 0 and list(flagged.trend_info()) == [0, 0, 3, 0]
    off, reg = items[0], items[1]
    bad_q = np.array([(reg[off[j]:off[j + 1]] == 2).any() for j in range(len(m.Xq))])
    bad_g = np.zeros(m.F, dtype=bool)
    bad_g[m.group[bad_q]] = True
    assert bad_g.any() and not bad_g.all()
    for what, model in (("failed", broken), ("flagged", flagged)):
        Y, V = _block(model, m.Xq, m.RADIUS, m.DELTA, m.group, m.a, m.wth, th=th).fetch_block()
        assert np.all(np.isnan(V[bad_g])) and np.all(np.isnan(Y[bad_g])) and np.all(np.isfinite(V[~bad_g])), what
        if what == "failed":                                     # the other groups keep the bits of a sound model
            assert _bits(V[~bad_g], Vb[~bad_g]) and _bits(Y[~bad_g], Yb[~bad_g])
    _record(test="failed", groups_marked=int(bad_g.sum()))


# ------------------------------------------------------------------------------------------ refusals and state
def test_refusals_and_state():
    L = pmk.lib()
    m, items, refs, th, oth, model = _main_f64()
    d, w = th.desc(), m.wth.desc()
    Xq = np.ascontiguousarray(m.Xq[:40])
    group = (np.arange(40) // 8).astype(np.int32)
    a = np.ones(40)
    gp, ap = group.ctypes.data_as(C.POINTER(C.c_int32)), M._d(a)

    def refused(q, code, text, th_=d, w_=w, F=5, g=gp):
        assert L.pmk_query_items_block(q.h, None if th_ is None else C.byref(th_), C.byref(w_), F, g, ap, 1) == code
        assert text.encode() in L.pmk_last_error(), L.pmk_last_error()

    q = M.DeviceQuery(model, Xq)
    refused(q, -1, "not planned")
    q.plan(m.RADIUS, m.DELTA)
    refused(q, -2, "pmk_query_items_multi")                                    # no items yet
    q.items_fitted()
    refused(q, -2, "pmk_query_items_multi")                                    # the single-output items
    q.items_multi(th, False)
    ms = pmk.ModulatedSqExpKernelType(2.0, 1.3).desc()
    refused(q, -2, "PMK_MODSQEXP", ms)
    unknown = th.desc()
    unknown.family = 99
    refused(q, -2, "unknown kernel family", unknown)
    bb = pmk.BrownianBridge10(1.0).desc()
    refused(q, -2, "blending profile", d, bb)
    bad = group.copy()
    bad[17] = 1                                                                # below its predecessor
    refused(q, -3, "group[17]", g=bad.ctypes.data_as(C.POINTER(C.c_int32)))
    refused(q, -3, "group[32]", F=4)                                           # group 4 leaves [0, 4)
    buf = np.empty((5, 2), order="F")
    assert L.pmk_query_fetch_block(q.h, M._d(buf), 5, None) == -2              # nothing has run
    # mean only: no variance, no pieces
    q.items_block(group, a, m.wth, theta=th, variance=False)
    Y0, V0 = q.fetch_block()
    assert V0 is None and L.pmk_query_fetch_block(q.h, M._d(buf), 5, M._d(np.empty(5))) == -3
    assert L.pmk_query_get_items_block(q.h, None, None, None, None, None, None, None, None, None) == -2
    assert L.pmk_query_fetch_block(q.h, M._d(buf), 4, None) == -4
    q.items_block(group, a, m.wth, theta=th)
    Y1, V1 = q.fetch_block()
    assert _bits(Y0, Y1)
    # the member cap
    big = M.DeviceQuery(model, np.repeat(m.Xq[:1], 4097, 0))
    big.plan(m.RADIUS, m.DELTA)
    big.items_multi(th, False)
    zeros = np.zeros(4097, dtype=np.int32)
    ones = np.ones(4097)
    assert L.pmk_query_items_block(big.h, C.byref(d), C.byref(w), 1, zeros.ctypes.data_as(C.POINTER(C.c_int32)), M._d(ones), 1) == -5
    assert b"group 0" in L.pmk_last_error() and b"region" in L.pmk_last_error()
    # a trend change without new items, a stale solve, new items, a new plan, a change of R on one query
    model.set_trend("constant")
    refused(q, -3, "pmk_model_solve_multi")
    model.solve_multi()
    refused(q, -2, "trend")
    q.items_multi(th, False)
    assert L.pmk_query_fetch_block(q.h, M._d(buf), 5, None) == -2              # new items discarded the results
    q.items_block(group, a, m.wth, theta=th)
    model.set_targets_multi(m.Ys(3))
    model.solve_multi()
    q.items_multi(th, False)
    q.items_block(group, a, m.wth, theta=th)
    Y3, V3 = q.fetch_block()
    assert Y3.shape == (5, 3) and np.all(np.isfinite(Y3)) and np.all(V3 > 0)
    q.plan(m.RADIUS, m.DELTA)
    assert L.pmk_query_fetch_block(q.h, M._d(np.empty((5, 3), order="F")), 5, None) == -2
    # the one-shot and the front end agree with the staged calls
    Yo, Vo = np.empty((5, 3), order="F"), np.empty(5)
    assert L.pmk_predict_mixture_block_fitted(model.h, C.byref(w), 40, M._d(Xq), m.RADIUS, m.DELTA, 5, gp, ap, M._d(Yo), 5,
                                              M._d(Vo)) == 0
    assert _bits(Yo, Y3) and _bits(Vo, V3)
    # a query of explicit items belongs to no blend
    region = np.zeros(40, dtype=np.int32)
    qe = M.DeviceQuery.from_items(model, 40, Xq.ctypes.data_as(C.c_void_p), region.ctypes.data_as(C.c_void_p))
    qe.items_multi(th, False)
    refused(qe, -2, "pmk_query_create_items")
    # a model of factors holds no kernels until it is given them
    loaded = M.DeviceModel.from_factors(m.Xs, model.weights(), [model.get(r, M.GET_L) for r in range(4)])
    loaded.set_bsp(m.root, 0)
    loaded.set_targets_multi(m.Ys(2))
    loaded.set_trend("linear")
    loaded.solve_multi()
    ql = M.DeviceQuery(loaded, Xq)
    ql.plan(m.RADIUS, m.DELTA)
    ql.items_multi(th, False)
    refused(ql, -3, "holds no kernels", None)
    # no resident factor
    unfit = M.DeviceModel(m.Xs, [np.ascontiguousarray(y[:, 0]) for y in m.Ys(1)])
    unfit.set_bsp(m.root, 0)
    qu = M.DeviceQuery(unfit, Xq)
    qu.plan(m.RADIUS, m.DELTA)
    refused(qu, -1, "resident factor")
    # the one-shot on a shard of the leaves
    shard = M.DeviceModel(m.Xs[2:], [np.ascontiguousarray(y[:, 0]) for y in m.Ys(1)[2:]])
    shard.fit(th, SIGMA2["f64"])
    shard.set_bsp(m.root, 2)
    assert L.pmk_predict_mixture_block_fitted(shard.h, C.byref(w), 40, M._d(Xq), m.RADIUS, m.DELTA, 5, gp, ap, M._d(Yo), 5,
                                              M._d(Vo)) == -3 and b"every leaf" in L.pmk_last_error()
    # a stage that was refused leaves its timer closed: the next run is timed
    ctx = pmk.default_context()
    ctx.enable_timers(True)
    big.items_multi(th, False)                                                 # the model's trend has changed since
    assert L.pmk_query_items_block(big.h, C.byref(d), C.byref(w), 1, zeros.ctypes.data_as(C.POINTER(C.c_int32)), M._d(ones), 1) == -5
    q.items_multi(th, False)
    q.items_block(group, a, m.wth, theta=th)
    q.fetch_block()
    assert ctx.timer_ms("items_block") > 0
    ctx.enable_timers(False)
    _record(test="state", refusals=17)


def test_the_front_end_on_a_list_built_and_a_tree_built_eta():
    m, items, refs, _ = main_case("f64", "spline34", "linear")
    th = CC.FAMILIES["spline34"][0]
    eta = pmk.MixtureGPType(m.Xs, pmk.fetchhyperplanes(m.root))
    pmk.fitmixtureGP_trend_(eta, m.Ys(2), th, SIGMA2["f64"], "linear")
    Yb, Vb = pmk.querymixtureGP_block(m.Xq, m.group, m.a, eta, m.root, m.LEVELS, m.RADIUS, m.DELTA, m.wth)
    out = BR.block_ref(items[:2], items[2], m.owth, m.group, m.a, m.F, refs, m.Xq, U_OF["f64"])
    var = _worst_ratio(np.abs(np.asarray(np.asarray(Vb, dtype=LD) - out["Var"], dtype=np.float64)), out["unit"])
    assert Yb.shape == (m.F, 2) and var <= RATIO_MAX, var
    Ym, none = pmk.querymixtureGP_block(m.Xq, m.group, m.a, eta, m.root, m.LEVELS, m.RADIUS, m.DELTA, m.wth, variance=False)
    assert none is None and _bits(Ym, Yb)
    # the same points through a tree-built eta: its patches hold the points in another order, so units, not bits
    tree = pmk.MixtureGPType.from_tree(m.root, m.X, eps=m.EPS)
    pmk.fitmixtureGP_trend_(tree, np.asfortranarray(CMC.targets(m.X, 2)), th, SIGMA2["f64"], "linear")
    Yt, Vt = pmk.querymixtureGP_block(m.Xq, m.group, m.a, tree, m.root, m.LEVELS, m.RADIUS, m.DELTA, m.wth)
    tvar = _worst_ratio(np.abs(np.asarray(np.asarray(Vt, dtype=LD) - out["Var"], dtype=np.float64)), out["unit"])
    assert Yt.shape == Yb.shape and np.allclose(Yt, Yb, rtol=1e-9, atol=1e-9) and tvar <= RATIO_MAX, tvar
    _record(test="front_end", var=var, tree_var=tvar)
