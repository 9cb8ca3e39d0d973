"""Joint covariance of a query batch under the blend on the GPU (pmk_query_items_cov / _mix_cov / _fetch_cov /
_get_items_cov, pmk_predict_mixture_cov_fitted; the kernels of pmk_cov.hip) and the posterior draws built on it.

Reference: tests/_cov_refs.py, the numpy.longdouble restatement that tests/test_cov_refs.py pins to the oracle.  The error
unit of a block entry is that of _cov_refs.py,
    e(a, b) = (n + 32) u kappa2(L) (k0 + |V_a| |V_b|),   u = 2^-53 (fp64) or 2^-24 (fp32),
the unit of a blended entry the wn-weighted sum of its regions' units, and every ratio err / unit must stay <= 10.
tests/test_cov_refs.py checks on the same inputs (tests/_cov_cases.py) that a plain numpy / LAPACK evaluation in the
model's precision stays below one unit and that kappa2(L) <= 10^3 for every patch.

A tree of `levels` has 2^(levels - 1) leaves in this package: the four leaves of the main workload are levels = 3, the 512
leaves of the task-loop case levels = 10.

Every measured ratio is printed ("COV {json}", run with -s) and a run of the whole module writes the worst ratios to
profiles/cov_accuracy.json.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
from patchmixturekriging_amd import mixture as M
import _cov_cases as CC
import _cov_refs as CR
import _vgrad_edge_cases as VE
from test_gpu_grad import _explicit_query, _tree8, _worst_ratio

pytestmark = pytest.mark.gpu

U_OF, SIGMA2, RATIO_MAX = CC.U_OF, CC.SIGMA2, CC.RATIO_MAX
_RECORDS = []
ACCURACY_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cov_accuracy.json")


def _record(**kw):
    _RECORDS.append(kw)
    print("COV " + json.dumps(kw, sort_keys=True))


@pytest.fixture(scope="module", autouse=True)
def _write_accuracy_file():
    """only a run of the whole module replaces the file"""
    yield
    if {r["test"] for r in _RECORDS} >= {"main", "edges", "many", "mixed", "bb10", "diag", "state", "sample"}:
        with open(ACCURACY_JSON, "w") as f:
            f.write("[\n" + ",\n".join(" " + json.dumps(r, sort_keys=True) for r in _RECORDS) + "\n]\n")


_MAIN, _REFS = {}, {}


def _main(dtype):
    if dtype not in _MAIN:
        _MAIN[dtype] = CC.Main(dtype)
    return _MAIN[dtype]


def _ref(key, oth, X, sigma2):
    """the long-double factor of one patch, built once per process"""
    if key not in _REFS:
        _REFS[key] = CR.RegionRef(oth, X, sigma2)
    return _REFS[key]


def _fitted(Xs, ys, th, dtype, root):
    model = M.DeviceModel(Xs, ys, dtype=dtype)
    if isinstance(th, list):
        model.fit_patches(th, [SIGMA2[dtype]] * len(Xs))
    else:
        model.fit(th, SIGMA2[dtype])
    model.set_bsp(root, 0)
    return model


def _main_model(m, th, dtype):
    return _fitted(m.Xs, [np.ascontiguousarray(m.y[i]) for i in m.inds], th, dtype, m.root)


def _device_blocks(q, P):
    out = {}
    for r in range(P):
        idx, S = q.item_covs(r)
        if len(idx):
            out[r] = (idx.astype(np.int64), S)
    return out


def _check_blocks(blocks, points, refs, dtype, addend=None):
    """worst err / unit of the device blocks against the reference; -> (worst, kappa, reference blocks, units)"""
    worst = kappa = 0.0
    S_ref, units = {}, {}
    for r, (idx, S) in blocks.items():
        assert np.all(np.diff(idx) >= 0), r                      # rows in ascending query index (a query may hold two items)
        assert np.array_equal(S, S.T), r                         # symmetric bit for bit
        out = refs[r].cov(points[idx], None if addend is None else addend[idx])
        assert not out["clamped"].any()
        unit = (refs[r].n + 32) * U_OF[dtype] * out["unit"]
        err = np.abs(np.asarray(S, dtype=CR.LD) - out["S"]).astype(np.float64)
        worst = max(worst, _worst_ratio(err, unit))
        kappa = max(kappa, refs[r].kappa)
        S_ref[r], units[r] = (idx, out["S"]), unit
    return worst, kappa, S_ref, units


def _staged(model, Xq, radius, delta, th, wth, fitted=False):
    q = M.DeviceQuery(model, Xq)
    q.plan(radius, delta)
    q.items_fitted() if fitted else q.items(th)
    q.mix(wth)
    q.items_cov(None if fitted else th)
    q.mix_cov(wth)
    return q


# ------------------------------------------------------------------------------------------ the main workload
@pytest.mark.parametrize("family,dtype", [("spline34", "f64"), ("gaussian", "f64"), ("spline34", "f32")])
def test_blocks_blend_bits_and_the_one_shot(family, dtype):
    m = _main(dtype)
    th, oth = CC.FAMILIES[family]
    model = _main_model(m, th, dtype)
    assert np.all(model.info() == 0)
    q = _staged(model, m.Xq, m.RADIUS, m.DELTA, th, m.wth)
    counts = np.diff(q.region_offsets(4))
    assert counts.max() > 2 * CC.TQ and counts.min() < CC.TQ, counts           # three strips in one region, one in another
    dbg = q.debug()
    per_query = np.diff(dbg["item_offsets"])
    assert per_query.min() >= 1 and per_query.max() <= 3 and (per_query > 1).sum() > 100
    Yq, Vq = q.fetch()
    Cov = q.fetch_cov()
    refs = {r: _ref(("main", family, dtype, r), oth, m.Xs[r], SIGMA2[dtype]) for r in range(4)}
    blocks = _device_blocks(q, 4)
    assert [len(blocks[r][0]) for r in range(4)] == list(counts)
    worst, kappa, S_ref, units = _check_blocks(blocks, m.Xq, refs, dtype)
    items = (dbg["item_offsets"], dbg["item_region"])
    ref_cov, unit = CR.mix_cov_ref(items, S_ref, dbg["item_t"], m.owth, units)
    blend = _worst_ratio(np.abs(np.asarray(Cov, dtype=CR.LD) - ref_cov).astype(np.float64), unit)
    diag = _worst_ratio(np.abs(np.diag(Cov) - Vq), np.diag(unit))
    _record(test="main", family=family, dtype=dtype, blocks=worst, blend=blend, diag_vs_vq=diag, kappa=kappa,
            region_items=[int(c) for c in counts])
    assert kappa <= CC.KAPPA_MAX and worst <= RATIO_MAX and blend <= RATIO_MAX and diag <= RATIO_MAX, (kappa, worst, blend, diag)
    assert np.array_equal(Cov, Cov.T)                                          # symmetric bit for bit
    shared = CR.shared_region_mask(items)
    assert not shared.all() and np.all(Cov[~shared] == 0) and not np.signbit(Cov[~shared]).any()
    # a second run gives identical bits
    q.items_cov(th)
    q.mix_cov(m.wth)
    assert np.array_equal(q.fetch_cov(), Cov)
    for r, (idx, S) in _device_blocks(q, 4).items():
        assert np.array_equal(S, blocks[r][1])
    # the one-shot (the model's own kernels) equals the staged calls bit for bit
    Nq = len(m.Xq)
    Y1, V1, C1 = np.empty(Nq), np.empty(Nq), np.full((Nq, Nq + 3), -7.0)
    w = m.wth.desc()
    Xc = np.ascontiguousarray(m.Xq)
    _lib.check(pmk.lib().pmk_predict_mixture_cov_fitted(model.h, C.byref(w), Nq, M._d(Xc), m.RADIUS, m.DELTA, M._d(Y1), M._d(V1),
                                                        M._d(C1), Nq + 3), "pmk_predict_mixture_cov_fitted")
    assert np.array_equal(Y1, Yq) and np.array_equal(V1, Vq) and np.array_equal(C1[:, :Nq], Cov) and np.all(C1[:, Nq:] == -7.0)
    # with Cov NULL no covariance stage runs; the means and variances are the same
    Y2, V2 = np.empty(Nq), np.empty(Nq)
    _lib.check(pmk.lib().pmk_predict_mixture_cov_fitted(model.h, C.byref(w), Nq, M._d(Xc), m.RADIUS, m.DELTA, M._d(Y2), M._d(V2),
                                                        None, 0), "pmk_predict_mixture_cov_fitted")
    assert np.array_equal(Y2, Yq) and np.array_equal(V2, Vq)


def test_an_entry_keeps_its_bits_in_a_sub_batch():
    m = _main("f64")
    th, _ = CC.FAMILIES["spline34"]
    model = _main_model(m, th, "f64")
    q = _staged(model, m.Xq, m.RADIUS, m.DELTA, th, m.wth)
    idx, S = q.item_covs(0)
    assert len(idx) > 2 * CC.TQ
    Cov = q.fetch_cov()
    # the first and the last item of the region: the first and the third strip of the full batch
    for a, b in ((0, len(idx) - 1), (3, len(idx) // 2), (len(idx) // 2 - 1, len(idx) // 2)):
        ja, jb = int(idx[a]), int(idx[b])
        others = [j for j in (5, 77, 300, 411, 650) if j not in (ja, jb)][:3]
        sub = [others[0], jb, others[1], ja, others[2]]
        q2 = _staged(model, m.Xq[sub], m.RADIUS, m.DELTA, th, m.wth)
        idx2, S2 = q2.item_covs(0)
        pa, pb = list(idx2).index(3), list(idx2).index(1)
        assert S2[pa, pb] == S[a, b] and S2[pb, pa] == S[b, a] and S2[pa, pa] == S[a, a] and S2[pb, pb] == S[b, b]
        assert q2.fetch_cov()[3, 1] == Cov[ja, jb]


# ------------------------------------------------------------------------------------------ strip and patch edges
def _edge_run(D, dtype, th, fit_th, oths, set_addend=False):
    Xs = CC.edge_patches(D, dtype)
    xq, region = CC.edge_items(Xs, CC.EDGE_COUNTS, dtype)
    model = _fitted(Xs, [np.sin(X[:, 0]) for X in Xs], fit_th, dtype, _tree8(D))
    assert np.all(model.info() == 0)
    q = _explicit_query(model, xq, region)
    addend = None
    if set_addend:
        addend = np.random.default_rng(5).uniform(0.0, 0.5, len(xq))
        q.set_diag(addend)
    q.items_cov(th)
    blocks = _device_blocks(q, 8)
    for r, c in enumerate(CC.EDGE_COUNTS):
        assert (len(blocks[r][0]) if r in blocks else 0) == c
        if c:
            assert np.array_equal(blocks[r][0], np.nonzero(region == r)[0])    # the returned query index list
    refs = {r: _ref(("edge", D, dtype, oths[r].family, r), oths[r], Xs[r], SIGMA2[dtype]) for r in blocks}
    worst, kappa, _, _ = _check_blocks(blocks, xq, refs, dtype, addend)
    return worst, kappa, blocks, q


@pytest.mark.parametrize("D,dtype", [(2, "f64"), (2, "f32"), (3, "f64")])
def test_strip_and_patch_edges_through_explicit_items(D, dtype):
    th, oth = CC.FAMILIES["spline34"]
    worst, kappa, blocks, q = _edge_run(D, dtype, th, th, [oth] * 8)
    _record(test="edges", D=D, dtype=dtype, blocks=worst, kappa=kappa)
    assert kappa <= CC.KAPPA_MAX and worst <= RATIO_MAX, (kappa, worst)
    # an empty region answers m = 0; the blend of explicit items is refused
    idx, S = q.item_covs(5)
    assert len(idx) == 0 and S.shape == (0, 0)
    w = th.desc()
    assert pmk.lib().pmk_query_mix_cov(q.h, C.byref(w)) == -2


def test_mixed_families_per_patch_and_the_models_own_kernels():
    names = CC.MIXED_NAMES
    for dtype in ("f64", "f32"):
        worst, kappa, _, _ = _edge_run(2, dtype, None, [CC.FAMILIES[n][0] for n in names], [CC.FAMILIES[n][1] for n in names])
        _record(test="mixed", dtype=dtype, blocks=worst, kappa=kappa)
        assert kappa <= CC.KAPPA_MAX and worst <= RATIO_MAX, (kappa, worst)
    # every patch Spline34 through fit_patches: the per-patch instantiation equals the uniform one bit for bit
    th, oth = CC.FAMILIES["spline34"]
    _, _, uniform, _ = _edge_run(2, "f64", th, th, [oth] * 8)
    _, _, own, _ = _edge_run(2, "f64", None, [th] * 8, [oth] * 8)
    for r in uniform:
        assert np.array_equal(uniform[r][1], own[r][1]), r


def test_brownian_bridge_at_one_dimension():
    th, oth = CC.FAMILIES["bb10"]
    Xs = CC.bb_patches()
    xq, region = CC.bb_items()
    model = _fitted(Xs, [np.sin(3 * X[:, 0]) for X in Xs], th, "f64", _tree8(1))
    assert np.all(model.info() == 0)
    q = _explicit_query(model, xq, region)
    q.items_cov(th)
    blocks = _device_blocks(q, 8)
    refs = {r: _ref(("bb", r), oth, Xs[r], SIGMA2["f64"]) for r in blocks}
    worst, kappa, _, _ = _check_blocks(blocks, xq, refs, "f64")
    _record(test="bb10", blocks=worst, kappa=kappa)
    assert kappa <= CC.KAPPA_MAX and worst <= RATIO_MAX, (kappa, worst)


def test_set_diag_addends_appear_on_block_diagonals_only():
    th, oth = CC.FAMILIES["spline34"]
    worst, kappa, with_addend, _ = _edge_run(2, "f64", th, th, [oth] * 8, set_addend=True)
    _, _, plain, _ = _edge_run(2, "f64", th, th, [oth] * 8)
    _record(test="diag", blocks=worst, kappa=kappa)
    assert worst <= RATIO_MAX, worst
    for r in plain:
        a, b = with_addend[r][1], plain[r][1]
        off = ~np.eye(len(a), dtype=bool)
        assert np.array_equal(a[off], b[off]) and np.all(np.diag(a) > np.diag(b))


def test_more_tasks_than_workgroups():
    mm = CC.Many()
    th, oth = CC.FAMILIES["spline34"]
    P = len(mm.Xs)
    assert P == 512
    model = _fitted(mm.Xs, [np.ascontiguousarray(mm.y[i]) for i in mm.inds], th, "f64", mm.root)
    assert np.all(model.info() == 0)
    q = _staged(model, mm.Xq, mm.RADIUS, mm.DELTA, th, mm.wth)
    counts = np.diff(q.region_offsets(P))
    assert (counts > 0).sum() > 304                              # more strips than any chip has compute units
    blocks = _device_blocks(q, P)
    refs = {r: _ref(("many", r), oth, mm.Xs[r], SIGMA2["f64"]) for r in blocks}
    worst, kappa, S_ref, units = _check_blocks(blocks, mm.Xq, refs, "f64")
    dbg = q.debug()
    ref_cov, unit = CR.mix_cov_ref((dbg["item_offsets"], dbg["item_region"]), S_ref, dbg["item_t"], mm.owth, units)
    Cov = q.fetch_cov()
    blend = _worst_ratio(np.abs(np.asarray(Cov, dtype=CR.LD) - ref_cov).astype(np.float64), unit)
    doubled = [int(r) for r, (idx, _) in blocks.items() if np.any(np.diff(idx) == 0)]
    assert doubled                                                   # a query with two items of one region: every pair counts
    _record(test="many", blocks=worst, blend=blend, kappa=kappa, strips=int((counts > 0).sum()), doubled_regions=doubled)
    assert kappa <= CC.KAPPA_MAX and worst <= RATIO_MAX and blend <= RATIO_MAX, (kappa, worst, blend)
    assert np.array_equal(Cov, Cov.T)


# ------------------------------------------------------------------------------------------ clamp, failed patch
def test_the_clamp_holds_on_the_block_diagonal_only():
    th, _ = CC.FAMILIES["spline34"]
    Xs, xq, region, kind = VE.b_inputs("spline34", "f64")
    s2 = [SIGMA2["f64"]] * 8
    s2[VE.B_PATCH] = VE.B_SIGMA2["f64"]
    model = M.DeviceModel(Xs, [np.sin(X[:, 0]) for X in Xs], dtype="f64")
    model.fit_patches([th] * 8, s2)
    model.set_bsp(_tree8(2), 0)
    assert np.all(model.info() == 0)
    q = _explicit_query(model, xq, region)
    q.items_cov()
    idx, S = q.item_covs(VE.B_PATCH)
    assert np.array_equal(idx, np.nonzero(region == VE.B_PATCH)[0])
    d = np.diag(S)
    assert np.array_equal(d == VE.MIN_V, kind == VE.CLAMPED), d
    assert np.all(d[kind == VE.OUTSIDE] == 1.0)
    off = S[~np.eye(len(S), dtype=bool)]
    # unclamped: queries at different lattice points have covariance 0, below min_v, and none sits on the clamp value
    assert np.all(np.isfinite(off)) and np.any(off < VE.MIN_V) and np.all(off != VE.MIN_V)
    assert np.array_equal(S, S.T)


def test_failed_patch_gives_nan_and_the_rest_keep_their_bits():
    m = _main("f64")
    th, _ = CC.FAMILIES["spline34"]
    sound = _main_model(m, th, "f64")
    broken = M.DeviceModel(m.Xs, [np.ascontiguousarray(m.y[i]) for i in m.inds], dtype="f64")
    diag = [np.zeros(len(x)) for x in m.Xs]
    diag[2][3] = -3.0                                            # the factorisation of this patch fails (tests/test_gpu_breakdown.py)
    broken.set_diag(diag)
    broken.fit(th, SIGMA2["f64"])
    broken.set_bsp(m.root, 0)
    assert broken.info()[2] != 0 and np.all(np.delete(broken.info(), 2) == 0)
    qs = _staged(sound, m.Xq, m.RADIUS, m.DELTA, th, m.wth)
    qb = _staged(broken, m.Xq, m.RADIUS, m.DELTA, th, m.wth)
    for r in range(4):
        Ss, Sb = qs.item_covs(r)[1], qb.item_covs(r)[1]
        assert np.all(np.isnan(Sb)) if r == 2 else np.array_equal(Sb, Ss), r
    dbg = qb.debug()
    reg, off = dbg["item_region"], dbg["item_offsets"]
    bad_q = np.array([(reg[off[j]:off[j + 1]] == 2).any() for j in range(len(m.Xq))])
    assert bad_q.any() and not bad_q.all()
    Cs, Cb = qs.fetch_cov(), qb.fetch_cov()
    bad = bad_q[:, None] | bad_q[None, :]
    assert np.all(np.isnan(Cb[bad])) and np.array_equal(Cb[~bad], Cs[~bad])


# ------------------------------------------------------------------------------------------ state
def _blend_ratio(q, m, refs, dtype="f64"):
    P = len(m.Xs)
    worst, _, S_ref, units = _check_blocks(_device_blocks(q, P), q.Xq, refs, dtype)
    dbg = q.debug()
    ref_cov, unit = CR.mix_cov_ref((dbg["item_offsets"], dbg["item_region"]), S_ref, dbg["item_t"], m.owth, units)
    return worst, _worst_ratio(np.abs(np.asarray(q.fetch_cov(), dtype=CR.LD) - ref_cov).astype(np.float64), unit)


def test_a_new_plan_discards_the_results_and_arenas_are_reused():
    m = _main("f64")
    th, oth = CC.FAMILIES["spline34"]
    model = _main_model(m, th, "f64")
    refs = {r: _ref(("main", "spline34", "f64", r), oth, m.Xs[r], SIGMA2["f64"]) for r in range(4)}
    L = pmk.lib()
    w = m.wth.desc()
    buf = np.empty((len(m.Xq), len(m.Xq)))
    q = _staged(model, m.Xq, 0.3, m.DELTA, th, m.wth)
    small_total = q.total
    first = q.fetch_cov()
    # a larger radius: more items, the arenas grow; the results are gone until the stages have rerun
    q.plan(m.RADIUS, m.DELTA)
    assert q.total > small_total
    assert L.pmk_query_fetch_cov(q.h, M._d(buf), len(m.Xq)) == -2
    assert L.pmk_query_mix_cov(q.h, C.byref(w)) == -2
    assert L.pmk_query_get_items_cov(q.h, 0, None, None, None, 0) == -2
    q.items(th); q.mix(m.wth); q.items_cov(th)
    assert L.pmk_query_fetch_cov(q.h, M._d(buf), len(m.Xq)) == -2
    q.mix_cov(m.wth)
    grown = _blend_ratio(q, m, refs)
    # a smaller plan after the larger one: stale arena rows and columns do not leak
    q.plan(0.3, m.DELTA)
    assert q.total == small_total
    q.items(th); q.mix(m.wth); q.items_cov(th); q.mix_cov(m.wth)
    again = q.fetch_cov()
    shrunk = _blend_ratio(q, m, refs)
    _record(test="state", grown_blocks=grown[0], grown_blend=grown[1], shrunk_blocks=shrunk[0], shrunk_blend=shrunk[1])
    assert max(grown + shrunk) <= RATIO_MAX, (grown, shrunk)
    assert np.array_equal(again, first)


def test_refusals():
    L = pmk.lib()
    m = _main("f64")
    th, _ = CC.FAMILIES["spline34"]
    d, w = th.desc(), m.wth.desc()
    model = _main_model(m, th, "f64")
    Xq = m.Xq[:40]
    buf = np.empty((40, 40))
    q = M.DeviceQuery(model, Xq)
    assert L.pmk_query_items_cov(q.h, C.byref(d)) == -1                      # no plan
    assert L.pmk_query_get_items_cov(q.h, 0, None, None, None, 0) == -1
    q.plan(m.RADIUS, m.DELTA)
    assert L.pmk_query_mix_cov(q.h, C.byref(w)) == -2                        # before items_cov
    assert L.pmk_query_get_items_cov(q.h, 0, None, None, None, 0) == -2
    assert L.pmk_query_fetch_cov(q.h, M._d(buf), 40) == -2                   # before mix_cov
    ms = pmk.ModulatedSqExpKernelType(2.0, 1.3).desc()
    assert L.pmk_query_items_cov(q.h, C.byref(ms)) == -2                     # PMK_MODSQEXP with D > 1
    assert b"PMK_MODSQEXP" in L.pmk_last_error()
    q.items_cov(th)
    assert L.pmk_query_fetch_cov(q.h, M._d(buf), 40) == -2
    assert L.pmk_query_fetch_cov_dev(q.h, None, 40) == -2
    assert L.pmk_query_get_items_cov(q.h, 4, None, None, None, 0) == -3      # not a leaf of the model
    bb = pmk.BrownianBridge10(1.0).desc()
    assert L.pmk_query_mix_cov(q.h, C.byref(bb)) == -2                       # the blending profile is stationary
    q.mix_cov(m.wth)
    assert L.pmk_query_fetch_cov(q.h, M._d(buf), 39) == -4 and L.pmk_query_fetch_cov(q.h, None, 40) == -2
    assert L.pmk_query_fetch_cov(q.h, M._d(buf), 40) == 0
    # a Brownian-bridge theta is admitted: nothing here differentiates
    assert L.pmk_query_items_cov(q.h, C.byref(bb)) == 0
    # no resident factor
    unfit = M.DeviceModel(m.Xs, [np.ascontiguousarray(m.y[i]) for i in m.inds])
    unfit.set_bsp(m.root, 0)
    qu = M.DeviceQuery(unfit, Xq)
    qu.plan(m.RADIUS, m.DELTA)
    assert L.pmk_query_items_cov(qu.h, C.byref(d)) == -1
    # a model of factors holds no kernels until it is given them; then it serves (a resident factor is all it needs)
    loaded = M.DeviceModel.from_factors(m.Xs, model.weights(), [model.get(r, M.GET_L) for r in range(4)])
    loaded.set_bsp(m.root, 0)
    ql = M.DeviceQuery(loaded, Xq)
    ql.plan(m.RADIUS, m.DELTA)
    assert L.pmk_query_items_cov(ql.h, None) == -3
    assert L.pmk_predict_mixture_cov_fitted(loaded.h, C.byref(w), 40, M._d(np.ascontiguousarray(Xq)), m.RADIUS, m.DELTA, None, None,
                                            M._d(buf), 40) == -3
    loaded.set_kernels([th] * 4)
    ql.items_cov()
    q.items_cov(th)
    for r in range(4):
        a, b = ql.item_covs(r), q.item_covs(r)
        assert np.array_equal(a[0], b[0]) and np.allclose(a[1], b[1], rtol=0, atol=1e-9)
    # a shard of the leaves
    shard = M.DeviceModel(m.Xs[2:], [np.ascontiguousarray(m.y[i]) for i in m.inds[2:]])
    shard.fit(th, SIGMA2["f64"])
    shard.set_bsp(m.root, 2)
    qs = M.DeviceQuery(shard, Xq)
    qs.plan(m.RADIUS, m.DELTA)
    assert L.pmk_query_items_cov(qs.h, C.byref(d)) == -3
    assert L.pmk_predict_mixture_cov_fitted(shard.h, C.byref(w), 40, M._d(np.ascontiguousarray(Xq)), m.RADIUS, m.DELTA, None, None,
                                            M._d(buf), 40) == -3
    # more queries than the limit, before any launch
    big = np.random.default_rng(3).uniform(-3.9, 3.9, (16385, 2))
    qb = M.DeviceQuery(model, big)
    qb.plan(0.0, m.DELTA)
    assert L.pmk_query_items_cov(qb.h, C.byref(d)) == -5
    assert b"PMK_COV_MAX_QUERIES" in L.pmk_last_error()
    assert L.pmk_predict_mixture_cov_fitted(model.h, C.byref(w), 16385, M._d(big), 0.0, m.DELTA, None, None, M._d(buf), 16385) == -5
    assert L.pmk_predict_mixture_cov_fitted(model.h, C.byref(w), 40, M._d(np.ascontiguousarray(Xq)), m.RADIUS, m.DELTA, None, None,
                                            M._d(buf), 39) == -4
    # an explicit query: items_cov and get_items_cov serve, mix_cov does not
    xe = np.ascontiguousarray(Xq[:6])
    qe = _explicit_query(model, xe, np.array([0, 0, 1, 3, 3, 3], dtype=np.int32))
    assert L.pmk_query_mix_cov(qe.h, C.byref(w)) == -2
    qe.items_cov(th)
    assert [len(qe.item_covs(r)[0]) for r in range(4)] == [2, 1, 0, 3]
    assert L.pmk_query_mix_cov(qe.h, C.byref(w)) == -2


# ------------------------------------------------------------------------------------------ posterior draws
def test_posterior_draws():
    import torch
    m = _main("f64")
    th, _ = CC.FAMILIES["spline34"]
    eta = pmk.MixtureGPType(m.Xs, pmk.fetchhyperplanes(m.root))
    pmk.fitmixtureGP_(eta, [np.ascontiguousarray(m.y[i]) for i in m.inds], th, SIGMA2["f64"])
    # eight queries that share regions: around the corner where the four leaves meet, at distinct places
    rng = np.random.default_rng(9)
    centre = np.mean([x.mean(0) for x in m.Xs], 0)
    Xq = centre + rng.uniform(-0.5, 0.5, (8, 2))
    args = (Xq, eta, m.root, m.LEVELS, m.RADIUS, m.DELTA, m.wth)
    Yq, Vq, Cov = pmk.querymixtureGP_cov(*args)
    Y0, V0, _ = pmk.querymixtureGP_patches(*args)
    assert np.array_equal(Yq, Y0) and np.array_equal(Vq, V0) and np.array_equal(Cov, Cov.T)
    assert (np.abs(Cov[~np.eye(8, dtype=bool)]) > 0).sum() >= 20               # the queries share regions
    n = 4096
    dev = torch.device("cuda", 0)
    draws, jitter = pmk.samplemixtureGP(*args, n, generator=torch.Generator(device=dev).manual_seed(17))
    again, _ = pmk.samplemixtureGP(*args, n, generator=torch.Generator(device=dev).manual_seed(17))
    assert jitter == 0.0 and tuple(draws.shape) == (n, 8) and torch.equal(draws, again)
    # with z passed in, draws - Yq is z L^T with L L^T = Cov + jitter I
    z = torch.randn((n, 8), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    dz, jz = pmk.samplemixtureGP(*args, n, z=z)
    assert jz == 0.0
    Lt = torch.linalg.lstsq(z, dz - torch.as_tensor(Yq, device=dev)[None, :]).solution          # L^T, from n >> 8 equations
    LLt = (Lt.T @ Lt).cpu().numpy()
    assert np.allclose(np.triu(Lt.cpu().numpy().T, 1), 0.0, atol=1e-9)                          # L is lower triangular
    # L L^T = Cov to 10 units of the blended entries, plus what a Cholesky in double of an 8 x 8 matrix and the recovery
    # of L from z may add: 9 u sqrt(C_ii C_jj) each (Higham, Accuracy and Stability, Thm 10.3), also where two queries share
    # no region and the unit is zero
    q = _staged(eta._model, Xq, m.RADIUS, m.DELTA, th, m.wth, fitted=True)
    assert np.array_equal(q.fetch_cov(), Cov)
    oth = CC.FAMILIES["spline34"][1]
    refs = {r: _ref(("main", "spline34", "f64", r), oth, m.Xs[r], SIGMA2["f64"]) for r in range(4)}
    _, _, S_ref, units = _check_blocks(_device_blocks(q, 4), Xq, refs, "f64")
    dbg = q.debug()
    _, unit = CR.mix_cov_ref((dbg["item_offsets"], dbg["item_region"]), S_ref, dbg["item_t"], m.owth, units)
    bound = RATIO_MAX * unit + 2 * 9 * U_OF["f64"] * np.sqrt(np.outer(np.diag(Cov), np.diag(Cov)))
    ratio = RATIO_MAX * float((np.abs(LLt - Cov) / bound).max())
    # the sample covariance within 6 standard errors, entry by entry
    x = draws.cpu().numpy() - Yq[None, :]
    samp = x.T @ x / n
    se = np.sqrt((np.outer(np.diag(Cov), np.diag(Cov)) + Cov ** 2) / n)
    z_worst = float((np.abs(samp - Cov) / se).max())
    _record(test="sample", llt_ratio=ratio, worst_standard_errors=z_worst, jitter=jitter)
    assert ratio <= RATIO_MAX and z_worst <= 6.0, (ratio, z_worst)
