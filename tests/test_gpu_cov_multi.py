"""Joint covariance of a query batch on the multi-output path on the GPU, under a trend and for R target columns
(pmk_query_items_cov_multi, pmk_predict_mixture_cov_multi_fitted; the kernels of pmk_cov_trend.hip) and the draws of the R
columns built on it (querymixtureGP_cov_multi, samplemixtureGP_multi).

Reference: tests/_cov_multi_refs.py, the numpy.longdouble restatement that tests/test_cov_multi_refs.py pins to the dense
saddle-point form and to tests/_trend_refs.py.  The error unit of a block entry is
    (n + 32) u [ kappa2(L) (k0 + |V_a| |V_b|) + |dz_a| |z_b| + |z_a| |dz_b| ],
    |dz| = kappa2(U) |L_G^-1|_2 (|h| + | |C_H|^T |kq| |),   u = 2^-53 (fp64) or 2^-24 (fp32),
the unit of a blended entry the wn-weighted sum of its regions' units, and every ratio err / unit must stay <= 10, measured
against the long-double reference.  tests/test_cov_multi_refs.py checks on the same inputs (tests/_cov_multi_cases.py) that a
plain numpy / LAPACK evaluation in the model's precision stays below one unit and that kappa2(L) <= 10^3 for every patch.

Every measured ratio is printed ("COVM {json}", run with -s) and a run of the whole module writes them to
profiles/cov_multi_accuracy.json.
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
import _cov_multi_cases as CMC
import _cov_multi_refs as CMR
import _cov_refs as CR
from test_gpu_cov import _check_blocks, _device_blocks
from test_gpu_grad import _explicit_query, _tree8, _worst_ratio

pytestmark = pytest.mark.gpu

U_OF, SIGMA2, RATIO_MAX = CC.U_OF, CC.SIGMA2, CC.RATIO_MAX
_RECORDS = []
ACCURACY_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cov_multi_accuracy.json")
ALL_TESTS = {"main", "no_trend", "bits", "edges", "mixed", "diag", "many", "nq_edges", "marks", "failed", "state", "one_shot",
             "front_ends", "sample"}


def _record(**kw):
    _RECORDS.append(kw)
    print("COVM " + json.dumps(kw, sort_keys=True))


@pytest.fixture(scope="module", autouse=True)
def _write_accuracy_file():
    """only a run of the whole module replaces the file"""
    yield
    if {r["test"] for r in _RECORDS} >= ALL_TESTS:
        with open(ACCURACY_JSON, "w") as f:
            f.write("[\n" + ",\n".join(" " + json.dumps(r, sort_keys=True) for r in _RECORDS) + "\n]\n")


_MAIN, _REFS = {}, {}
TH, OTH = CC.FAMILIES["spline34"]


def _main(dtype="f64"):
    if dtype not in _MAIN:
        _MAIN[dtype] = CMC.Main(dtype)
    return _MAIN[dtype]


def _ref(key, oth, X, sigma2, trend):
    """the long-double factor, C_H and L_G of one patch, built once per process"""
    key = key + (trend,)
    if key not in _REFS:
        _REFS[key] = CMR.TrendRegionRef(oth, X, sigma2, trend)
    return _REFS[key]


def _main_refs(m, trend, dtype="f64", skip=()):
    return {r: _ref(("main", dtype, r), OTH, m.Xs[r], SIGMA2[dtype], trend) for r in range(4) if r not in skip}


def _model(Xs, Ys, th, dtype, root, trend, diag=None):
    """fit, attach the tree, R target columns, the trend, the multi-output solve"""
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


def _main_model(m, trend, R=1, dtype="f64"):
    return _model(m.Xs, m.Ys(R), TH, dtype, m.root, trend)


def _stages(q, th, wth, fitted=False):
    q.items_multi_fitted(True) if fitted else q.items_multi(th, True)
    q.mix_multi(wth)
    q.items_cov_multi(None if fitted else th)
    q.mix_cov(wth)
    return q


def _staged(model, Xq, radius, delta, th, wth, fitted=False):
    q = M.DeviceQuery(model, Xq)
    q.plan(radius, delta)
    return _stages(q, th, wth, fitted)


def _blend(q, owth, S_ref, units):
    """(ratio of the blend, ratio of its diagonal against Vq, Cov, Vq, the shared-region mask)"""
    dbg = q.debug()
    items = (dbg["item_offsets"], dbg["item_region"])
    ref_cov, unit = CR.mix_cov_ref(items, S_ref, dbg["item_t"], owth, units)
    Cov = q.fetch_cov()
    _, Vq = q.fetch_multi(q.model.R)
    blend = _worst_ratio(np.abs(np.asarray(Cov, dtype=CR.LD) - ref_cov).astype(np.float64), unit)
    off, reg = items
    # the diagonal is Vq where no query holds two items of one region (there it carries their cross term)
    single = np.array([len(set(reg[off[j]:off[j + 1]])) == off[j + 1] - off[j] for j in range(q.Nq)], dtype=bool)
    diag = _worst_ratio(np.abs(np.diag(Cov) - Vq)[single], np.diag(unit)[single])
    return blend, diag, Cov, Vq, CR.shared_region_mask(items)


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ------------------------------------------------------------------------------------------ the main workload
@pytest.mark.parametrize("trend,R,dtype", [(t, R, d) for d in ("f64", "f32") for t in CMC.TRENDS for R in (1, 3)])
def test_blocks_blend_and_diagonal_under_a_trend(trend, R, dtype):
    m = _main(dtype)
    model = _main_model(m, trend, R, dtype)
    assert np.all(model.info() == 0) and np.all(model.trend_info() == 0)
    q = _staged(model, m.Xq, m.RADIUS, m.DELTA, TH, m.wth)
    counts = np.diff(q.region_offsets(4))
    assert CC.TQ < counts.max() and counts.min() < CC.TQ, counts               # pairs of different strips in one region
    blocks = _device_blocks(q, 4)
    worst, kappa, S_ref, units = _check_blocks(blocks, m.Xq, _main_refs(m, trend, dtype), dtype)
    blend, diag, Cov, Vq, shared = _blend(q, m.owth, S_ref, units)
    Yq, _ = q.fetch_multi(R)
    assert Yq.shape == (len(m.Xq), R) and np.all(np.isfinite(Yq))
    _record(test="main", trend=trend, R=R, dtype=dtype, blocks=worst, blend=blend, diag_vs_vq=diag, kappa=kappa,
            region_items=[int(c) for c in counts])
    assert kappa <= CC.KAPPA_MAX and worst <= RATIO_MAX and blend <= RATIO_MAX and diag <= RATIO_MAX, (kappa, worst, blend, diag)
    assert np.array_equal(Cov, Cov.T)                                          # symmetric bit for bit
    assert not shared.all() and np.all(Cov[~shared] == 0) and not np.signbit(Cov[~shared]).any()
    # the trend's term is there: the single-output call on the same plan gives the simple-kriging blocks, which are smaller
    q.items_cov(TH)
    for r, (idx, S) in _device_blocks(q, 4).items():
        assert np.all(np.diag(blocks[r][1]) > np.diag(S)), r


def test_without_a_trend_the_blocks_are_those_of_the_single_output_call():
    m = _main()
    model = _main_model(m, None, 2)
    q = _staged(model, m.Xq, m.RADIUS, m.DELTA, TH, m.wth)
    multi, Cm = _device_blocks(q, 4), q.fetch_cov()
    q.items_cov(TH)
    q.mix_cov(m.wth)
    single, Cs = _device_blocks(q, 4), q.fetch_cov()
    assert sorted(multi) == sorted(single) and all(_bits(multi[r][1], single[r][1]) for r in single) and _bits(Cm, Cs)
    # a model that had a trend and dropped it: bit-identical again
    other = _main_model(m, "linear", 2)
    q2 = _staged(other, m.Xq, m.RADIUS, m.DELTA, TH, m.wth)
    assert not _bits(q2.fetch_cov(), Cs)
    other.set_trend(None)
    other.solve_multi()
    _stages(q2, TH, m.wth)
    again = _device_blocks(q2, 4)
    assert all(_bits(again[r][1], single[r][1]) for r in single) and _bits(q2.fetch_cov(), Cs)
    _record(test="no_trend", regions=len(single))


def test_bits_symmetry_sub_batches_and_reruns():
    m = _main()
    model = _main_model(m, "linear", 2)
    q = _staged(model, m.Xq, m.RADIUS, m.DELTA, TH, m.wth)
    blocks, Cov = _device_blocks(q, 4), q.fetch_cov()
    for r, (idx, S) in blocks.items():
        assert _bits(S, S.T), r
    assert _bits(Cov, Cov.T)
    # two runs agree
    _stages(q, TH, m.wth)
    assert _bits(q.fetch_cov(), Cov) and all(_bits(S, blocks[r][1]) for r, (idx, S) in _device_blocks(q, 4).items())
    # an entry keeps its bits when the batch is permuted and when other queries are added or left out
    idx, S = blocks[0]
    assert len(idx) > CC.TQ
    for a, b in ((0, len(idx) - 1), (3, len(idx) // 2), (len(idx) // 2 - 1, len(idx) // 2)):      # first and second strip
        ja, jb = int(idx[a]), int(idx[b])
        others = [j for j in (5, 77, 300, 411, 200) if j not in (ja, jb)][:3]
        sub = [others[0], jb, others[1], ja, others[2]]
        q2 = _staged(model, m.Xq[sub], m.RADIUS, m.DELTA, TH, m.wth)
        idx2, S2 = q2.item_covs(0)
        pa, pb = list(idx2).index(3), list(idx2).index(1)
        assert S2[pa, pb] == S[a, b] and S2[pb, pa] == S[b, a] and S2[pa, pa] == S[a, a] and S2[pb, pb] == S[b, b]
        C2 = q2.fetch_cov()
        assert C2[3, 1] == Cov[ja, jb] and C2[1, 3] == Cov[jb, ja] and C2[3, 3] == Cov[ja, ja]
    perm = np.random.default_rng(2).permutation(len(m.Xq))
    qp = _staged(model, m.Xq[perm], m.RADIUS, m.DELTA, TH, m.wth)
    assert _bits(qp.fetch_cov(), Cov[np.ix_(perm, perm)])
    _record(test="bits", region0_items=int(len(idx)))


# ------------------------------------------------------------------------------------------ kernel edges through explicit items
def _edge_run(D, trend, dtype, fit_th, oths, th=TH, set_addend=False):
    Xs = CMC.edge_patches(D, trend, dtype)
    xq, region = CMC.edge_items(Xs, dtype)
    qt = CMC.Q_OF[trend](D)
    R = 16 - qt                                                   # the widest item row
    model = _model(Xs, [CMC.targets(X, R) for X in Xs], fit_th, dtype, _tree8(D), trend)
    assert np.all(model.info() == 0)
    flagged = CMC.flagged(D, trend)
    tinfo = model.trend_info()
    assert tinfo[0] == 0                                          # n = q: a finite block
    assert [int(r) for r in np.nonzero(tinfo)[0]] == flagged and all(tinfo[r] == len(Xs[r]) + 1 for r in flagged)
    q = _explicit_query(model, xq, region)
    addend = None
    if set_addend:
        addend = np.random.default_rng(5).uniform(0.0, 0.5, len(xq))
        q.set_diag(addend)
    if th is None:
        q.items_multi_fitted(True)
    else:
        q.items_multi(th, True)
    q.items_cov_multi(th)
    blocks = _device_blocks(q, 8)
    for r, c in enumerate(CMC.EDGE_COUNTS):
        assert (len(blocks[r][0]) if r in blocks else 0) == c
        if c:
            assert np.array_equal(blocks[r][0], np.nonzero(region == r)[0])
    for r in flagged:
        assert np.all(np.isnan(blocks.pop(r)[1])), r
    refs = {r: _ref(("edge", D, dtype, oths[r].family, r), oths[r], Xs[r], SIGMA2[dtype], trend) for r in blocks}
    worst, kappa, _, _ = _check_blocks(blocks, xq, refs, dtype, addend)
    # the block's diagonal is the item variance the model reports, in the unit of the blend's diagonal check
    _, v = q.item_values_multi()
    pos = {r: np.nonzero(region == r)[0] for r in blocks}
    dv = max(_worst_ratio(np.abs(np.diag(blocks[r][1]) - v[pos[r]]),
                          (refs[r].n + 32) * U_OF[dtype] * np.diag(refs[r].cov(xq[pos[r]], None if addend is None else addend[pos[r]])["unit"]))
             for r in blocks)
    assert np.all(np.isfinite(blocks[0][1]))
    return worst, kappa, dv, blocks, q


@pytest.mark.parametrize("D,trend,dtype", [(D, t, "f64") for D, t in CMC.EDGE_TRENDS] + [(2, "linear", "f32")])
def test_kernel_edges_through_explicit_items(D, trend, dtype):
    worst, kappa, dv, blocks, q = _edge_run(D, trend, dtype, TH, [OTH] * 8)
    _record(test="edges", D=D, trend=trend, q=CMC.Q_OF[trend](D), R=16 - CMC.Q_OF[trend](D), dtype=dtype, blocks=worst,
            diag_vs_item_v=dv, kappa=kappa)
    assert kappa <= CC.KAPPA_MAX and worst <= RATIO_MAX and dv <= RATIO_MAX, (kappa, worst, dv)
    # an empty region answers m = 0; the blend of explicit items is refused
    idx, S = q.item_covs(5)
    assert len(idx) == 0 and S.shape == (0, 0)
    w = TH.desc()
    assert pmk.lib().pmk_query_mix_cov(q.h, C.byref(w)) == -2


def test_mixed_families_per_patch_and_the_models_own_kernels():
    names = CC.MIXED_NAMES
    worst, kappa, dv, own, _ = _edge_run(2, "linear", "f64", [CC.FAMILIES[n][0] for n in names], [CC.FAMILIES[n][1] for n in names], th=None)
    _record(test="mixed", blocks=worst, diag_vs_item_v=dv, kappa=kappa)
    assert kappa <= CC.KAPPA_MAX and worst <= RATIO_MAX and dv <= RATIO_MAX, (kappa, worst, dv)
    # every patch Spline34 through fit_patches: the per-patch instantiation equals the uniform one bit for bit
    _, _, _, uniform, _ = _edge_run(2, "linear", "f64", TH, [OTH] * 8)
    _, _, _, per_patch, _ = _edge_run(2, "linear", "f64", [TH] * 8, [OTH] * 8, th=None)
    assert all(_bits(uniform[r][1], per_patch[r][1]) for r in uniform)


def test_set_diag_addends_appear_on_block_diagonals_only():
    worst, kappa, dv, with_addend, _ = _edge_run(2, "linear", "f64", TH, [OTH] * 8, set_addend=True)
    _, _, _, plain, _ = _edge_run(2, "linear", "f64", TH, [OTH] * 8)
    _record(test="diag", blocks=worst, diag_vs_item_v=dv, kappa=kappa)
    assert worst <= RATIO_MAX and dv <= RATIO_MAX, (worst, dv)
    for r in plain:
        a, b = with_addend[r][1], plain[r][1]
        off = ~np.eye(len(a), dtype=bool)
        assert np.array_equal(a[off], b[off]) and np.all(np.diag(a) > np.diag(b))


def test_a_query_with_two_items_of_one_region():
    mm = CC.Many()
    P = len(mm.Xs)
    model = _model(mm.Xs, [np.ascontiguousarray(mm.y[i])[:, None] for i in mm.inds], TH, "f64", mm.root, "constant")
    assert np.all(model.info() == 0) and np.all(model.trend_info() == 0)
    q = _staged(model, mm.Xq, mm.RADIUS, mm.DELTA, TH, mm.wth)
    blocks = _device_blocks(q, P)
    refs = {r: _ref(("many", r), OTH, mm.Xs[r], SIGMA2["f64"], "constant") for r in blocks}
    worst, kappa, S_ref, units = _check_blocks(blocks, mm.Xq, refs, "f64")
    blend, diag, Cov, _, _ = _blend(q, mm.owth, S_ref, units)
    doubled = [int(r) for r, (idx, _) in blocks.items() if np.any(np.diff(idx) == 0)]
    assert doubled                                                   # every pair of items counts
    _record(test="many", blocks=worst, blend=blend, diag_vs_vq=diag, kappa=kappa, doubled_regions=doubled)
    assert kappa <= CC.KAPPA_MAX and worst <= RATIO_MAX and blend <= RATIO_MAX and diag <= RATIO_MAX, (kappa, worst, blend, diag)
    assert _bits(Cov, Cov.T)


def test_no_query_one_query_and_a_padded_leading_dimension():
    m = _main()
    model = _main_model(m, "linear", 3)
    L = pmk.lib()
    w, d = m.wth.desc(), TH.desc()
    full = _staged(model, m.Xq, m.RADIUS, m.DELTA, TH, m.wth).fetch_cov()
    # one query: its variance, bit for bit the entry of the full batch
    q1 = _staged(model, m.Xq[7:8], m.RADIUS, m.DELTA, TH, m.wth)
    C1 = q1.fetch_cov()
    assert C1.shape == (1, 1) and C1[0, 0] == full[7, 7]
    # no query at all: every stage answers 0 and the result is a (0, 0) array
    q0 = M.DeviceQuery(model, np.zeros((0, 2)))
    assert q0.plan(m.RADIUS, m.DELTA) == 0
    q0.items_multi(TH, True)
    q0.mix_multi(m.wth)
    buf = np.full((1, 1), -7.0)
    assert L.pmk_query_items_cov_multi(q0.h, C.byref(d)) == 0 and L.pmk_query_mix_cov(q0.h, C.byref(w)) == 0
    assert L.pmk_query_fetch_cov(q0.h, M._d(buf), 1) == 0 and buf[0, 0] == -7.0
    assert q0.fetch_cov().shape == (0, 0)
    # a padded ldc of the staged fetch
    Nq = 33
    q = _staged(model, m.Xq[:Nq], m.RADIUS, m.DELTA, TH, m.wth)
    pad = np.full((Nq, Nq + 5), -7.0)
    assert L.pmk_query_fetch_cov(q.h, M._d(pad), Nq + 5) == 0
    assert _bits(pad[:, :Nq], q.fetch_cov()) and np.all(pad[:, Nq:] == -7.0)
    _record(test="nq_edges", sizes=[0, 1, Nq])


# ------------------------------------------------------------------------------------------ marks
def _marked_run(m, model, sound, bad_patch):
    qb = _staged(model, m.Xq, m.RADIUS, m.DELTA, TH, m.wth)
    dbg = qb.debug()
    reg, off = dbg["item_region"], dbg["item_offsets"]
    bad_q = np.array([(reg[off[j]:off[j + 1]] == bad_patch).any() for j in range(len(m.Xq))])
    assert bad_q.any() and not bad_q.all()
    for r in range(4):
        Sb = qb.item_covs(r)[1]
        assert np.all(np.isnan(Sb)) if r == bad_patch else np.all(np.isfinite(Sb)), r
    Cb = qb.fetch_cov()
    bad = bad_q[:, None] | bad_q[None, :]
    assert np.all(np.isnan(Cb[bad])) and np.all(np.isfinite(Cb[~bad]))
    # the other entries keep the bits of a batch without that patch's queries, and of a sound model
    keep = np.nonzero(~bad_q)[0]
    qk = _staged(model, m.Xq[keep], m.RADIUS, m.DELTA, TH, m.wth)
    assert _bits(qk.fetch_cov(), Cb[np.ix_(keep, keep)])
    if sound is not None:
        assert _bits(_staged(sound, m.Xq[keep], m.RADIUS, m.DELTA, TH, m.wth).fetch_cov(), Cb[np.ix_(keep, keep)])
    return int(bad_q.sum())


def test_a_patch_with_fewer_points_than_basis_functions():
    m = _main()
    Xs = list(m.Xs)
    Xs[2] = np.ascontiguousarray(Xs[2][:2])                      # n = 2 < q = 3
    model = _model(Xs, [CMC.targets(x, 2) for x in Xs], TH, "f64", m.root, "linear")
    assert np.all(model.info() == 0) and list(model.trend_info()) == [0, 0, 3, 0]
    n_bad = _marked_run(m, model, None, 2)
    # n = q: a finite block, tinfo 0
    Xs[2] = np.ascontiguousarray(m.Xs[2][:3])
    exact = _model(Xs, [CMC.targets(x, 2) for x in Xs], TH, "f64", m.root, "linear")
    assert np.all(exact.trend_info() == 0)
    q = _staged(exact, m.Xq, m.RADIUS, m.DELTA, TH, m.wth)
    assert np.all(np.isfinite(q.item_covs(2)[1])) and np.all(np.isfinite(q.fetch_cov()))
    _record(test="marks", queries_of_the_flagged_patch=n_bad)


def test_a_patch_whose_factorisation_failed():
    m = _main()
    sound = _main_model(m, "linear", 2)
    diag = [np.zeros(len(x)) for x in m.Xs]
    diag[2][3] = -3.0                                            # the factorisation of this patch fails (tests/test_gpu_breakdown.py)
    broken = _model(m.Xs, m.Ys(2), TH, "f64", m.root, "linear", diag=diag)
    assert broken.info()[2] != 0 and np.all(np.delete(broken.info(), 2) == 0)
    n_bad = _marked_run(m, broken, sound, 2)
    _record(test="failed", queries_of_the_failed_patch=n_bad)


# ------------------------------------------------------------------------------------------ state
def test_refusals_and_state():
    L = pmk.lib()
    m = _main()
    d, w = TH.desc(), m.wth.desc()
    model = _main_model(m, "linear", 2)
    Xq = np.ascontiguousarray(m.Xq[:40])
    buf = np.empty((40, 40))

    def refused(q, code, text, th=d):
        assert L.pmk_query_items_cov_multi(q.h, None if th is None else C.byref(th)) == code
        assert text.encode() in L.pmk_last_error(), L.pmk_last_error()

    q = M.DeviceQuery(model, Xq)
    refused(q, -1, "not planned")                                              # no plan
    q.plan(m.RADIUS, m.DELTA)
    refused(q, -2, "pmk_query_items_multi")                                    # no items yet
    q.items_fitted()
    refused(q, -2, "pmk_query_items_multi")                                    # the single-output items
    q.items_multi(TH, True)
    ms = pmk.ModulatedSqExpKernelType(2.0, 1.3).desc()
    refused(q, -2, "PMK_MODSQEXP", ms)
    unknown = TH.desc()
    unknown.family = 99
    refused(q, -2, "unknown kernel family", unknown)
    q.mix_multi(m.wth)
    q.items_cov_multi(TH)
    assert L.pmk_query_fetch_cov(q.h, M._d(buf), 40) == -2                     # before mix_cov
    q.mix_cov(m.wth)
    first = q.fetch_cov()
    # pmk_query_items_cov after it gives the single-output blocks again, and the other way round
    q.items_cov(TH)
    q.mix_cov(m.wth)
    plain = q.fetch_cov()
    qs = M.DeviceQuery(model, Xq)
    qs.plan(m.RADIUS, m.DELTA)
    qs.items(TH); qs.mix(m.wth); qs.items_cov(TH); qs.mix_cov(m.wth)
    assert _bits(plain, qs.fetch_cov()) and not _bits(plain, first)
    q.items_cov_multi(TH)
    q.mix_cov(m.wth)
    assert _bits(q.fetch_cov(), first)
    # new items discard the blocks with a trend's term; a re-plan discards everything
    q.items_multi(TH, True)
    assert L.pmk_query_mix_cov(q.h, C.byref(w)) == -2 and L.pmk_query_get_items_cov(q.h, 0, None, None, None, 0) == -2
    _stages(q, TH, m.wth)
    q.plan(0.3, m.DELTA)
    assert L.pmk_query_fetch_cov(q.h, M._d(buf), 40) == -2 and L.pmk_query_mix_cov(q.h, C.byref(w)) == -2
    refused(q, -2, "pmk_query_items_multi")
    q.plan(m.RADIUS, m.DELTA)
    _stages(q, TH, m.wth)
    assert _bits(q.fetch_cov(), first)
    # set_trend makes the weights stale; after the solve the items belong to another trend
    model.set_trend("constant")
    refused(q, -3, "stale")
    model.solve_multi()
    refused(q, -2, "run the items again")
    _stages(q, TH, m.wth)
    constant = q.fetch_cov()
    assert not _bits(constant, first) and not _bits(constant, plain)
    model.set_trend("linear")
    model.solve_multi()
    refused(q, -2, "run the items again")
    _stages(q, TH, m.wth)
    assert _bits(q.fetch_cov(), first)
    # the items of the blended leave-one-out are lookups, not functions of x
    tree = pmk.MixtureGPType.from_tree(m.root, m.X, eps=m.EPS)
    pmk.fitmixtureGP_trend_(tree, np.asfortranarray(CMC.targets(m.X, 2)), TH, SIGMA2["f64"], "constant")
    tree._model.loo()
    qt = M.DeviceQuery(tree._model, m.X)
    qt.plan(m.RADIUS, m.DELTA)
    qt.items_loo_multi(False, True)
    refused(qt, -2, "pmk_query_items_loo_multi")
    qt.items_multi_fitted(True)
    assert L.pmk_query_items_cov_multi(qt.h, None) == 0
    # a model of factors holds no kernels until it is given them
    loaded = M.DeviceModel.from_factors(m.Xs, model.weights(), [model.get(r, M.GET_L) for r in range(4)])
    loaded.set_bsp(m.root, 0)
    loaded.set_targets_multi(m.Ys(2))
    loaded.set_trend("linear")
    loaded.solve_multi()
    ql = M.DeviceQuery(loaded, Xq)
    ql.plan(m.RADIUS, m.DELTA)
    ql.items_multi(TH, True)
    refused(ql, -3, "holds no kernels", None)
    assert L.pmk_predict_mixture_cov_multi_fitted(loaded.h, C.byref(w), 40, M._d(Xq), m.RADIUS, m.DELTA, None, 40, None, M._d(buf), 40) == -3
    # a shard of the leaves
    shard = M.DeviceModel(m.Xs[2:], [np.ascontiguousarray(y[:, 0]) for y in m.Ys(1)[2:]])
    shard.fit(TH, SIGMA2["f64"])
    shard.set_bsp(m.root, 2)
    qh = M.DeviceQuery(shard, Xq)
    qh.plan(m.RADIUS, m.DELTA)
    refused(qh, -3, "every leaf")
    assert L.pmk_predict_mixture_cov_multi_fitted(shard.h, C.byref(w), 40, M._d(Xq), m.RADIUS, m.DELTA, None, 40, None, M._d(buf), 40) == -3
    # no resident factor
    unfit = M.DeviceModel(m.Xs, [np.ascontiguousarray(y[:, 0]) for y in m.Ys(1)])
    unfit.set_bsp(m.root, 0)
    qu = M.DeviceQuery(unfit, Xq)
    qu.plan(m.RADIUS, m.DELTA)
    refused(qu, -1, "resident factor")
    # more queries than the limit, before any launch
    big = np.random.default_rng(3).uniform(-3.9, 3.9, (16385, 2))
    qb = M.DeviceQuery(model, big)
    qb.plan(0.0, m.DELTA)
    qb.items_multi(TH, False)
    refused(qb, -5, "PMK_COV_MAX_QUERIES")
    assert L.pmk_predict_mixture_cov_multi_fitted(model.h, C.byref(w), 16385, M._d(big), 0.0, m.DELTA, None, 16385, None, M._d(buf), 16385) == -5
    assert L.pmk_predict_mixture_cov_multi_fitted(model.h, C.byref(w), 40, M._d(Xq), m.RADIUS, m.DELTA, None, 40, None, M._d(buf), 39) == -4
    _record(test="state", refusals=14)


# ------------------------------------------------------------------------------------------ one-shot and front ends
def test_the_one_shot_equals_the_staged_calls():
    m = _main()
    R = 3
    model = _main_model(m, "linear", R)
    Nq = 120
    Xc = np.ascontiguousarray(m.Xq[:Nq])
    q = _staged(model, Xc, m.RADIUS, m.DELTA, TH, m.wth, fitted=True)
    Yq, Vq = q.fetch_multi(R)
    Cov = q.fetch_cov()
    L, w = pmk.lib(), m.wth.desc()
    Y1, V1, C1 = np.full((R, Nq + 2), -7.0), np.empty(Nq), np.full((Nq, Nq + 3), -7.0)
    _lib.check(L.pmk_predict_mixture_cov_multi_fitted(model.h, C.byref(w), Nq, M._d(Xc), m.RADIUS, m.DELTA, M._d(Y1), Nq + 2, M._d(V1),
                                                      M._d(C1), Nq + 3), "pmk_predict_mixture_cov_multi_fitted")
    assert _bits(Y1[:, :Nq].T, Yq) and _bits(V1, Vq) and _bits(C1[:, :Nq], Cov)
    assert np.all(Y1[:, Nq:] == -7.0) and np.all(C1[:, Nq:] == -7.0)
    # with Cov NULL no covariance stage runs; with Vq NULL the items run mean-only; the means are the same
    Y2, V2 = np.empty((R, Nq)), np.empty(Nq)
    _lib.check(L.pmk_predict_mixture_cov_multi_fitted(model.h, C.byref(w), Nq, M._d(Xc), m.RADIUS, m.DELTA, M._d(Y2), Nq, M._d(V2),
                                                      None, 0), "pmk_predict_mixture_cov_multi_fitted")
    assert _bits(Y2.T, Yq) and _bits(V2, Vq)
    C3 = np.empty((Nq, Nq))
    _lib.check(L.pmk_predict_mixture_cov_multi_fitted(model.h, C.byref(w), Nq, M._d(Xc), m.RADIUS, m.DELTA, None, 0, None,
                                                      M._d(C3), Nq), "pmk_predict_mixture_cov_multi_fitted")
    assert _bits(C3, Cov)
    _record(test="one_shot", Nq=Nq, R=R)


def _corner_queries(m, n=8, seed=9):
    """queries that share regions: around the corner where the four leaves meet, at distinct places"""
    centre = np.mean([x.mean(0) for x in m.Xs], 0)
    return centre + np.random.default_rng(seed).uniform(-0.5, 0.5, (n, 2))


def test_the_front_end_on_a_list_built_and_a_tree_built_eta():
    m = _main()
    R = 2
    Y = CMC.targets(m.X, R)
    Xq = _corner_queries(m)
    eta = pmk.MixtureGPType(m.Xs, pmk.fetchhyperplanes(m.root))
    pmk.fitmixtureGP_trend_(eta, [np.ascontiguousarray(Y[i]) for i in m.inds], TH, SIGMA2["f64"], "linear")
    args = (Xq, eta, m.root, m.LEVELS, m.RADIUS, m.DELTA, m.wth)
    Yq, Vq, Cov = pmk.querymixtureGP_cov_multi(*args)
    Y0, V0 = pmk.querymixtureGP_multi_patches(*args)
    assert Yq.shape == (8, R) and _bits(Yq, Y0) and _bits(Vq, V0) and _bits(Cov, Cov.T)
    # the diagonal is the variance the model predicts
    q = _staged(eta._model, Xq, m.RADIUS, m.DELTA, TH, m.wth, fitted=True)
    assert _bits(q.fetch_cov(), Cov)
    worst, _, S_ref, units = _check_blocks(_device_blocks(q, 4), Xq, _main_refs(m, "linear"), "f64")
    blend, diag, _, _, _ = _blend(q, m.owth, S_ref, units)
    dbg = q.debug()
    _, unit = CR.mix_cov_ref((dbg["item_offsets"], dbg["item_region"]), S_ref, dbg["item_t"], m.owth, units)
    # the same points through a tree-built eta
    tree = pmk.MixtureGPType.from_tree(m.root, m.X, eps=m.EPS)
    pmk.fitmixtureGP_trend_(tree, np.asfortranarray(Y), TH, SIGMA2["f64"], "linear")
    Yt, Vt, Ct = pmk.querymixtureGP_cov_multi(Xq, tree, m.root, m.LEVELS, m.RADIUS, m.DELTA, m.wth)
    # both are within RATIO_MAX units of the reference
    tb = _worst_ratio(np.abs(Ct - Cov), 2 * RATIO_MAX * unit)
    assert Yt.shape == Yq.shape and np.allclose(Yt, Yq, rtol=1e-9, atol=1e-9) and np.allclose(Vt, Vq, rtol=1e-9, atol=1e-12)
    # a multi-output fit without a trend serves too: the covariance of querymixtureGP_cov
    plain = pmk.MixtureGPType(m.Xs, pmk.fetchhyperplanes(m.root))
    pmk.fitmixtureGP_multi_(plain, [np.ascontiguousarray(Y[i]) for i in m.inds], TH, SIGMA2["f64"])
    _, _, Cp = pmk.querymixtureGP_cov_multi(Xq, plain, m.root, m.LEVELS, m.RADIUS, m.DELTA, m.wth)
    _, _, Cs = pmk.querymixtureGP_cov(Xq, plain, m.root, m.LEVELS, m.RADIUS, m.DELTA, m.wth)
    assert _bits(Cp, Cs) and np.all(np.diag(Cov) > np.diag(Cp))
    _record(test="front_ends", blocks=worst, blend=blend, diag_vs_vq=diag, tree_vs_list=tb)
    assert worst <= RATIO_MAX and blend <= RATIO_MAX and diag <= RATIO_MAX and tb <= 1.0, (worst, blend, diag, tb)


# ------------------------------------------------------------------------------------------ draws
def test_posterior_draws_of_the_columns():
    import torch
    m = _main()
    R = 3
    Y = CMC.targets(m.X, R)
    eta = pmk.MixtureGPType(m.Xs, pmk.fetchhyperplanes(m.root))
    pmk.fitmixtureGP_trend_(eta, [np.ascontiguousarray(Y[i]) for i in m.inds], TH, SIGMA2["f64"], "constant")
    Xq = _corner_queries(m)
    args = (Xq, eta, m.root, m.LEVELS, m.RADIUS, m.DELTA, m.wth)
    Yq, Vq, Cov = pmk.querymixtureGP_cov_multi(*args)
    assert (np.abs(Cov[~np.eye(8, dtype=bool)]) > 0).sum() >= 20               # the queries share regions
    n = 4096
    dev = torch.device("cuda", 0)
    draws, jitter = pmk.samplemixtureGP_multi(*args, n, generator=torch.Generator(device=dev).manual_seed(17))
    again, _ = pmk.samplemixtureGP_multi(*args, n, generator=torch.Generator(device=dev).manual_seed(17))
    assert jitter == 0.0 and tuple(draws.shape) == (n, 8, R) and torch.equal(draws, again)
    # with z passed in, column c is Yq[:, c] + z[:, :, c] L^T with L L^T = Cov, computed with torch from the fetched Cov
    z = torch.randn((n, 8, R), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    dz, jz = pmk.samplemixtureGP_multi(*args, n, z=z)
    assert jz == 0.0
    Ct, Yt = torch.as_tensor(Cov, device=dev), torch.as_tensor(np.ascontiguousarray(Yq), device=dev)
    Lc, info = torch.linalg.cholesky_ex(Ct)
    assert int(info) == 0
    # two evaluations of a sum of eight products and one addition: 2 (8 + 2) u (|Yq| + |z| |L|^T), entry by entry
    tol = 20 * U_OF["f64"] * (Yt.abs().max() + (z.abs().amax(2) @ Lc.abs().T).max())
    for c in range(R):
        assert float((dz[:, :, c] - (Yt[:, c][None, :] + z[:, :, c] @ Lc.T)).abs().max()) <= float(tol), c
    with pytest.raises(ValueError, match="z must have shape"):
        pmk.samplemixtureGP_multi(*args, n, z=z[:, :, :2])
    # L L^T = Cov to 10 units of the blended entries plus what a Cholesky in double of an 8 x 8 matrix may add: 9 u
    # sqrt(C_ii C_jj) (Higham, Accuracy and Stability, Thm 10.3), also where the unit is zero: the bound of tests/test_gpu_cov.py
    q = _staged(eta._model, Xq, m.RADIUS, m.DELTA, TH, m.wth, fitted=True)
    assert _bits(q.fetch_cov(), Cov)
    _, _, S_ref, units = _check_blocks(_device_blocks(q, 4), Xq, _main_refs(m, "constant"), "f64")
    dbg = q.debug()
    _, unit = CR.mix_cov_ref((dbg["item_offsets"], dbg["item_region"]), S_ref, dbg["item_t"], m.owth, units)
    bound = RATIO_MAX * unit + 2 * 9 * U_OF["f64"] * np.sqrt(np.outer(np.diag(Cov), np.diag(Cov)))
    LLt = (Lc @ Lc.T).cpu().numpy()
    ratio = RATIO_MAX * float((np.abs(LLt - Cov) / bound).max())
    # the sample covariance of every column within 6 standard errors, entry by entry; two columns are uncorrelated
    x = draws.cpu().numpy() - Yq[None, :, :]
    se = np.sqrt((np.outer(np.diag(Cov), np.diag(Cov)) + Cov ** 2) / n)
    z_worst = max(float((np.abs(x[:, :, c].T @ x[:, :, c] / n - Cov) / se).max()) for c in range(R))
    se_cross = np.sqrt(np.outer(np.diag(Cov), np.diag(Cov)) / n)                 # Var(x_j y_k) for independent x, y
    z_cross = max(float((np.abs(x[:, :, a].T @ x[:, :, b] / n) / se_cross).max()) for a in range(R) for b in range(a + 1, R))
    _record(test="sample", llt_ratio=ratio, worst_standard_errors=z_worst, worst_cross_standard_errors=z_cross, jitter=jitter)
    assert ratio <= RATIO_MAX and z_worst <= 6.0 and z_cross <= 6.0, (ratio, z_worst, z_cross)
    # a covariance that holds NaN raises before any factorisation
    Xs = list(m.Xs)
    Xs[2] = np.ascontiguousarray(Xs[2][:2])
    bad = pmk.MixtureGPType(Xs, pmk.fetchhyperplanes(m.root))
    with pytest.raises(pmk.TrendRankException):
        pmk.fitmixtureGP_trend_(bad, [CMC.targets(x, R) for x in Xs], TH, SIGMA2["f64"], "linear")
    called = []                                                 # the fit stopped at the flag: the model is resident all the same
    monkey = torch.linalg.cholesky_ex
    torch.linalg.cholesky_ex = lambda *a, **k: called.append(1) or monkey(*a, **k)
    try:
        with pytest.raises(np.linalg.LinAlgError, match="NaN"):
            pmk.samplemixtureGP_multi(Xq, bad, m.root, m.LEVELS, m.RADIUS, m.DELTA, m.wth, 4)
    finally:
        torch.linalg.cholesky_ex = monkey
    assert not called
