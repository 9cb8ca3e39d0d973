"""Posterior draws from the region blocks on the GPU (pmk_query_items_cov_blocks / _factor_cov / _factor_info /
_get_items_cov_factor / _draw; the kernels of pmk_draw.hip) and method="blocks" of the sampling front ends.

Reference and units: tests/_draw_refs.py, whose conditions tests/test_draw_refs.py checks on the same inputs.
  * a factor: |L L^T - (S + jitter I)| against the device's own block S of item_covs, unit (m + 8) 2^-53 sqrt(S_aa S_bb),
    bound 10 units (numpy.linalg.cholesky stays below 0.25 units on these blocks: test_draw_refs.py);
  * the blend: draw with z = I returns A^T, and A A^T (long double on the host) against fetch_cov of the same plan, bound
    sum over the blended entries of wn wn' (10 block units + 8 x 2^-53 |S_ab|): the factors' bound and the roundings of the
    two weights, their product and the chain of mix_cov and of draw_mix.

Every measured ratio is printed ("DRAW {json}", run with -s) and a run of the whole module writes them to
profiles/draw_accuracy.json.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import mixture as M
import _cov_cases as CC
import _cov_refs as CR
import _draw_refs as DR
from test_gpu_cov import _fitted, _main, _main_model
from test_gpu_cov_multi import _main as _multi_main, _main_model as _multi_model
from test_gpu_grad import _explicit_query, _worst_ratio

pytestmark = pytest.mark.gpu

LD, U53, RATIO_MAX, SIGMA2 = DR.LD, DR.U53, DR.RATIO_MAX, CC.SIGMA2
_RECORDS = []
ACCURACY_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "draw_accuracy.json")
ALL_TESTS = {"factor", "dense", "dense_trend", "bits", "tiles", "jitter", "failed", "distribution", "beyond", "state"}
LAPACK_WORST = 0.22                                           # numpy.linalg.cholesky on the reference blocks (test_draw_refs.py)


def _record(**kw):
    _RECORDS.append(kw)
    print("DRAW " + json.dumps(kw, sort_keys=True))


@pytest.fixture(scope="module", autouse=True)
def _write_accuracy_file():
    """only a run of the whole module replaces the file"""
    yield
    if {r["test"] for r in _RECORDS} >= ALL_TESTS:
        with open(ACCURACY_JSON, "w") as f:
            f.write("[\n" + ",\n".join(" " + json.dumps(r, sort_keys=True) for r in _RECORDS) + "\n]\n")


def _planned(model, Xq, radius, delta, th, wth):
    q = M.DeviceQuery(model, Xq)
    q.plan(radius, delta)
    q.items(th)
    q.mix(wth)
    return q


def _blocks(q, P):
    """{r: (idx, S_r, L_r)} of the regions with items"""
    out = {}
    for r in range(P):
        idx, S = q.item_covs(r)
        if len(idx):
            out[r] = (idx.astype(np.int64), S, q.item_cov_factor(r))
    return out


def _factor_worst(blocks, jitter=None):
    """worst |L L^T - (S + jitter I)| / unit; L lower triangular with a positive diagonal"""
    worst = 0.0
    for r, (idx, S, L) in blocks.items():
        assert L.shape == S.shape and np.all(np.triu(L, 1) == 0) and np.all(np.diag(L) > 0), r
        Sj = S if jitter is None else S + jitter[r] * np.eye(len(S))
        worst = max(worst, DR.factor_ratio(L, Sj))
    return worst


def _ladder(q, P):
    """the jitter ladder of the front ends through the staged calls -> (finfo at rel = 0, rel, jitter)"""
    rel = np.zeros(P)
    q.factor_cov(rel)
    first, jit = q.factor_info()
    finfo = first
    while np.any(finfo > 0):
        bad = finfo > 0
        rel[bad] = np.where(rel[bad] == 0.0, 2.0 ** -52, 10.0 * rel[bad])
        assert np.all(rel <= 2.0 ** -26)
        q.factor_cov(rel)
        finfo, jit = q.factor_info()
    return first, rel, jit


def _weights(q, owth):
    """W [Nq, total] (long double) of the device's plan and the first sorted position of every region with items"""
    dbg = q.debug()
    items = (dbg["item_offsets"], dbg["item_region"])
    return DR.weight_matrix(items, dbg["item_t"], owth), DR.sorted_layout(items)[1], items


def _identity_draw(q, wth):
    """A [Nq, total]: draw with z = I returns A^T, once from host arrays and once from device tensors, bit for bit"""
    import torch
    total = int(q.total)
    E = q.draw(wth, np.eye(total))
    assert E.shape == (total, q.Nq)
    dev = torch.device("cuda", q.model.ctx.device)
    zt = torch.eye(total, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    Et = q.draw(wth, zt)
    q.model.ctx.synchronize()
    assert np.array_equal(Et.cpu().numpy(), E)
    return np.ascontiguousarray(E.T)


def _dense_check(q, P, wth, owth, Cov):
    """-> (factor ratio, blend ratio) of a factored plan whose dense covariance is Cov"""
    blocks = _blocks(q, P)
    W, roff, items = _weights(q, owth)
    assert [roff[r] for r in sorted(roff)] == [int(q.region_offsets(P)[r]) for r in sorted(roff)]
    A = _identity_draw(q, wth)
    # a unit normal at one item moves only the queries that hold an item of its region, by a multiple of the item's column
    Wd = np.asarray(W, dtype=np.float64)
    for r, (idx, S, L) in blocks.items():
        cols = slice(roff[r], roff[r] + len(idx))
        holds = (Wd[:, cols] != 0).any(1)
        assert np.all(A[~holds, cols] == 0) and np.all((A[:, cols] != 0).any(1) == holds), r
    AAt = np.asarray(A, dtype=LD) @ np.asarray(A, dtype=LD).T
    bound = np.zeros((q.Nq, q.Nq))
    for r, (idx, S, L) in blocks.items():
        Wr = Wd[:, roff[r]:roff[r] + len(idx)]
        bound += Wr @ (RATIO_MAX * DR.block_unit(S) + 8 * U53 * np.abs(S)) @ Wr.T
    shared = CR.shared_region_mask(items)
    assert not shared.all() and np.all(AAt[~shared] == 0) and np.all(Cov[~shared] == 0) and np.all(bound[~shared] == 0)
    blend = RATIO_MAX * _worst_ratio(np.abs(AAt - np.asarray(Cov, dtype=LD)).astype(np.float64), bound)
    return _factor_worst(blocks), blend


# ------------------------------------------------------------------------------------------ factors and the dense covariance
@pytest.mark.parametrize("family,dtype", [("spline34", "f64"), ("gaussian", "f64"), ("spline34", "f32")])
def test_factors_and_equivalence_with_the_dense_covariance(family, dtype):
    m = _main(dtype)
    th, _ = CC.FAMILIES[family]
    model = _main_model(m, th, dtype)
    q = _planned(model, DR.main_queries(m), m.RADIUS, m.DELTA, th, m.wth)
    q.items_cov(th)
    q.mix_cov(m.wth)
    Cov = q.fetch_cov()
    q.factor_cov()
    finfo, jit = q.factor_info()
    assert np.all(finfo == 0) and np.all(jit == 0.0)
    factor, blend = _dense_check(q, 4, m.wth, m.owth, Cov)
    _record(test="factor", family=family, dtype=dtype, factor=factor, lapack=LAPACK_WORST)
    _record(test="dense", family=family, dtype=dtype, blend=blend)
    assert factor <= RATIO_MAX and blend <= RATIO_MAX, (factor, blend)
    # the blocks of items_cov_blocks are those of items_cov, and so are the factors
    before = _blocks(q, 4)
    q.items_cov_blocks(th)
    q.factor_cov()
    for r, (idx, S, L) in _blocks(q, 4).items():
        assert np.array_equal(S, before[r][1]) and np.array_equal(L, before[r][2]), r


def test_equivalence_under_a_linear_trend_with_two_columns():
    m = _multi_main()
    th = CC.FAMILIES["spline34"][0]
    model = _multi_model(m, "linear", 2)
    q = M.DeviceQuery(model, np.ascontiguousarray(m.Xq[:DR.NQ_MAIN]))
    q.plan(m.RADIUS, m.DELTA)
    q.items_multi(th, True)
    q.mix_multi(m.wth)
    q.items_cov_multi(th)
    q.mix_cov(m.wth)
    Cov = q.fetch_cov()
    dense = {r: q.item_covs(r)[1] for r in range(4)}
    q.items_cov_blocks(th, multi=True)
    for r in range(4):
        assert np.array_equal(q.item_covs(r)[1], dense[r]), r
    q.factor_cov()
    assert np.all(q.factor_info()[0] == 0)
    factor, blend = _dense_check(q, 4, m.wth, m.owth, Cov)
    _record(test="dense_trend", factor=factor, blend=blend)
    assert factor <= RATIO_MAX and blend <= RATIO_MAX, (factor, blend)


# ------------------------------------------------------------------------------------------ tiles and bits
def _tree16():
    return pmk.setuppartition(np.random.default_rng(6).uniform(-4, 4, (128, 2)), 5)[0]


def _tile_model():
    th = CC.FAMILIES["spline34"][0]
    Xs = DR.tile_patches()
    return _fitted(Xs, [np.sin(X[:, 0]) for X in Xs], th, "f64", _tree16()), th


def test_tile_edges_through_explicit_items_and_bits():
    model, th = _tile_model()
    assert np.all(model.info() == 0)
    xq, region = DR.tile_items()
    q = _explicit_query(model, xq, region)
    q.items_cov(th)
    q.factor_cov()
    finfo, jit = q.factor_info()
    assert np.all(finfo == 0) and np.all(jit == 0.0)
    blocks = _blocks(q, 16)
    assert [len(blocks[r][0]) if r in blocks else 0 for r in range(16)] == DR.TILE_COUNTS
    worst = _factor_worst(blocks)
    _record(test="tiles", factor=worst, counts=DR.TILE_COUNTS, lapack=0.129)
    assert worst <= RATIO_MAX, worst
    assert q.item_cov_factor(9).shape == (0, 0)
    # the draw belongs to a blend: explicit items have none
    w = th.desc()
    z = np.zeros(len(xq))
    assert pmk.lib().pmk_query_draw(q.h, C.byref(w), 1, z.ctypes.data, len(xq), z.ctypes.data, len(xq)) == -2
    # a second run gives the same factors
    q.items_cov(th)
    q.factor_cov()
    for r, (idx, S, L) in _blocks(q, 16).items():
        assert np.array_equal(L, blocks[r][2]), r
    # the items of the other regions replaced (fewer, elsewhere, another order): regions 7 and 8 keep their factors' bits
    keep = (region == 7) | (region == 8)
    rng = np.random.default_rng(77)
    other_r = rng.integers(0, 7, 90).astype(np.int32)
    xq2 = np.vstack([rng.uniform(-2.5, 2.5, (90, 2)), xq[keep]])
    region2 = np.concatenate([other_r, region[keep]])
    q2 = _explicit_query(model, xq2, region2)
    q2.items_cov(th)
    q2.factor_cov()
    for r in (7, 8):
        assert np.array_equal(q2.item_covs(r)[1], blocks[r][1]) and np.array_equal(q2.item_cov_factor(r), blocks[r][2]), r
    # a retry with another rel for region 8: it is factored again, every other region keeps its bits
    rel = np.zeros(16)
    rel[8] = 1e-6
    q.factor_cov(rel)
    finfo, jit = q.factor_info()
    S8 = blocks[8][1]
    assert np.all(finfo == 0) and abs(jit[8] / (1e-6 * np.trace(S8) / len(S8)) - 1) < 1e-13      # the trace in another order
    assert np.all(np.delete(jit, 8) == 0.0)
    again = _blocks(q, 16)
    for r in blocks:
        same = np.array_equal(again[r][2], blocks[r][2])
        assert same == (r != 8), r
    retry = _factor_worst({8: again[8]}, jit)
    _record(test="bits", retry_factor=retry)
    assert retry <= RATIO_MAX, retry


# ------------------------------------------------------------------------------------------ jitter, failed patch
def _main_eta(m, model=None):
    th, _ = CC.FAMILIES["spline34"]
    eta = pmk.MixtureGPType(m.Xs, pmk.fetchhyperplanes(m.root))
    if model is None:
        pmk.fitmixtureGP_(eta, [np.ascontiguousarray(m.y[i]) for i in m.inds], th, SIGMA2["f64"])
    else:
        eta._model = model
    eta._model.set_bsp(m.root, 0)
    return eta


def test_a_duplicated_query_needs_jitter_in_its_region_only():
    import torch
    m = _main("f64")
    th, _ = CC.FAMILIES["spline34"]
    eta = _main_eta(m)
    Xq = DR.duplicated_queries(m)
    q = _planned(eta._model, Xq, 0.0, m.DELTA, th, m.wth)
    home = int(q.debug()["item_region"][7])
    q.items_cov(th)
    first, rel, jit = _ladder(q, 4)
    m_home = len(q.item_covs(home)[0])
    assert first[home] == m_home and np.all(np.delete(first, home) == 0), first      # the second copy is the last row
    assert rel[home] > 0 and np.all(np.delete(rel, home) == 0) and jit[home] > 0
    worst = _factor_worst(_blocks(q, 4), jit)
    n = 256
    draws, jitter = pmk.samplemixtureGP(Xq, eta, m.root, m.LEVELS, 0.0, m.DELTA, m.wth, n, method="blocks",
                                        generator=torch.Generator(device=torch.device("cuda", 0)).manual_seed(5))
    assert jitter == jit[home] and tuple(draws.shape) == (n, len(Xq))
    x = draws.cpu().numpy()
    gap = float(np.abs(x[:, 7] - x[:, -1]).max())
    # the two copies differ by sqrt(2 jitter) times a standard normal (up to the rounding the jitter covers): 6 deviations
    _record(test="jitter", factor=worst, jitter=jitter, rel=float(rel[home]), gap=gap, gap_scale=float(np.sqrt(2 * jitter)))
    assert worst <= RATIO_MAX and 0 < gap <= 6.0 * np.sqrt(2 * jitter) + 64 * U53 * np.abs(x[:, 7]).max(), (worst, gap, jitter)
    assert float(np.std(x[:, 7])) > 1e3 * gap


def test_a_failed_patch_is_marked_and_nan_only_where_it_is_blended():
    m = _main("f64")
    th, _ = CC.FAMILIES["spline34"]
    sound = _main_model(m, th, "f64")
    broken = M.DeviceModel(m.Xs, [np.ascontiguousarray(m.y[i]) for i in m.inds], dtype="f64")
    diag = [np.zeros(len(x)) for x in m.Xs]
    diag[2][3] = -3.0                                            # the factorisation of this patch fails (tests/test_gpu_cov.py)
    broken.set_diag(diag)
    broken.fit(th, SIGMA2["f64"])
    broken.set_bsp(m.root, 0)
    assert broken.info()[2] != 0
    Xq = DR.main_queries(m)
    out = {}
    for name, model in (("sound", sound), ("broken", broken)):
        q = _planned(model, Xq, m.RADIUS, m.DELTA, th, m.wth)
        q.items_cov(th)
        q.factor_cov()
        finfo, _ = q.factor_info()
        z = np.random.default_rng(8).standard_normal((5, int(q.total)))
        out[name] = (finfo, q.draw(m.wth, z), q.debug())
    assert np.all(out["sound"][0] == 0) and list(out["broken"][0]) == [0, 0, -1, 0]
    dbg = out["broken"][2]
    reg, off = dbg["item_region"], dbg["item_offsets"]
    bad_q = np.array([(reg[off[j]:off[j + 1]] == 2).any() for j in range(len(Xq))])
    assert bad_q.any() and not bad_q.all()
    Es, Eb = out["sound"][1], out["broken"][1]
    assert np.all(np.isnan(Eb[:, bad_q])) and np.array_equal(Eb[:, ~bad_q], Es[:, ~bad_q]) and np.all(np.isfinite(Es))
    with pytest.raises(np.linalg.LinAlgError, match="region 2"):
        pmk.samplemixtureGP(Xq, _main_eta(m, broken), m.root, m.LEVELS, m.RADIUS, m.DELTA, m.wth, 4, method="blocks")
    _record(test="failed", nan_queries=int(bad_q.sum()))


# ------------------------------------------------------------------------------------------ distribution
def test_the_distribution_of_the_block_draws():
    import torch
    m = _main("f64")
    eta = _main_eta(m)
    rng = np.random.default_rng(9)
    centre = np.mean([x.mean(0) for x in m.Xs], 0)
    Xq = centre + rng.uniform(-0.5, 0.5, (8, 2))                 # the eight queries of test_posterior_draws (tests/test_gpu_cov.py)
    args = (Xq, eta, m.root, m.LEVELS, m.RADIUS, m.DELTA, m.wth)
    Yq, Vq, Cov = pmk.querymixtureGP_cov(*args)
    n = 4096
    dev = torch.device("cuda", 0)
    draws, jitter = pmk.samplemixtureGP(*args, n, generator=torch.Generator(device=dev).manual_seed(17), method="blocks")
    again, _ = pmk.samplemixtureGP(*args, n, generator=torch.Generator(device=dev).manual_seed(17), method="blocks")
    assert jitter == 0.0 and tuple(draws.shape) == (n, 8) and torch.equal(draws, again)
    x = draws.cpu().numpy() - Yq[None, :]
    samp = x.T @ x / n
    se = np.sqrt((np.outer(np.diag(Cov), np.diag(Cov)) + Cov ** 2) / n)
    z_worst = float((np.abs(samp - Cov) / se).max())
    # z passed in gives Yq + E of the staged calls, bit for bit
    q = M.DeviceQuery(eta._model, Xq)
    q.plan(m.RADIUS, m.DELTA)
    q.items_fitted()
    q.mix(m.wth)
    q.items_cov_blocks()
    q.factor_cov()
    z = np.random.default_rng(3).standard_normal((16, int(q.total)))
    dz, jz = pmk.samplemixtureGP(*args, 16, z=z, method="blocks")
    assert jz == 0.0 and np.array_equal(dz.cpu().numpy(), Yq[None, :] + q.draw(m.wth, z))
    with pytest.raises(ValueError, match="shape"):
        pmk.samplemixtureGP(*args, 16, z=z[:, :-1], method="blocks")
    # the default method is the dense one, unchanged
    dd, _ = pmk.samplemixtureGP(*args, 16, generator=torch.Generator(device=dev).manual_seed(17))
    de, _ = pmk.samplemixtureGP(*args, 16, generator=torch.Generator(device=dev).manual_seed(17), method="dense")
    assert torch.equal(dd, de)
    _record(test="distribution", worst_standard_errors=z_worst, draws=n)
    assert z_worst <= 6.0, z_worst


# ------------------------------------------------------------------------------------------ beyond the old limit
def test_a_batch_beyond_the_limit_of_the_dense_covariance():
    mm = CC.Many()
    th, _ = CC.FAMILIES["spline34"]
    P = len(mm.Xs)
    model = _fitted(mm.Xs, [np.ascontiguousarray(mm.y[i]) for i in mm.inds], th, "f64", mm.root)
    Nq = 16385
    Xq = np.random.default_rng(12).uniform(-3.9, 3.9, (Nq, 2))
    q = _planned(model, Xq, mm.RADIUS, mm.DELTA, th, mm.wth)
    L = pmk.lib()
    d, w = th.desc(), mm.wth.desc()
    assert L.pmk_query_items_cov(q.h, C.byref(d)) == -5
    q.items_cov_blocks(th)
    counts = np.diff(q.region_offsets(P))
    first, rel, jit = _ladder(q, P)
    assert L.pmk_query_mix_cov(q.h, C.byref(w)) == -5 and b"PMK_COV_MAX_QUERIES" in L.pmk_last_error()
    rng = np.random.default_rng(13)
    total = int(q.total)
    z = rng.standard_normal((4, total))
    E = q.draw(mm.wth, z)
    assert E.shape == (4, Nq) and np.all(np.isfinite(E))
    dbg = q.debug()
    off, reg = dbg["item_offsets"], dbg["item_region"]
    wn = np.asarray(CR.blend_weights(off, dbg["item_t"], mm.owth), dtype=np.float64)
    roff = q.region_offsets(P)
    # eight regions: the largest, two that needed jitter if there are such, the rest at random
    pick = [int(np.argmax(counts))] + [int(r) for r in np.nonzero(rel > 0)[0][:2]]
    pick += [int(r) for r in rng.permutation(P) if counts[r] > 0 and r not in pick][:8 - len(pick)]
    worst = _factor_worst({r: (q.item_covs(r)[0], q.item_covs(r)[1], q.item_cov_factor(r)) for r in pick}, jit)
    # 64 queries: E against the host blend of the fetched L_r z_r
    factors, blend = {}, 0.0
    for j in rng.choice(Nq, 64, replace=False):
        ref, mag = np.zeros(4), np.zeros(4)
        for i in range(off[j], off[j + 1]):
            r = int(reg[i])
            if r not in factors:
                factors[r] = (q.item_covs(r)[0], q.item_cov_factor(r))
            idx, Lr = factors[r]
            # the rows of query j in the block, in item order (two if the query holds two items of the region)
            a = np.nonzero(idx == j)[0][list(np.nonzero(reg[off[j]:off[j + 1]] == r)[0]).index(i - off[j])]
            zr = z[:, roff[r]:roff[r] + len(idx)]
            ref += wn[i] * (zr @ Lr[a])
            mag += wn[i] * (np.abs(zr) @ np.abs(Lr[a]))
        blend = max(blend, float((np.abs(E[:, j] - ref) / ((counts.max() + 8) * U53 * mag)).max()))
    _record(test="beyond", Nq=Nq, total=total, largest_block=int(counts.max()), regions_with_jitter=int((rel > 0).sum()),
            jitter=float(jit.max()), factor=worst, blend=blend)
    assert counts.max() >= 24 and worst <= RATIO_MAX and blend <= 1.0, (counts.max(), worst, blend)


# ------------------------------------------------------------------------------------------ refusals and state
def test_refusals_and_state():
    L = pmk.lib()
    m = _main("f64")
    th, _ = CC.FAMILIES["spline34"]
    d, w = th.desc(), m.wth.desc()
    model = _main_model(m, th, "f64")
    Xq = DR.main_queries(m)
    q = M.DeviceQuery(model, Xq)
    fi = np.zeros(4, dtype=np.int32)
    buf = np.zeros((64, 64))
    assert L.pmk_query_items_cov_blocks(q.h, C.byref(d), 0) == -1                # no plan
    assert L.pmk_query_factor_cov(q.h, None) == -1 and L.pmk_query_factor_info(q.h, None, None) == -1
    assert L.pmk_query_get_items_cov_factor(q.h, 0, None, None, 0) == -1
    q.plan(m.RADIUS, m.DELTA)
    q.items(th)
    q.mix(m.wth)
    total, Nq = int(q.total), len(Xq)
    z, E = np.zeros((2, total)), np.zeros((2, Nq))
    draw = lambda n=2, ldz=total, lde=Nq, wd=w, zz=z, ee=E: L.pmk_query_draw(
        q.h, C.byref(wd), n, None if zz is None else zz.ctypes.data, ldz, None if ee is None else ee.ctypes.data, lde)
    assert L.pmk_query_factor_cov(q.h, None) == -2 and b"blocks" in L.pmk_last_error()       # no blocks on this plan
    assert L.pmk_query_factor_info(q.h, None, None) == -2 and draw() == -2
    ms = pmk.ModulatedSqExpKernelType(2.0, 1.3).desc()
    assert L.pmk_query_items_cov_blocks(q.h, C.byref(ms), 0) == -2               # the checks of pmk_query_items_cov
    assert L.pmk_query_items_cov_blocks(q.h, C.byref(d), 1) == -3                # ... and of _multi: no multi-output solve
    q.items_cov_blocks(th)
    assert L.pmk_query_get_items_cov_factor(q.h, 0, None, None, 0) == -2 and draw() == -2    # before a factorisation
    assert L.pmk_query_factor_info(q.h, None, None) == -2
    bad = np.zeros(4)
    for v in (-1e-9, np.nan, np.inf):
        bad[1] = v
        assert L.pmk_query_factor_cov(q.h, M._d(bad)) == -2 and b"rel[1]" in L.pmk_last_error()
    assert L.pmk_query_get_items_cov_factor(q.h, 0, None, None, 0) == -2         # a refused call factors nothing
    q.factor_cov()
    assert L.pmk_query_factor_info(q.h, fi.ctypes.data_as(C.POINTER(C.c_int32)), None) == 0 and np.all(fi == 0)
    mr = C.c_int64()
    assert L.pmk_query_get_items_cov_factor(q.h, 0, C.byref(mr), None, 0) == 0 and mr.value == len(q.item_covs(0)[0])
    assert L.pmk_query_get_items_cov_factor(q.h, 4, None, None, 0) == -3         # not a leaf of the model
    assert L.pmk_query_get_items_cov_factor(q.h, 0, None, M._d(buf), mr.value - 1) == -4
    bb = pmk.BrownianBridge10(1.0).desc()
    assert draw(wd=bb) == -2 and b"stationary" in L.pmk_last_error()             # the blending profile
    assert draw(ldz=total - 1) == -4 and draw(lde=Nq - 1) == -4
    assert draw(zz=None) == -2 and draw(ee=None) == -2 and draw(n=-1) == -2
    assert draw(n=0, zz=None, ee=None) == 0
    assert draw() == 0
    first = q.draw(m.wth, np.ones((3, total)))
    # padded leading dimensions: the columns past total and Nq are neither read as items nor written
    zp, Ep = np.full((3, total + 5), np.nan), np.full((3, Nq + 2), -7.0)
    zp[:, :total] = 1.0
    assert L.pmk_query_draw(q.h, C.byref(w), 3, zp.ctypes.data, total + 5, Ep.ctypes.data, Nq + 2) == 0
    assert np.array_equal(Ep[:, :Nq], first) and np.all(Ep[:, Nq:] == -7.0)
    # new blocks discard the factors; so does a new plan, with the blocks
    q.items_cov(th)
    assert draw() == -2 and L.pmk_query_get_items_cov_factor(q.h, 0, None, None, 0) == -2
    q.factor_cov()
    assert np.array_equal(q.draw(m.wth, np.ones((3, total))), first)
    q.plan(0.3, m.DELTA)
    assert L.pmk_query_factor_cov(q.h, None) == -2 and draw() == -2
    q.items(th)
    q.mix(m.wth)
    q.items_cov_blocks(th)
    q.factor_cov()
    assert q.draw(m.wth, np.ones((1, int(q.total)))).shape == (1, Nq)
    # under a trend new items discard blocks and factors
    mm = _multi_main()
    tmodel = _multi_model(mm, "linear", 2)
    qt = M.DeviceQuery(tmodel, np.ascontiguousarray(mm.Xq[:DR.NQ_MAIN]))
    qt.plan(mm.RADIUS, mm.DELTA)
    qt.items_multi(th, True)
    qt.mix_multi(mm.wth)
    assert L.pmk_query_items_cov_blocks(qt.h, C.byref(d), 1) == 0 and L.pmk_query_factor_cov(qt.h, None) == 0
    qt.items_multi(th, True)
    assert L.pmk_query_factor_cov(qt.h, None) == -2 and L.pmk_query_factor_info(qt.h, None, None) == -2
    _record(test="state", total=total)
