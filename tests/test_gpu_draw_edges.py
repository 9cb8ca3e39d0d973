"""The block draws on the GPU at tile depth, chunk seams, R columns and jitter (the kernels of pmk_draw.hip, pmk_query_factor_cov
and pmk_query_draw, method="blocks" of samplemixtureGP and samplemixtureGP_multi).

Inputs: tests/_draw_edge_cases.py, whose conditions tests/test_draw_edges_refs.py checks on the CPU.  Units and bounds are
those of tests/test_gpu_draw.py:
  * a factor: |L L^T - (S + jitter I)| in units (m + 8) 2^-53 sqrt(S_aa S_bb), bound 10;
  * the blend: A A^T of the identity draw (long double on the host) against fetch_cov, bound the sum over the blended
    entries of wn wn' (10 block units + 8 x 2^-53 |S_ab|); where a region needed jitter both sides carry jitter_r W_r W_r^T;
  * a draw against the long-double host blend of the fetched factors: unit (m_max + 8) 2^-53 sum wn (|z| . |L_r[a]|), bound 1;
  * a distribution: 6 standard errors.

1. the lattice: every factor is 5 or 6 tiles deep, the identity draw takes three chunks (256, 256 and the rest);
2. a draw's bits do not depend on the call, the chunk or the leading dimensions it came in;
3. a pivot that fails in the third or fourth tile, and the retry that writes the tiles the first attempt left;
4. a query with two items of one region (tests/_cov_cases.Many, query 89 and region 88): the cross term under jitter;
5. every blending profile;
6. samplemixtureGP_multi(method="blocks").

Every measured ratio is printed ("DRAWEDGE {json}", run with -s) and a run of the whole module writes them to
profiles/draw_edges_accuracy.json.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import mixture as M
import _cov_cases as CC
import _cov_multi_cases as CMC
import _cov_refs as CR
import _draw_edge_cases as DE
import _draw_refs as DR
import _grad_edge_cases as GE
from test_draw_refs import pivot_rule
from test_gpu_cov import _fitted, _main, _main_model
from test_gpu_cov_multi import _corner_queries, _main as _multi_main, _main_model as _multi_model
from test_gpu_draw import _blocks, _dense_check, _factor_worst, _identity_draw, _ladder, _main_eta, _planned, _weights
from test_gpu_grad import _worst_ratio

pytestmark = pytest.mark.gpu

LD, U53, RATIO_MAX, SIGMA2 = DR.LD, DR.U53, DR.RATIO_MAX, CC.SIGMA2
_RECORDS = []
ACCURACY_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "draw_edges_accuracy.json")
ALL_TESTS = {"lattice", "lattice_trend", "chunks", "one_query", "seam", "doubled", "profile", "multi", "multi_refusals",
             "list_and_tree"}
_MODELS = {}


def _record(**kw):
    _RECORDS.append(kw)
    print("DRAWEDGE " + json.dumps(kw, sort_keys=True))


@pytest.fixture(scope="module", autouse=True)
def _write_accuracy_file():
    """only a run of the whole module replaces the file"""
    yield
    if {r["test"] for r in _RECORDS} >= ALL_TESTS:
        with open(ACCURACY_JSON, "w") as f:
            f.write("[\n" + ",\n".join(" " + json.dumps(r, sort_keys=True) for r in _RECORDS) + "\n]\n")


def _model(family="spline34", dtype="f64"):
    """the main workload's model, fitted once per family and precision"""
    if (family, dtype) not in _MODELS:
        _MODELS[(family, dtype)] = _main_model(_main(dtype), CC.FAMILIES[family][0], dtype)
    return _MODELS[(family, dtype)]


def _deep(q, P=4):
    counts = np.diff(q.region_offsets(P))
    assert counts.min() > 2 * DE.TILE and np.any(counts % DE.TILE) and q.total > 512 and q.total % DE.TILE, counts
    return [int(c) for c in counts]


def _host_blend_worst(q, P, owth, z, E, queries):
    """worst |E[:, j] - sum_i wn_i (L_r z_r)[a(i)]| over the given queries, the sum in long double from the fetched factors,
    in units (m_max + 8) 2^-53 sum_i wn_i (|z_r| . |L_r[a(i)]|)"""
    dbg = q.debug()
    off, reg = dbg["item_offsets"], dbg["item_region"]
    wn = CR.blend_weights(off, dbg["item_t"], owth)
    roff = q.region_offsets(P)
    m_max = int(np.diff(roff).max())
    zl = np.asarray(z, dtype=LD)
    fac, worst = {}, 0.0
    for j in queries:
        ref, mag = np.zeros(len(z), dtype=LD), np.zeros(len(z), dtype=LD)
        for i in range(off[j], off[j + 1]):
            r = int(reg[i])
            if r not in fac:
                fac[r] = (q.item_covs(r)[0], np.asarray(q.item_cov_factor(r), dtype=LD))
            idx, Lr = fac[r]
            # the rows of query j in the block, in item order (two if the query holds two items of the region)
            a = np.nonzero(idx == j)[0][list(np.nonzero(reg[off[j]:off[j + 1]] == r)[0]).index(i - off[j])]
            zr = zl[:, roff[r]:roff[r] + len(idx)]
            ref += wn[i] * (zr @ Lr[a])
            mag += wn[i] * (np.abs(zr) @ np.abs(Lr[a]))
        worst = max(worst, float((np.abs(E[:, j] - ref) / ((m_max + 8) * U53 * mag)).max()))
    return worst


# ------------------------------------------------------------------------------------------ 1. the lattice
@pytest.mark.parametrize("family,dtype", [("spline34", "f64"), ("gaussian", "f64"), ("spline34", "f32")])
def test_multi_tile_factors_under_the_blend(family, dtype):
    m = _main(dtype)
    th, _ = CC.FAMILIES[family]
    q = _planned(_model(family, dtype), DE.lattice_queries(dtype), m.RADIUS, m.DELTA, th, m.wth)
    q.items_cov(th)
    q.mix_cov(m.wth)
    Cov = q.fetch_cov()
    q.factor_cov()
    finfo, jit = q.factor_info()
    assert np.all(finfo == 0) and np.all(jit == 0.0)
    counts = _deep(q)
    factor, blend = _dense_check(q, 4, m.wth, m.owth, Cov)       # n = total draws: chunks of 256, 256 and the rest
    _record(test="lattice", family=family, dtype=dtype, factor=factor, blend=blend, region_items=counts, total=int(q.total))
    assert factor <= RATIO_MAX and blend <= RATIO_MAX, (factor, blend)


def test_multi_tile_factors_under_a_linear_trend_with_two_columns():
    m = _multi_main()
    th = CC.FAMILIES["spline34"][0]
    q = M.DeviceQuery(_multi_model(m, "linear", 2), DE.lattice_queries())
    q.plan(m.RADIUS, m.DELTA)
    q.items_multi(th, True)
    q.mix_multi(m.wth)
    q.items_cov_multi(th)
    q.mix_cov(m.wth)
    Cov = q.fetch_cov()
    q.items_cov_blocks(th, multi=True)
    q.factor_cov()
    finfo, jit = q.factor_info()
    assert np.all(finfo == 0) and np.all(jit == 0.0)
    counts = _deep(q)
    factor, blend = _dense_check(q, 4, m.wth, m.owth, Cov)
    _record(test="lattice_trend", factor=factor, blend=blend, region_items=counts, total=int(q.total))
    assert factor <= RATIO_MAX and blend <= RATIO_MAX, (factor, blend)


# ------------------------------------------------------------------------------------------ 2. chunks
def _lattice_factored(radius=None):
    m = _main("f64")
    th, _ = CC.FAMILIES["spline34"]
    q = _planned(_model(), DE.lattice_queries(), m.RADIUS if radius is None else radius, m.DELTA, th, m.wth)
    q.items_cov_blocks(th)
    q.factor_cov()
    assert np.all(q.factor_info()[0] == 0)
    return m, q


def test_the_bits_of_a_draw_do_not_depend_on_its_chunk():
    import torch
    m, q = _lattice_factored()
    total, Nq, n = int(q.total), q.Nq, DE.N_CHUNK_DRAWS
    _deep(q)
    z = np.random.default_rng(DE.Z_SEED).standard_normal((n, total))
    E = q.draw(m.wth, z)
    assert E.shape == (n, Nq) and np.all(np.isfinite(E))
    # separate calls: the rows on both sides of the seam at 256 come from other chunks, at other offsets
    assert sum(DE.SPLITS) == n
    s = 0
    for k in DE.SPLITS:
        assert np.array_equal(q.draw(m.wth, np.ascontiguousarray(z[s:s + k])), E[s:s + k]), (s, k)
        s += k
    for s in DE.ALONE:
        assert np.array_equal(q.draw(m.wth, np.ascontiguousarray(z[s:s + 1])), E[s:s + 1]), s
    # padded leading dimensions from host arrays: the staging buffers are re-based per chunk
    L, w = pmk.lib(), m.wth.desc()
    zp, Ep = np.full((n, total + 5), np.nan), np.full((n, Nq + 2), -7.0)
    zp[:, :total] = z
    assert L.pmk_query_draw(q.h, C.byref(w), n, zp.ctypes.data, total + 5, Ep.ctypes.data, Nq + 2) == 0
    assert np.array_equal(Ep[:, :Nq], E) and np.all(Ep[:, Nq:] == -7.0)
    assert np.array_equal(zp[:, :total], z) and np.all(np.isnan(zp[:, total:]))
    # ... and from device tensors: E + lde s0 and z + ldz s0 with no staging
    dev = torch.device("cuda", q.model.ctx.device)
    zt = torch.as_tensor(zp, device=dev)
    Et = torch.full((n, Nq + 2), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    q.draw(m.wth, zt[:, :total], out=Et[:, :Nq])
    q.model.ctx.synchronize()
    Eh, zh = Et.cpu().numpy(), zt.cpu().numpy()
    assert np.array_equal(Eh[:, :Nq], E) and np.all(Eh[:, Nq:] == -7.0)
    assert np.array_equal(zh[:, :total], z) and np.all(np.isnan(zh[:, total:]))
    # 64 queries against the long-double host blend of the fetched L_r z_r
    m_max = int(np.diff(q.region_offsets(4)).max())
    worst = _host_blend_worst(q, 4, m.owth, z, E, np.random.default_rng(22).choice(Nq, 64, replace=False))
    _record(test="chunks", draws=n, total=total, largest_block=m_max, host_blend=worst)
    assert worst <= 1.0, worst


def test_a_single_query():
    m = _main("f64")
    th, _ = CC.FAMILIES["spline34"]
    Xl = DE.lattice_queries()
    full = _planned(_model(), Xl, m.RADIUS, m.DELTA, th, m.wth)
    j = int(np.argmax(np.diff(full.debug()["item_offsets"])))    # a query that blends as many regions as any
    q = _planned(_model(), np.ascontiguousarray(Xl[j:j + 1]), m.RADIUS, m.DELTA, th, m.wth)
    q.items_cov(th)
    q.mix_cov(m.wth)
    Cov = q.fetch_cov()
    q.factor_cov()
    finfo, jit = q.factor_info()
    total = int(q.total)
    assert q.Nq == 1 and Cov.shape == (1, 1) and total >= 2 and np.all(finfo == 0) and np.all(jit == 0.0)
    blocks = _blocks(q, 4)
    assert len(blocks) == total and all(S.shape == (1, 1) for _, S, _ in blocks.values())     # every block is one row
    rng = np.random.default_rng(23)
    for n in (1, 33):
        E = q.draw(m.wth, rng.standard_normal((n, total)))
        assert E.shape == (n, 1) and np.all(np.isfinite(E)) and np.all(E != 0)
    W, roff, _ = _weights(q, m.owth)
    A = _identity_draw(q, m.wth)
    assert A.shape == (1, total) and np.all(A != 0)
    Wd = np.asarray(W, dtype=np.float64)
    bound = sum(float(Wd[0, roff[r]] ** 2 * (RATIO_MAX * DR.block_unit(S) + 8 * U53 * np.abs(S))[0, 0]) for r, (_, S, _) in blocks.items())
    AAt = float(np.abs(np.asarray(A, dtype=LD) @ np.asarray(A, dtype=LD).T - LD(Cov[0, 0]))[0, 0])
    blend = RATIO_MAX * AAt / bound
    _record(test="one_query", query=j, items=total, blend=blend, factor=_factor_worst(blocks))
    assert blend <= RATIO_MAX and _factor_worst(blocks) <= RATIO_MAX, blend


# ------------------------------------------------------------------------------------------ 3. a failed pivot past the first tile
_SEAM_BASE = {}


def _seam_base():
    """the lattice at radius 0 without a copy: the factors every unaffected region must keep"""
    if not _SEAM_BASE:
        m, q = _lattice_factored(0.0)
        _SEAM_BASE.update(blocks=_blocks(q, 4), seams=DE.seam_batches(m))
    return _SEAM_BASE["blocks"], _SEAM_BASE["seams"]


@pytest.mark.parametrize("name", DE.SEAMS)
def test_a_pivot_that_fails_past_the_first_tile_and_the_retry(name):
    m = _main("f64")
    th, _ = CC.FAMILIES["spline34"]
    base, seams = _seam_base()
    case = seams[name]
    Xq, r_star, row, first_q, copy_q = case["Xq"], case["region"], case["row"], case["first"], case["copy"]
    others = [r for r in range(4) if r != r_star]
    q = _planned(_model(), Xq, 0.0, m.DELTA, th, m.wth)
    reg = q.debug()["item_region"]
    assert q.total == q.Nq and reg[first_q] == r_star and reg[copy_q] == r_star
    q.items_cov(th)
    idx, S_star = q.item_covs(r_star)
    assert int(idx[row]) == copy_q and int(idx[DE.SEAM_FIRST_ROW]) == first_q and len(idx) == len(base[r_star][0]) + 1
    # the CPU mirror of the pivot rule on the device's own block: where it fails, and the rung it passes at
    want = pivot_rule(S_star)
    rung = [rel for rel in DE.ladder_rungs() if pivot_rule(S_star, rel * np.trace(S_star) / len(idx)) == 0][0]
    assert want == row + 1 and row >= 2 * DE.TILE, (want, row)
    q.factor_cov(np.zeros(4))
    finfo, jit0 = q.factor_info()
    assert finfo[r_star] == want and np.all(finfo[others] == 0) and np.all(jit0 == 0.0), (finfo, want)
    # an entry of a factor is a function of its region's block and jitter alone
    for r in others:
        assert np.array_equal(q.item_covs(r)[1], base[r][1]) and np.array_equal(q.item_cov_factor(r), base[r][2]), r
    # the ladder: after every call of it the other regions hold the same bits
    plain, rels = q.factor_cov, []

    def watched(rel=None):
        plain(rel)
        rels.append(np.array(rel, dtype=np.float64))
        for r in others:
            assert np.array_equal(q.item_cov_factor(r), base[r][2]), (r, rel)
    q.factor_cov = watched
    first, rel, jit = _ladder(q, 4)
    q.factor_cov = plain
    assert first[r_star] == want and np.all(first[others] == 0)
    assert rel[r_star] == rung and np.all(rel[others] == 0) and jit[r_star] > 0 and np.all(jit[others] == 0), (rel, rung)
    assert len(rels) >= 2 and all(np.all(x[others] == 0) for x in rels) and np.all(np.diff([x[r_star] for x in rels]) > 0)
    blocks = _blocks(q, 4)
    retry, rest = _factor_worst({r_star: blocks[r_star]}, jit), _factor_worst({r: blocks[r] for r in others})
    # 64 draws: the two copies differ by sqrt(2 jitter) times a standard normal, up to the rounding the jitter covers
    z = np.random.default_rng(24).standard_normal((64, int(q.total)))
    E = q.draw(m.wth, z)
    assert np.all(np.isfinite(E))
    gap = float(np.abs(E[:, first_q] - E[:, copy_q]).max())
    gap_max = 6.0 * np.sqrt(2 * jit[r_star]) + 64 * U53 * np.abs(E[:, first_q]).max()
    _record(test="seam", seam=name, region=r_star, rows=len(idx), finfo=int(want), rel=float(rung), jitter=float(jit[r_star]),
            retry_factor=retry, other_factors=rest, gap=gap, gap_max=float(gap_max))
    assert retry <= RATIO_MAX and rest <= RATIO_MAX and 0 < gap <= gap_max, (retry, rest, gap, gap_max)
    assert float(np.std(E[:, first_q])) > 1e3 * gap


# ------------------------------------------------------------------------------------------ 4. two items of one region
def test_two_items_of_one_region_in_one_query_under_jitter():
    mm = CC.Many()
    th, _ = CC.FAMILIES["spline34"]
    P = len(mm.Xs)
    model = _fitted(mm.Xs, [np.ascontiguousarray(mm.y[i]) for i in mm.inds], th, "f64", mm.root)
    q = _planned(model, mm.Xq, mm.RADIUS, mm.DELTA, th, mm.wth)
    dbg = q.debug()
    off, reg = dbg["item_offsets"], dbg["item_region"]
    assert list(reg[off[89]:off[90]]).count(88) == 2             # tests/test_cov_refs.py asserts it of the oracle's plan
    q.items_cov(th)
    q.mix_cov(mm.wth)
    Cov = q.fetch_cov()
    first, rel, jit = _ladder(q, P)
    assert first[88] > 0 and rel[88] > 0 and jit[88] > 0          # the doubled row is singular
    assert np.all((rel > 0) == (first > 0)) and np.all((jit > 0) == (rel > 0))
    blocks = _blocks(q, P)
    W, roff, items = _weights(q, mm.owth)
    A = _identity_draw(q, mm.wth)
    Wd = np.asarray(W, dtype=np.float64)
    Nq = q.Nq
    AAt, ref, bound = np.zeros((Nq, Nq), dtype=LD), np.asarray(Cov, dtype=LD).copy(), np.zeros((Nq, Nq))
    for r, (idx, S, L) in blocks.items():
        cols = slice(roff[r], roff[r] + len(idx))
        rows = np.nonzero((Wd[:, cols] != 0).any(1))[0]
        assert np.all(np.delete(A[:, cols], rows, axis=0) == 0), r
        ix = np.ix_(rows, rows)
        Ar, Wr = np.asarray(A[rows][:, cols], dtype=LD), W[rows][:, cols]
        AAt[ix] += Ar @ Ar.T
        ref[ix] += LD(jit[r]) * (Wr @ Wr.T)
        Sj = S + jit[r] * np.eye(len(S))
        bound[ix] += Wd[rows][:, cols] @ (RATIO_MAX * DR.block_unit(Sj) + 8 * U53 * np.abs(Sj)) @ Wd[rows][:, cols].T
    shared = CR.shared_region_mask(items)
    assert not shared.all() and np.all(AAt[~shared] == 0) and np.all(Cov[~shared] == 0) and np.all(bound[~shared] == 0)
    err = np.abs(AAt - ref).astype(np.float64)
    blend = RATIO_MAX * _worst_ratio(err, bound)
    # the query with two items: its variance carries 2 wn wn' S_ab of the pair, and its row the sum of both items' terms
    idx88 = blocks[88][0]
    mates = [int(k) for k in np.unique(idx88) if k != 89]
    assert list(idx88).count(89) == 2 and mates
    a, b = [int(v) for v in np.nonzero(idx88 == 89)[0]]
    cross = 2 * Wd[89, roff[88] + a] * Wd[89, roff[88] + b] * blocks[88][1][a, b]
    own = RATIO_MAX * float(err[89, 89] / bound[89, 89])
    row = RATIO_MAX * float((err[89, mates] / bound[89, mates]).max())
    factor = _factor_worst(blocks, jit)
    # the two rows of query 89 in L_88 differ by the jitter's sqrt(2 jitter) alone, which A A^T squares away: a draw against
    # the long-double host blend tells the two item positions apart
    z = np.random.default_rng(25).standard_normal((4, int(q.total)))
    E = q.draw(mm.wth, z)
    host = _host_blend_worst(q, P, mm.owth, z, E, [89] + mates)
    second = float(Wd[89, roff[88] + b] * blocks[88][2][b, b] * np.abs(z[:, roff[88] + b]).min())
    assert second > 1e3 * (len(idx88) + 8) * U53 * np.abs(E[:, 89]).max()       # the second item's own column is no rounding
    _record(test="doubled", host_blend=host, second_item_term=second, factor=factor, blend=blend, entry_89_89=own,
            row_89_region_88=row, jitter=float(jit[88]), rel=float(rel[88]),
            cross_term_in_bounds=float(cross / bound[89, 89]), regions_with_jitter=int((rel > 0).sum()), total=int(q.total))
    assert cross > 1e3 * bound[89, 89]                            # without the cross term the entry is far outside its bound
    assert factor <= RATIO_MAX and blend <= RATIO_MAX and own <= RATIO_MAX and row <= RATIO_MAX, (factor, blend, own, row)
    assert host <= 1.0, host


# ------------------------------------------------------------------------------------------ 5. every blending profile
@pytest.mark.parametrize("name", sorted(GE.weight_kernels(1.0)))
def test_every_blending_profile(name):
    m = _main("f64")
    th, _ = CC.FAMILIES["spline34"]
    wth, owth = GE.weight_kernels(m.RADIUS)[name]
    L, w = pmk.lib(), wth.desc()
    Xq = DR.main_queries(m)
    q = _planned(_model(), Xq, m.RADIUS, m.DELTA, th, m.wth)
    q.items_cov(th)
    q.factor_cov()
    total = int(q.total)
    z, E = np.zeros((1, total)), np.zeros((1, len(Xq)))
    rc = L.pmk_query_mix_cov(q.h, C.byref(w))
    assert L.pmk_query_draw(q.h, C.byref(w), 1, z.ctypes.data, total, E.ctypes.data, len(Xq)) == rc      # refused alike
    # a Brownian-bridge profile is no profile, for the covariance and for the draw
    bb = pmk.BrownianBridge10(1.0).desc()
    rb = L.pmk_query_mix_cov(q.h, C.byref(bb))
    assert rb != 0 and L.pmk_query_draw(q.h, C.byref(bb), 1, z.ctypes.data, total, E.ctypes.data, len(Xq)) == rb
    assert rc == 0, (name, rc)                                   # the seven profiles of the mix are profiles of the draw
    q.mix(wth)
    q.mix_cov(wth)
    Cov = q.fetch_cov()
    q.factor_cov()
    factor, blend = _dense_check(q, 4, wth, owth, Cov)
    _record(test="profile", profile=name, factor=factor, blend=blend)
    assert factor <= RATIO_MAX and blend <= RATIO_MAX, (factor, blend)


# ------------------------------------------------------------------------------------------ 6. the R columns
def _multi_eta(m, trend, R=3):
    Y = CMC.targets(m.X, R)
    eta = pmk.MixtureGPType(m.Xs, pmk.fetchhyperplanes(m.root))
    pmk.fitmixtureGP_trend_(eta, [np.ascontiguousarray(Y[i]) for i in m.inds], CC.FAMILIES["spline34"][0], SIGMA2["f64"], trend)
    eta._model.set_bsp(m.root, 0)
    return eta


@pytest.mark.parametrize("trend", CMC.TRENDS)
def test_block_draws_of_the_columns(trend):
    import torch
    m = _multi_main()
    R = 3
    eta = _multi_eta(m, trend, R)
    Xq = _corner_queries(m)
    args = (Xq, eta, m.root, m.LEVELS, m.RADIUS, m.DELTA, m.wth)
    # z passed in: column c is Yq[:, c] + E of the staged calls on z[:, :, c], bit for bit
    q = M.DeviceQuery(eta._model, Xq)
    q.plan(m.RADIUS, m.DELTA)
    q.items_multi_fitted()
    q.mix_multi(m.wth)
    q.items_cov_blocks(None, multi=True)
    q.factor_cov()
    finfo, jit = q.factor_info()
    assert np.all(finfo == 0) and np.all(jit == 0.0)
    Yq, _ = q.fetch_multi(R)
    total = int(q.total)
    z = np.random.default_rng(3).standard_normal((16, total, R))
    dz, jz = pmk.samplemixtureGP_multi(*args, 16, z=z, method="blocks")
    assert jz == 0.0 and tuple(dz.shape) == (16, 8, R)
    dz = dz.cpu().numpy()
    for c in range(R):
        assert np.array_equal(dz[:, :, c], Yq[:, c][None, :] + q.draw(m.wth, np.ascontiguousarray(z[:, :, c]))), c
    for bad in (z[:, :, :2], z[:, :-1, :], z[:, :, 0]):
        with pytest.raises(ValueError, match="z must have shape"):
            pmk.samplemixtureGP_multi(*args, 16, z=bad, method="blocks")
    # seeded: equal generators give equal draws; their distribution is that of querymixtureGP_cov_multi, column by column
    n = 4096
    dev = torch.device("cuda", 0)
    draws, jitter = pmk.samplemixtureGP_multi(*args, n, generator=torch.Generator(device=dev).manual_seed(17), method="blocks")
    again, _ = pmk.samplemixtureGP_multi(*args, n, generator=torch.Generator(device=dev).manual_seed(17), method="blocks")
    assert jitter == 0.0 and tuple(draws.shape) == (n, 8, R) and torch.equal(draws, again)
    Ym, _, Cov = pmk.querymixtureGP_cov_multi(*args)
    assert np.array_equal(Ym, Yq)
    x = draws.cpu().numpy() - Ym[None, :, :]
    se = np.sqrt((np.outer(np.diag(Cov), np.diag(Cov)) + Cov ** 2) / n)
    z_worst = max(float((np.abs(x[:, :, c].T @ x[:, :, c] / n - Cov) / se).max()) for c in range(R))
    se_cross = np.sqrt(np.outer(np.diag(Cov), np.diag(Cov)) / n)                 # Var(x_j y_k) for independent x, y
    z_cross = max(float((np.abs(x[:, :, a].T @ x[:, :, b] / n) / se_cross).max()) for a in range(R) for b in range(a + 1, R))
    _record(test="multi", trend=trend, R=R, total=total, worst_standard_errors=z_worst, worst_cross_standard_errors=z_cross, draws=n)
    assert z_worst <= 6.0 and z_cross <= 6.0, (z_worst, z_cross)


def test_a_flagged_trend_is_refused_before_any_draw(monkeypatch):
    m = _multi_main()
    R = 3
    Xs = list(m.Xs)
    Xs[2] = np.ascontiguousarray(Xs[2][:2])                      # n = 2 < q = 3: the trend of this patch is flagged
    bad = pmk.MixtureGPType(Xs, pmk.fetchhyperplanes(m.root))
    with pytest.raises(pmk.TrendRankException):
        pmk.fitmixtureGP_trend_(bad, [CMC.targets(x, R) for x in Xs], CC.FAMILIES["spline34"][0], SIGMA2["f64"], "linear")
    called = []                                                 # the fit stopped at the flag: the model is resident all the same
    plain = M.DeviceQuery.draw
    monkeypatch.setattr(M.DeviceQuery, "draw", lambda self, *a, **k: called.append(1) or plain(self, *a, **k))
    with pytest.raises(np.linalg.LinAlgError, match="region 2 "):
        pmk.samplemixtureGP_multi(_corner_queries(m), bad, m.root, m.LEVELS, m.RADIUS, m.DELTA, m.wth, 4, method="blocks")
    assert not called
    _record(test="multi_refusals", flagged_region=2)


def test_block_draws_on_a_list_built_and_a_tree_built_eta():
    """The same z through a list-built and a from_tree eta must give np.array_equal draws."""
    th = CC.FAMILIES["spline34"][0]
    out = {}
    # the single-output front end on the main workload
    m = _main("f64")
    Xq = np.mean([x.mean(0) for x in m.Xs], 0) + np.random.default_rng(9).uniform(-0.5, 0.5, (8, 2))
    eta = _main_eta(m, _model())
    tree = pmk.MixtureGPType.from_tree(m.root, m.X, eps=m.EPS)
    pmk.fitmixtureGP_(tree, np.ascontiguousarray(m.y), th, SIGMA2["f64"])
    q = _planned(_model(), Xq, m.RADIUS, m.DELTA, th, m.wth)
    z = np.random.default_rng(4).standard_normal((16, int(q.total)))
    a, ja = pmk.samplemixtureGP(Xq, eta, m.root, m.LEVELS, m.RADIUS, m.DELTA, m.wth, 16, z=z, method="blocks")
    b, jb = pmk.samplemixtureGP(Xq, tree, m.root, m.LEVELS, m.RADIUS, m.DELTA, m.wth, 16, z=z, method="blocks")
    assert ja == 0.0 and jb == 0.0 and tuple(a.shape) == tuple(b.shape) == (16, 8)
    out["single"] = (a.cpu().numpy(), b.cpu().numpy())
    # the R columns under a linear trend
    mm = _multi_main()
    R = 3
    Xm = _corner_queries(mm)
    etam = _multi_eta(mm, "linear", R)
    treem = pmk.MixtureGPType.from_tree(mm.root, mm.X, eps=mm.EPS)
    pmk.fitmixtureGP_trend_(treem, np.asfortranarray(CMC.targets(mm.X, R)), th, SIGMA2["f64"], "linear")
    qm = M.DeviceQuery(etam._model, Xm)
    qm.plan(mm.RADIUS, mm.DELTA)
    zm = np.random.default_rng(5).standard_normal((16, int(qm.total), R))
    a, ja = pmk.samplemixtureGP_multi(Xm, etam, mm.root, mm.LEVELS, mm.RADIUS, mm.DELTA, mm.wth, 16, z=zm, method="blocks")
    b, jb = pmk.samplemixtureGP_multi(Xm, treem, mm.root, mm.LEVELS, mm.RADIUS, mm.DELTA, mm.wth, 16, z=zm, method="blocks")
    assert ja == 0.0 and jb == 0.0 and tuple(a.shape) == tuple(b.shape) == (16, 8, R)
    out["multi"] = (a.cpu().numpy(), b.cpu().numpy())
    diff = {k: float(np.abs(x - y).max() / np.abs(x).max()) for k, (x, y) in out.items()}
    _record(test="list_and_tree", single_rel_diff=diff["single"], multi_rel_diff=diff["multi"])
    assert np.array_equal(*out["single"]) and np.array_equal(*out["multi"]), diff
