"""CPU checks of the inputs of tests/test_gpu_draw_edges.py (tests/_draw_edge_cases.py): the conditions the GPU tests assume
hold of the reference alone, and the jitter ladder of the front ends driven without a device.

1. The lattice workload, on the model of _cov_cases.Main and under a linear trend on that of _cov_multi_cases.Main: every
   region block is at least three tiles of 32 deep, one of them is no multiple of the tile, the batch holds more than 512
   items (an identity draw crosses two chunk seams) and no multiple of 32, kappa2(S_r) <= 10^3 (the Gaussian family:
   <= 10^9, see test_the_lattice_workload), numpy.linalg.cholesky stays
   under one unit (m + 8) 2^-53 sqrt(S_aa S_bb), the device's pivot rule passes every block at rel = 0, and A A^T of
   _draw_refs.blend_matrix equals _cov_refs.mix_cov_ref to long-double rounding.
2. The seam batches: the pivot rule fails the block of the chosen region exactly at the second copy's row, which is the first
   row of tile 2, the last row of tile 2 or the last row of the block, passes every other region, and passes the chosen one
   on the ladder; the rung is printed.
3. The 512-leaf workload: with the jitter the ladder ends on, A A^T = Cov + sum_r jitter_r W_r W_r^T in long double on the
   rows of the queries of the doubled region, the cross term of the query with two items included.
4. mixture._sample_blocks on a stand-in query (no device, no library): the rel arrays it hands to factor_cov, rung by rung,
   the region LinAlgError names at the ladder's end, and the refusal of a failed patch that holds items.

Every measured condition is printed ("DRAWEDGEREF ...", run with -s).
"""
import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import mixture as M
import _cov_cases as CC
import _cov_multi_cases as CMC
import _cov_multi_refs as CMR
import _cov_refs as CR
import _draw_edge_cases as DE
import _draw_refs as DR
from test_draw_refs import _check_workload, _ref_blocks, pivot_rule

LD = DR.LD


# ------------------------------------------------------------------------------------------ 1. the lattice
def _lattice_conditions(name, items, S_blocks, kappa_max=CC.KAPPA_MAX):
    """the conditions of the docstring on the blocks of one plan of the lattice"""
    sizes = [len(S_blocks[r][0]) for r in sorted(S_blocks)]
    tiles = [-(-s // DE.TILE) for s in sizes]
    total = int(items[0][-1])
    kappa = lapack = 0.0
    for r, (idx, S) in S_blocks.items():
        Sd = np.asarray(S, dtype=np.float64)
        assert np.all(np.diff(idx) > 0), r                      # no query holds two items of a region, none is repeated
        kappa = max(kappa, DR.kappa2(Sd))
        lapack = max(lapack, DR.factor_ratio(np.linalg.cholesky(Sd), Sd))
        assert pivot_rule(Sd) == 0, r
    print("DRAWEDGEREF %s: region sizes %s, tiles %s, total %d; kappa2(S) <= %.3g; LAPACK worst L L^T ratio %.3g"
          % (name, sizes, tiles, total, kappa, lapack))
    assert len(sizes) == 4 and sum(sizes) == total
    assert min(tiles) >= 3 and any(s % DE.TILE for s in sizes), sizes
    assert total > 512 and total % DE.TILE != 0, total
    assert kappa <= kappa_max and lapack <= 1.0, (kappa, lapack)


@pytest.mark.parametrize("family,dtype", [("spline34", "f64"), ("gaussian", "f64"), ("spline34", "f32")])
def test_the_lattice_workload(family, dtype):
    """kappa2(S_r) <= 10^3 is asserted of the Spline34 blocks in both precisions (measured 411 and 557) and under the trend
    (759).  The posterior blocks of the Gaussian family cannot meet it on this model: 1.08 x 10^4 on this lattice, 5.5 x 10^4
    on 24 x 20 nodes moved by 0.1, 1.2 x 10^4 on 21 x 19 nodes moved by 0.03, and a lattice needs about this density to hold
    more than 512 items on [-3.8, 3.8]^2: a smooth kernel's posterior spectrum falls that fast at this spacing.  What the GPU test of that family assumes is only that every block
    factors in double without jitter: the pivot rule passes, numpy.linalg.cholesky stays under one unit, and kappa2 is within
    _draw_refs.KAPPA_S_MAX = 10^9, the bound tests/test_draw_refs.py puts on every block factored without jitter."""
    m = CC.Main(dtype)
    sub = DE.lattice(m)
    assert sub.Xq.shape == (DE.NX * DE.NY, 2) and len(np.unique(sub.Xq, axis=0)) == DE.NX * DE.NY
    items = CC.oracle_items(sub)
    name = "lattice %s %s" % (family, dtype)
    S_blocks = _check_workload(name, CC.FAMILIES[family][1], m.Xs, CC.SIGMA2[dtype], items, sub.Xq, m.owth)
    _lattice_conditions(name, items, S_blocks, CC.KAPPA_MAX if family == "spline34" else DR.KAPPA_S_MAX)


def test_the_lattice_under_a_linear_trend():
    m = CMC.Main()
    sub = DE.lattice(m)
    items = CC.oracle_items(sub)
    oth = CC.FAMILIES["spline34"][1]
    S_blocks = {r: (idx, CMR.TrendRegionRef(oth, m.Xs[r], CC.SIGMA2["f64"], "linear").cov(pts)["S"])
                for r, (idx, pts) in CC.blocks_of(items, sub.Xq).items()}
    Cov = CR.mix_cov_ref(items[:2], S_blocks, items[2], m.owth)
    A = DR.blend_matrix(items[:2], DR.region_factors(S_blocks), items[2], m.owth)
    scale = np.sqrt(np.outer(np.diag(Cov), np.diag(Cov))).astype(np.float64)
    AAt = A @ A.T
    err = float((np.abs(AAt - Cov).astype(np.float64) / scale).max())
    assert np.all(AAt[~CR.shared_region_mask(items[:2])] == 0)
    print("DRAWEDGEREF lattice linear trend: A A^T against mix_cov_ref %.3g of sqrt(C_jj C_kk)" % err)
    assert err <= 1e3 * float(np.finfo(LD).eps), err           # the bound of test_draw_refs._check_workload
    _lattice_conditions("lattice linear trend", items, S_blocks)


# ------------------------------------------------------------------------------------------ 2. the seams
def test_the_seam_batches_fail_at_the_second_copy_and_pass_on_the_ladder():
    m = CC.Main("f64")
    oth = CC.FAMILIES["spline34"][1]
    seams = DE.seam_batches(m)
    assert tuple(seams) == DE.SEAMS
    for name, case in seams.items():
        Xq, r_star, row = case["Xq"], case["region"], case["row"]
        assert np.array_equal(Xq[case["copy"]], Xq[case["first"]]) and case["first"] < case["copy"]
        sub = DR.MainSub(m, Xq)
        sub.RADIUS = 0.0                                         # home items only: one region holds the two copies
        items = CC.oracle_items(sub)
        assert np.all(np.diff(items[0]) == 1)
        S_blocks = _ref_blocks(oth, m.Xs, CC.SIGMA2["f64"], items, Xq)
        for r, (idx, S) in S_blocks.items():
            Sd = np.asarray(S, dtype=np.float64)
            k = pivot_rule(Sd)
            if r != r_star:
                assert k == 0, (name, r, k)
                continue
            mr = len(idx)
            assert mr == case["rows_before"] + 1 and mr >= 3 * DE.TILE + 1
            assert int(idx[row]) == case["copy"] and int(idx[DE.SEAM_FIRST_ROW]) == case["first"]
            want = {"tile_first": DE.TILE * DE.SEAM_TILE, "tile_last": DE.TILE * DE.SEAM_TILE + DE.TILE - 1, "block_last": mr - 1}
            assert row == want[name] and row >= 2 * DE.TILE and k == row + 1, (name, row, k)
            if name != "block_last":
                assert row < mr - 1                              # rows after the failed pivot: tiles the first attempt leaves
            rungs = DE.ladder_rungs()
            passed = [i for i, rel in enumerate(rungs) if pivot_rule(Sd, rel * np.trace(Sd) / mr) == 0]
            assert passed, name
            print("DRAWEDGEREF seam %s: region %d of %d rows fails at pivot %d (tile %d, row %d of it), passes at rel = "
                  "2^-52 x 10^%d" % (name, r, mr, k, row // DE.TILE, row % DE.TILE, passed[0]))


# ------------------------------------------------------------------------------------------ 3. the jitter term of the blend
def test_the_jitter_term_of_a_doubled_region():
    mm = CC.Many()
    items = CC.oracle_items(mm)
    blocks = CC.blocks_of(items, mm.Xq)
    doubled = [r for r, (idx, _) in blocks.items() if np.any(np.diff(idx) == 0)]
    assert 88 in doubled and list(blocks[88][0]).count(89) == 2
    S_blocks = _ref_blocks(CC.FAMILIES["spline34"][1], mm.Xs, CC.SIGMA2["f64"], items, mm.Xq)
    jit, factors = {}, {}
    for r, (idx, S) in S_blocks.items():
        Sd = np.asarray(S, dtype=np.float64)
        jit[r] = 0.0
        if r in doubled:
            rung = [rel for rel in DE.ladder_rungs() if pivot_rule(Sd, rel * np.trace(Sd) / len(Sd)) == 0][0]
            jit[r] = rung * np.trace(Sd) / len(Sd)
            print("DRAWEDGEREF many: region %d passes at rel = %.3g, jitter %.3g" % (r, rung, jit[r]))
        factors[r] = DR.cholesky_psd_ld(np.asarray(S, dtype=LD) + LD(jit[r]) * np.eye(len(Sd), dtype=LD))
    A = DR.blend_matrix(items[:2], factors, items[2], mm.owth)
    W = DR.weight_matrix(items[:2], items[2], mm.owth)
    _, roff = DR.sorted_layout(items[:2])
    rows = np.unique(blocks[88][0])                                # the queries of region 88, query 89 among them
    assert 89 in rows and len(rows) >= 2
    want = CR.mix_cov_ref(items[:2], S_blocks, items[2], mm.owth)[rows]
    for r in doubled:
        Wr = W[:, roff[r]:roff[r] + len(S_blocks[r][0])]
        want = want + LD(jit[r]) * (Wr[rows] @ Wr.T)
    got = A[rows] @ A.T
    err = float(np.abs(got - want).max() / np.abs(want).max())
    pos = list(rows).index(89)
    w2 = W[89, roff[88]:roff[88] + len(S_blocks[88][0])]
    assert (w2 != 0).sum() == 2                                    # two weights in one factor: the cross term
    print("DRAWEDGEREF many: A A^T against Cov + jitter W W^T on %d rows: %.3g of the largest variance; entry (89, 89) %.6g"
          % (len(rows), err, float(got[pos, 89])))
    assert err <= 1e3 * float(np.finfo(LD).eps), err
    assert float(jit[88]) > 0


# ------------------------------------------------------------------------------------------ 4. the ladder without a device
class _Ctx:
    device = 0

    def synchronize(self):
        pass


class _Drawn(Exception):
    pass


def _standin(P, held, status):
    """a DeviceQuery that records what _sample_blocks asks of it; status(call, rel) -> finfo of the call-th factor_cov"""
    model = object.__new__(M.DeviceModel)          # no constructors: they would create device objects
    model.ctx, model.h, model.P, model.R = _Ctx(), None, P, 1
    q = object.__new__(M.DeviceQuery)
    q.model, q.L, q.h, q.Nq, q.total = model, None, None, 5, int(np.sum(held))
    log = dict(rel=[], blocks=[], draws=0)
    q.items_cov_blocks = lambda theta=None, multi=False: log["blocks"].append((theta, multi))
    q.region_offsets = lambda P_: np.concatenate([[0], np.cumsum(held)]).astype(np.int64)
    q.factor_cov = lambda rel=None: log["rel"].append(np.array(rel, dtype=np.float64))
    q.factor_info = lambda: (np.asarray(status(len(log["rel"]), log["rel"][-1]), dtype=np.int32), log["rel"][-1] * 1.0)

    def draw(*a, **k):
        log["draws"] += 1
        raise _Drawn()
    q.draw = draw
    return q, log


def _no_device_normals(monkeypatch):
    import torch
    monkeypatch.setattr(M, "_normals", lambda z, shape, dev, generator: torch.zeros(shape, dtype=torch.float64))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda dev=None: None)


def test_the_ladder_climbs_for_the_failed_regions_only_and_ends_naming_the_region(monkeypatch):
    _no_device_normals(monkeypatch)
    held = np.array([3, 2, 4, 1])
    # region 2 fails whatever rel is, region 1 on the first call only
    q, log = _standin(4, held, lambda call, rel: [0, 7 if call == 1 else 0, 2, 0])
    with pytest.raises(np.linalg.LinAlgError, match="region 2 "):
        M._sample_blocks(q, False, pmk.Spline34KernelType(1.0), 4, None, None, "samplemixtureGP")
    rungs = DE.ladder_rungs()
    rels = log["rel"]
    assert log["blocks"] == [(None, False)] and log["draws"] == 0
    assert len(rels) == 1 + len(rungs) and np.all(rels[0] == 0)
    assert rungs[0] == 2.0 ** -52 and all(b == 10.0 * a for a, b in zip(rungs, rungs[1:]))
    assert rungs[-1] <= 2.0 ** -26 < 10.0 * rungs[-1] and len(rungs) == 8          # 2^-52 x 10^7 <= 2^-26 < 2^-52 x 10^8
    for i, rel in enumerate(rels[1:]):
        assert rel[2] == rungs[i], (i, rel)
        assert rel[1] == 2.0 ** -52 and rel[0] == 0 and rel[3] == 0, (i, rel)
    print("DRAWEDGEREF ladder: %d rungs, the last 2^-52 x 10^%d = %.3g" % (len(rungs), len(rungs) - 1, rungs[-1]))


def test_the_ladder_stops_when_every_region_has_passed(monkeypatch):
    _no_device_normals(monkeypatch)
    held = np.array([3, 2, 4, 0])
    # region 1 passes at the second rung; region 3 is failed but holds no item of the batch: no refusal
    q, log = _standin(4, held, lambda call, rel: [0, 0 if rel[1] >= 10.0 * 2.0 ** -52 else 2, 0, -1])
    with pytest.raises(_Drawn):
        M._sample_blocks(q, False, pmk.Spline34KernelType(1.0), 4, None, None, "samplemixtureGP")
    assert [list(r) for r in log["rel"]] == [[0, 0, 0, 0], [0, 2.0 ** -52, 0, 0], [0, 10.0 * 2.0 ** -52, 0, 0]]
    assert log["draws"] == 1


@pytest.mark.parametrize("multi", [False, True])
def test_a_failed_patch_that_holds_items_is_refused_before_any_retry(monkeypatch, multi):
    _no_device_normals(monkeypatch)
    held = np.array([3, 2, 4, 1])
    q, log = _standin(4, held, lambda call, rel: [0, 5, 0, -1])       # region 1 would need the ladder, region 3 is failed
    with pytest.raises(np.linalg.LinAlgError, match="region 3 "):
        M._sample_blocks(q, multi, pmk.Spline34KernelType(1.0), 4, None, None, "samplemixtureGP_multi")
    assert len(log["rel"]) == 1 and np.all(log["rel"][0] == 0) and log["draws"] == 0 and log["blocks"] == [(None, multi)]
