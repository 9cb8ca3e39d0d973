"""The long-double restatement of block kriging (tests/_block_refs.py) pinned, on the CPU, to

1. a^T Cov a and a^T Yq of tests/_cov_multi_refs.py + tests/_cov_refs.py (the joint covariance under the blend, already
   pinned to the oracle), for trend none / constant / linear and R = 1 and 3;
2. the textbook form on a one-leaf tree, abar^T K** abar - kbar^T (K + sigma2 I)^-1 kbar through cho_solve;
3. the singleton identity: the variance of a one-query group with a = 1 is that query's Vq;

and the properties of the inputs of tests/test_gpu_block.py (tests/_block_cases.py) that its bounds rest on: kappa2(L) <= 10^3,
a plain numpy / LAPACK evaluation in the model's precision below one unit, and every aggregate's kappa - |Vbar|^2 at least
100 units above its floor.

The last one decides sigma2 of the fp32 cases (tests/_block_cases.py: 10, where the covariance tests use 0.05 and the margin
would be 0.18 to 0.58 units).  The GPU test also asserts on the device's own pieces that no aggregate of an accuracy case
sits on its floor.
"""
import numpy as np
import pytest
import scipy.linalg as sla

import _block_cases as BC
import _block_refs as BR
import _cov_cases as CC
import _cov_multi_cases as CMC
import _cov_multi_refs as CMR
import _cov_refs as CR

LD = CR.LD
_CACHE = {}


def _small():
    """the workload of tests/_cov_multi_cases.py (four leaves of 130 to 180 points), its first 120 queries in 3 + 1 + .. groups"""
    if "small" not in _CACHE:
        m = CMC.Main("f64")
        m.Xq = m.Xq[:120]
        items = CC.oracle_items(m)
        group = BC.cut(120, (3, 1, 7, 2, 20))
        a = np.random.default_rng(3).normal(0, 1, 120)
        _CACHE["small"] = (m, items, group, int(group[-1]) + 1, a)
    return _CACHE["small"]


@pytest.mark.parametrize("trend", [None, "constant", "linear"])
def test_the_aggregated_form_is_a_cov_a(trend):
    m, items, group, F, a = _small()
    oth = CC.FAMILIES["spline34"][1]
    refs = {r: CMR.TrendRegionRef(oth, m.Xs[r], CC.SIGMA2["f64"], trend) for r in range(4)}
    out = BR.block_ref(items[:2], items[2], m.owth, group, a, F, refs, m.Xq, CC.U_OF["f64"])
    blocks = CC.blocks_of(items, m.Xq)
    S = {r: (idx, refs[r].cov(xq)["S"]) for r, (idx, xq) in blocks.items()}
    # the dense route clamps the diagonal entry of every item; no item of this workload is clamped
    assert not any(refs[r].cov(xq)["clamped"].any() for r, (idx, xq) in blocks.items())
    Cov = CR.mix_cov_ref(items[:2], S, items[2], m.owth)
    A = np.zeros((F, len(m.Xq)), dtype=LD)
    A[group, np.arange(len(m.Xq))] = np.asarray(a, dtype=LD)
    want = np.einsum("fj,jk,fk->f", A, Cov, A)
    err = np.abs(np.asarray(out["Var"] - want, dtype=np.float64))
    assert np.all(err <= 1e-15 * np.abs(np.asarray(want, dtype=np.float64)) + 1e-18), err.max()
    assert np.all(np.asarray(out["Var"], dtype=np.float64) > 0)
    # the means, R = 1 and 3: a^T Yq with Yq the blend of the same item means
    wn = CR.blend_weights(items[0], items[2], m.owth)
    for R in (1, 3):
        U = np.random.default_rng(R).normal(0, 1, (len(items[1]), R))
        Yq = np.zeros((len(m.Xq), R), dtype=LD)
        np.add.at(Yq, out["query_of"], wn[:, None] * np.asarray(U, dtype=LD))
        mean = BR.block_ref(items[:2], items[2], m.owth, group, a, F, refs, m.Xq, CC.U_OF["f64"], item_means=U)["Mean"]
        assert np.all(np.abs(np.asarray(mean - A @ Yq, dtype=np.float64)) <= 1e-16 * (np.abs(A) @ np.abs(Yq)).astype(np.float64) + 1e-18)


def test_the_textbook_form_on_a_one_leaf_tree():
    rng = np.random.default_rng(11)
    X = rng.uniform(-2, 2, (60, 2))
    Xq = rng.uniform(-2, 2, (9, 2))
    sigma2 = 1e-2
    oth = CC.FAMILIES["gaussian"][1]
    group = np.array([0, 0, 0, 0, 1, 1, 1, 1, 1])
    a = rng.normal(0, 1, 9)
    items = (np.arange(10), np.zeros(9, dtype=np.int64), np.zeros(9))
    refs = {0: CMR.TrendRegionRef(oth, X, sigma2, None)}
    out = BR.block_ref(items[:2], items[2], CC.FAMILIES["spline34"][1], group, a, 2, refs, Xq, CC.U_OF["f64"])
    K = np.asarray(CR.kern(oth, X, X), dtype=np.float64) + sigma2 * np.eye(60)
    Kq = np.asarray(CR.kern(oth, X, Xq), dtype=np.float64)
    Kqq = np.asarray(CR.kern(oth, Xq, Xq), dtype=np.float64)
    cf = sla.cho_factor(K, lower=True)
    for f in (0, 1):
        ab = np.where(group == f, a, 0.0)
        kb = Kq @ ab
        want = ab @ Kqq @ ab - kb @ sla.cho_solve(cf, kb)
        assert abs(float(out["Var"][f]) - want) <= 1e-10 * abs(ab @ Kqq @ ab), (f, float(out["Var"][f]), want)


@pytest.mark.parametrize("trend", [None, "linear"])
def test_a_singleton_group_answers_the_querys_vq(trend):
    m, items, _, _, _ = _small()
    Nq = len(m.Xq)
    oth = CC.FAMILIES["spline34"][1]
    refs = {r: CMR.TrendRegionRef(oth, m.Xs[r], CC.SIGMA2["f64"], trend) for r in range(4)}
    off, reg = items[0], items[1]
    # Vq is the sum of the items' variances: equal to the block variance where no query holds two items of one region
    single = np.array([len(set(reg[off[j]:off[j + 1]])) == off[j + 1] - off[j] for j in range(Nq)])
    assert single.all()
    out = BR.block_ref(items[:2], items[2], m.owth, np.arange(Nq), np.ones(Nq), Nq, refs, m.Xq, CC.U_OF["f64"])
    wn = CR.blend_weights(off, items[2], m.owth)
    Vq = np.zeros(Nq, dtype=LD)
    for r, (idx, xq) in CC.blocks_of(items, m.Xq).items():
        sel = np.nonzero(reg == r)[0]
        np.add.at(Vq, idx, wn[sel] ** 2 * np.diag(refs[r].cov(xq)["S"]))
    assert np.all(np.abs(np.asarray(out["Var"] - Vq, dtype=np.float64)) <= 1e-17 + 1e-16 * np.asarray(Vq, dtype=np.float64))


# ------------------------------------------------------------------------------------------ the inputs of the GPU tests
def main_case(dtype, family, trend):
    """the reference of one case of the main workload, shared with tests/test_gpu_block.py -> (workload, items, refs, out)"""
    key = ("main", dtype, family, trend)
    if key not in _CACHE:
        if ("w", dtype) not in _CACHE:
            m = BC.Main(dtype)
            _CACHE[("w", dtype)] = (m, CC.oracle_items(m))
        m, items = _CACHE[("w", dtype)]
        oth = CC.FAMILIES[family][1]
        refs = {r: CMR.TrendRegionRef(oth, m.Xs[r], BC.SIGMA2[dtype], trend) for r in range(4)}
        out = BR.block_ref(items[:2], items[2], m.owth, m.group, m.a, m.F, refs, m.Xq, CC.U_OF[dtype])
        _CACHE[key] = (m, items, refs, out)
    return _CACHE[key]


MAIN_CASES = [(d, f, t) for d in ("f64", "f32") for f in ("spline34", "gaussian") for t, _ in BC.TREND_R]


@pytest.mark.parametrize("dtype,family,trend", MAIN_CASES)
def test_main_inputs_are_well_conditioned_and_a_plain_evaluation_stays_below_one_unit(dtype, family, trend):
    m, items, refs, out = main_case(dtype, family, trend)
    assert all(272 <= len(x) <= 298 for x in m.Xs) and len(m.Xq) == 700
    assert max(r.kappa for r in refs.values()) <= CC.KAPPA_MAX
    counts = sorted(set(a["count"] for a in out["aggs"]))
    assert counts[0] == 1 and counts[-1] == 65, counts
    # an aggregate of 65 members next to one of a single member, in one region
    assert any(x["region"] == y["region"] and x["count"] == 65 and y["count"] == 1 for x, y in zip(out["aggs"], out["aggs"][1:]))
    T_ = np.float64 if dtype == "f64" else np.float32
    oth = CC.FAMILIES[family][1]
    plain = BR.plain_block_var(items[:2], items[2], m.owth, m.group, m.a, m.F, [oth] * 4, m.Xs, BC.SIGMA2[dtype], trend, m.Xq, T_)
    ratio = np.abs(plain - np.asarray(out["Var"], dtype=np.float64)) / out["unit"]
    print("BLOCKREF", dtype, family, trend, "plain / unit", float(ratio.max()))
    assert ratio.max() < 1.0, ratio.max()


@pytest.mark.parametrize("dtype,family,trend", MAIN_CASES)
def test_every_aggregate_clears_its_floor_by_100_units(dtype, family, trend):
    """fp64: 8.8e6 units and more; fp32 with sigma2 = 10: 154 (spline34, linear) to 674 (gaussian, none) units"""
    _, _, _, out = main_case(dtype, family, trend)
    worst = min(a["margin"] for a in out["aggs"])
    print("BLOCKREF", dtype, family, trend, "least margin in units", worst)
    assert worst >= BC.MARGIN_MIN, worst


def edge_case(D, dtype):
    """the inputs and the reference of one strip-and-patch-edge case, shared with tests/test_gpu_block.py"""
    key = ("edge", D, dtype)
    if key not in _CACHE:
        root, Xs, Xq, group, a, home = BC.edge_queries(D, dtype)
        items = BC.edge_items(home)
        oth = CC.FAMILIES["spline34"][1]
        refs = {r: CMR.TrendRegionRef(oth, Xs[r], BC.SIGMA2[dtype], None) for r in sorted(set(home.tolist()))}
        F = int(group[-1]) + 1
        out = BR.block_ref(items[:2], items[2], CC.FAMILIES["spline34"][1], group, a, F, refs, Xq, CC.U_OF[dtype])
        _CACHE[key] = (root, Xs, Xq, group, a, home, items, refs, out)
    return _CACHE[key]


@pytest.mark.parametrize("D,dtype", [(1, "f64"), (2, "f64"), (4, "f64"), (2, "f32")])
def test_edge_inputs(D, dtype):
    root, Xs, Xq, group, a, home, items, refs, out = edge_case(D, dtype)
    assert [int(np.sum(home == r)) > 0 for r in range(8)] == [c > 0 for c in BC.EDGE_AGGS]
    assert [sum(1 for x in out["aggs"] if x["region"] == k) for k in range(8)] == list(BC.EDGE_AGGS)
    assert np.all(np.diff(group) >= 0) and [len(x) for x in Xs] == CC.EDGE_SIZES
    assert max(r.kappa for r in refs.values()) <= CC.KAPPA_MAX
    worst = min(x["margin"] for x in out["aggs"])
    T_ = np.float64 if dtype == "f64" else np.float32
    oth = CC.FAMILIES["spline34"][1]
    plain = BR.plain_block_var(items[:2], items[2], oth, group, a, int(group[-1]) + 1, [oth] * 8, Xs, BC.SIGMA2[dtype], None, Xq, T_)
    ratio = float((np.abs(plain - np.asarray(out["Var"], dtype=np.float64)) / out["unit"]).max())
    print("BLOCKREF edges", D, dtype, "least margin in units", worst, "plain / unit", ratio)
    assert worst >= BC.MARGIN_MIN and ratio < 1.0, (worst, ratio)
